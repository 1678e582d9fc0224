"""What the batch size decides about a solve's launches (okvisgpu_launch_regime; plan.cpp
launchRegime): few / many windows, one-stream or forked graph, where the GN prep and the gradient
test run, iterations per captured graph and the Cholesky schedule with its fallbacks. Integer logic,
so the expected values are written out by hand from the rules and checked without a
device: through the library's entry point, and by tests/cpp/launch_regime_check, the same function
compiled for the host with -fsanitize=address,undefined, over the same table."""
import os
import subprocess

import pytest

from _paths import REPO

KEYS = ("few", "many", "serial_graph", "lin_prep", "fused_gradnorm", "graph_iters", "chol_schedule")


def _case(n, cu, want, split=0, persistent=1, pipe=1, schedule=0, serial=-1, prep=-1, iters=-1):
    return (n, cu, split, persistent, pipe, schedule, serial, prep, iters), want


# (n, cu): few, many, serial_graph, lin_prep, fused_gradnorm, graph_iters, schedule without / with a split
BATCH = [
    (1, 256, (1, 0, 1, 1, 1, 4), 2, 2),    # 2n < cu: tile-parallel
    (64, 256, (1, 1, 1, 1, 1, 4), 2, 2),   # 4n == cu: still few; n == 64: many
    (65, 256, (0, 1, 1, 0, 0, 4), 2, 2),   # 4n > cu: not few, so no prep in the linearisation, no fused test
    (127, 256, (0, 1, 1, 0, 0, 4), 2, 2),
    (128, 256, (0, 1, 1, 0, 0, 4), 4, 5),  # 2n == cu: split pipelined with a split, else pipelined
    (129, 256, (0, 1, 1, 0, 0, 4), 4, 4),
    (255, 256, (0, 1, 1, 0, 0, 4), 4, 4),
    (256, 256, (0, 1, 0, 0, 0, 4), 4, 4),  # n == cu: forked graph, still pipelined
    (257, 256, (0, 1, 0, 0, 0, 4), 1, 1),  # n > cu: persistent
    (8, 32, (1, 0, 1, 1, 1, 4), 2, 2),
    (9, 32, (0, 0, 1, 0, 0, 4), 2, 2),
    (16, 32, (0, 0, 1, 0, 0, 4), 4, 5),
    (32, 32, (0, 0, 0, 0, 0, 4), 4, 4),
]

# requested schedule -> {(split, persistent fits, pipe fits): resolved}; fallbacks in order: 3 without
# a split -> 1, 5 without a split -> 4, 5 without both fits -> 3, 4 without the pipe fit -> 1, 1 or 3
# without the persistent fit -> 2
REQUESTED = {
    1: {(0, 0, 0): 2, (0, 0, 1): 2, (0, 1, 0): 1, (0, 1, 1): 1, (1, 0, 0): 2, (1, 0, 1): 2, (1, 1, 0): 1, (1, 1, 1): 1},
    2: {(0, 0, 0): 2, (0, 0, 1): 2, (0, 1, 0): 2, (0, 1, 1): 2, (1, 0, 0): 2, (1, 0, 1): 2, (1, 1, 0): 2, (1, 1, 1): 2},
    3: {(0, 0, 0): 2, (0, 0, 1): 2, (0, 1, 0): 1, (0, 1, 1): 1, (1, 0, 0): 2, (1, 0, 1): 2, (1, 1, 0): 3, (1, 1, 1): 3},
    4: {(0, 0, 0): 2, (0, 0, 1): 4, (0, 1, 0): 1, (0, 1, 1): 4, (1, 0, 0): 2, (1, 0, 1): 4, (1, 1, 0): 1, (1, 1, 1): 4},
    # 5 with a split and no persistent fit: 5 -> 3 -> 2, whatever the pipe fit
    5: {(0, 0, 0): 2, (0, 0, 1): 4, (0, 1, 0): 1, (0, 1, 1): 4, (1, 0, 0): 2, (1, 0, 1): 2, (1, 1, 0): 3, (1, 1, 1): 5},
}


def _table():
    t = []
    for n, cu, flags, s0, s1 in BATCH:
        t.append(_case(n, cu, flags + (s0,), split=0))
        t.append(_case(n, cu, flags + (s1,), split=1))
    for req, by in REQUESTED.items():
        for (split, persistent, pipe), sched in by.items():  # 300 windows on 256 CUs: many, forked
            t.append(_case(300, 256, (0, 1, 0, 0, 0, 4, sched), split=split, persistent=persistent, pipe=pipe,
                           schedule=req))
    # the measurement overrides
    t.append(_case(1, 256, (1, 0, 0, 1, 0, 4, 2), serial=0))    # forked: no fused test, the prep placement stays
    t.append(_case(1, 256, (1, 0, 1, 1, 1, 4, 2), serial=1))
    t.append(_case(300, 256, (0, 1, 1, 0, 0, 4, 1), serial=1))  # one stream, not few: nothing fused
    t.append(_case(300, 256, (0, 1, 0, 0, 0, 4, 1), serial=0))
    t.append(_case(1, 256, (1, 0, 1, 0, 1, 4, 2), prep=0))      # few: the prep as its own launch
    t.append(_case(65, 256, (0, 1, 1, 0, 0, 4, 2), prep=0))     # not few: never on
    for iters, k in ((0, 1), (1, 1), (8, 8), (1000, 64)):
        t.append(_case(3, 256, (1, 0, 1, 1, 1, k, 2), iters=iters))
    return t


TABLE = _table()


def test_table_covers_the_issue():
    assert len(TABLE) == 2 * len(BATCH) + 5 * 8 + 10 and len({c for c, _ in TABLE}) == len(TABLE)


@pytest.mark.parametrize("case,want", TABLE, ids=[" ".join(map(str, c)) for c, _ in TABLE])
def test_launch_regime(og, case, want):
    n, cu, split, persistent, pipe, schedule, serial, prep, iters = case
    got = og.launch_regime(n, cu, any_split=split, persistent_fits=persistent, pipe_fits=pipe, schedule=schedule,
                           serial_graph=serial, lin_prep=prep, graph_iters=iters)
    assert got == dict(zip(KEYS, want))


def test_launch_regime_under_host_sanitizers():
    """The same table through the stand-alone program built with -fsanitize=address,undefined
    (tests/cpp/launch_regime_check: plan.cpp compiled for the host, no device, no library)."""
    cpp = os.path.join(REPO, "tests", "cpp")
    r = subprocess.run(["make", "-C", cpp, "launch_regime_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = "".join(" ".join(map(str, c + w)) + "\n" for c, w in TABLE)
    r = subprocess.run([os.path.join(cpp, "launch_regime_check")], input=rows, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"launch_regime_check ok: {len(TABLE)} cases" in r.stdout
