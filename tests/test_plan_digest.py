"""The planner's output, pinned bit for bit (okvisgpu_plan_digest; plan.cpp analyse + layoutArena).

Every array the planner uploads is hashed (FNV-1a-64) in the arena table's order, next to every
entry's name, region and byte count and the plan's scalar totals, and compared with
tests/golden/plan_digest.json. The fixture was recorded from the commit before the planner became
its own translation unit (analyse() inside runtime.cpp, hashed in the order of that build()'s
uploads), so a change that must not alter the plan proves it here, on the CPU. A change that is
meant to alter the plan regenerates the fixture (`python tests/test_plan_digest.py`) and says so.

The cases are the smallest that reach every branch of the planner; cu_count is an argument, so the
batch-dependent choices (nested dissection, group sizes, light assembly) need no large batch."""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digest.json")
S10, S50 = (10, 500, 4000), (50, 2000, 16000)


def _s10(og):
    return [og.SynthWindow(*S10, seed=20251015)]


def _s50(og):
    return [og.SynthWindow(*S50, seed=20251015)]


def _batch70(og):
    # >= kManyWindows (light assembly lists) and >= 8 (XCD interleave); nd on at 256 CUs, off at 32
    shapes = [S10, (6, 150, 1000), (20, 800, 6000)]
    return [og.SynthWindow(*shapes[i % 3], seed=1 + i) for i in range(70)]


def _extrinsics(og, frozen):
    w = og.SynthWindow(*S10, seed=51, do_extrinsics=1)
    if frozen:
        w.problem.extrinsics_constant[1] = 1
    return [w]


def _gps(og):
    from _gps import gps_window
    return [gps_window(seed=7)[0]]


def _loss(og):
    from _submap import loss_window
    return [loss_window()[0]]


def _constants(og):
    w = og.SynthWindow(*S10, seed=20251015)
    p = w.problem
    p.pose_constant[0] = p.pose_constant[1] = 1
    for l in range(0, p.n_landmarks, 5):
        p.landmark_constant[l] = 1
    p.speed_bias_constant[0] = 1
    return [w]


# name -> (builder, builder key shared between cases, cu_count)
CASES = {
    "s10": (_s10, "s10", 256),
    "s50": (_s50, "s50", 256),
    "batch70_cu256": (_batch70, "batch70", 256),
    "batch70_cu32": (_batch70, "batch70", 32),
    "extrinsics": (lambda og: _extrinsics(og, False), "extrinsics", 256),
    "extrinsics_frozen": (lambda og: _extrinsics(og, True), "extrinsics_frozen", 256),
    "gps": (_gps, "gps", 256),
    "loss": (_loss, "loss", 256),
    "constants": (_constants, "constants", 256),
}
_built = {}


def _digest(og, name):
    build, key, cu = CASES[name]
    if key not in _built:
        _built[key] = build(og)
    problems = [getattr(w, "struct", None) or w.problem for w in _built[key]]
    return og.plan_digest(problems, cu)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_digest(og, golden, name):
    got, want = _digest(og, name), golden[name]
    assert got["totals"] == want["totals"]
    assert [e[:3] for e in got["entries"]] == [e[:3] for e in want["entries"]]  # name, region, bytes
    diff = [g[0] for g, w in zip(got["entries"], want["entries"]) if g[3] != w[3]]
    assert not diff, f"arrays whose bytes differ from the recorded plan: {diff}"


def test_cases_reach_the_branches(og, golden):
    """The fixture itself shows the branches the cases are there for."""
    t = {k: v["totals"] for k, v in golden.items()}
    size = {k: {e[0]: e[2] for e in v["entries"]} for k, v in golden.items()}
    assert t["s50"]["any_split"] == 1 and t["batch70_cu32"]["any_split"] == 0
    assert size["batch70_cu32"]["asm_ppl_items"] > 0 and size["s10"]["asm_ppl_items"] == 0
    assert size["extrinsics"]["xvisit_pose"] > size["extrinsics_frozen"]["xvisit_pose"] > 0
    assert size["extrinsics"]["pe_pose"] > 0 and size["s10"]["pe_pose"] == 0
    assert size["gps"]["host_in"] > 0 and size["loss"]["host_in"] > size["gps"]["host_in"]
    assert size["constants"]["fb_win"] < size["s10"]["fb_win"]
    assert all(v["obs_iso"] == 1 for v in t.values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _paths  # noqa: F401
    import okvisgpu

    out = {name: _digest(okvisgpu, name) for name in CASES}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {GOLDEN}: {len(out)} cases")
