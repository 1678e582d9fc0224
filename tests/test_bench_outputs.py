"""bench.py's plain run, --full switch and --dump-outputs: the sampling plan and the writer on the
CPU, one tiny plain run with --dump-outputs on the GPU (the dumped arrays are what a solve of the
same seeded windows returns)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from _paths import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402

FULL_ONLY_KEYS = ("gather", "per_solve_incl_pcie", "single_window", "roofline", "kernels", "survey_8d",
                  "cpu_baseline", "accuracy")


def test_full_and_dump_are_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "d", "--no-cpu"])
    assert a.full is True and a.dump_outputs == "d" and a.no_cpu is True


@pytest.mark.parametrize("n_windows,config", [(4, "s10"), (2048, "s50"), (2048, "s10"), (300000, "s50")])
def test_dump_plan_is_fixed_and_within_budget(n_windows, config):
    cfg = bench.CONFIGS[config]
    win, lm = bench.dump_plan(n_windows, cfg)
    win2, lm2 = bench.dump_plan(n_windows, cfg)
    for a, b in ((win, win2), (lm, lm2)):  # the same sample in every run
        assert (a is None and b is None) or np.array_equal(a, b)
    n_win = n_windows if win is None else len(win)
    n_lm = cfg["n_lm"] if lm is None else len(lm)
    assert n_win >= 1 and n_lm >= 1
    for idx, n in ((win, n_windows), (lm, cfg["n_lm"])):
        if idx is not None:
            assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    total = 8 * n_win * (cfg["n_kf"] * 16 + len(bench.SUMMARY_COLS) + n_lm * 4)
    total += 8 * (n_win if win is not None else 0) + 8 * (n_lm if lm is not None else 0)
    assert total <= 64 * 1000 * 1000
    if n_windows == 4:
        assert win is None and lm is None  # a small job is written whole
    if (n_windows, config) == (2048, "s50"):
        assert win is None and 0 < len(lm) < cfg["n_lm"]


def test_dump_outputs_writes_float64_npy(tmp_path):
    d = tmp_path / "out" / "nested"
    n = bench.dump_outputs(str(d), {"a": np.arange(6, dtype=np.int64).reshape(2, 3), "b": np.ones(4, dtype=np.float32)})
    assert n == 10 * 8 and sorted(os.listdir(d)) == ["a.npy", "b.npy"]
    a = np.load(d / "a.npy")
    assert a.dtype == np.float64 and a.shape == (2, 3) and np.array_equal(a, np.arange(6).reshape(2, 3))
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(d), {"big": np.zeros(64 * 1000 * 1000 // 8 + 1)})


@pytest.mark.gpu
def test_plain_run_dumps_what_the_solve_returns(og, gpu_ctx, tmp_path):
    """A plain run prints the headline line without the --full legs, runs exactly --steps timed
    steps, and --dump-outputs holds the results of that solve: the same seeded windows solved here
    through the C ABI give the same summaries and parameters. Bounds: two runs of the GPU path are
    each held to 1e-7 (relative cost) and 1e-6 m (positions) against the oracle by the parity
    suite, so they differ from each other by at most twice that."""
    n_win, steps, warmup = 4, 3, 1
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "s10",
                        "--windows", str(n_win), "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "window-iterations/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - n_win * 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    assert not [k for k in FULL_ONLY_KEYS if k in line]

    cfg = bench.CONFIGS["s10"]
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["landmarks", "poses", "speed_biases", "summary"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["summary"].shape == (n_win, len(bench.SUMMARY_COLS))
    assert got["poses"].shape == (n_win, cfg["n_kf"], 7) and got["speed_biases"].shape == (n_win, cfg["n_kf"], 9)
    assert got["landmarks"].shape == (n_win, cfg["n_lm"], 4)
    col = {k: i for i, k in enumerate(bench.SUMMARY_COLS)}
    assert np.array_equal(got["summary"][:, col["window"]], np.arange(n_win))
    assert np.all(got["summary"][:, col["num_iterations"]] == steps + warmup)

    ws = bench.make_windows(cfg, range(n_win))
    gpu_ctx.set_problems([w.problem for w in ws])
    sums = gpu_ctx.solve(bench.bench_options(steps + warmup))
    for i, (w, s) in enumerate(zip(ws, sums)):
        assert s["num_iterations"] == steps + warmup
        assert abs(got["summary"][i, col["final_cost"]] - s["final_cost"]) <= 2e-7 * s["final_cost"]
        assert abs(got["summary"][i, col["initial_cost"]] - s["initial_cost"]) <= 2e-7 * s["initial_cost"]
        assert np.abs(got["poses"][i, :, :3] - w.poses()[:, :3]).max() <= 2e-6
    # the solve moved the parameters: the dump is the result, not the seeded start
    ws[0].reset()
    assert np.abs(got["poses"][0, :, :3] - ws[0].poses()[:, :3]).max() > 1e-4
