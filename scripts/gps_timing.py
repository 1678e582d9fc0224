"""Time of okvisgpu_gps_evaluate (kind 0, fresh factors with a returned state, every output) at 64, 1,024
and 16,384 factors of 12 samples (a 20 Hz frame interval at 200 Hz) and of 45 samples.

Wall time: warm-up calls, then the median (and the quartiles) of REPS calls, each timed by a host clock
around the C call, which returns after a stream synchronise with the results in the caller's arrays
(allocated once; the state is zeroed before every call, outside the clock, so that every call
re-integrates), profiler off. Device time: a rocprofv3 kernel trace of this script in a child process of
its own (--child: 3 warm-up + 10 calls per shape, then the same with the four-matrix recursion,
OKVISGPU_GPS_FOUR_P=1), per shape the average / min / max of the kernel's duration; the staging share of a
call is its wall time minus that. Beside it the single-thread C++ port of the restatement
(scripts/gps_port.cpp, built with g++ -O2 when scripts/gps_port is missing) on the same inputs and the
same host: the port, not the reference; its sums of r and of the Jacobians stand next to the device's.
Writes the JSON to --out (default profiles/gps_timing.json) and prints it.
Usage: gps_timing.py [--out PATH] [--reps N] [--no-trace] [--trace-dir DIR]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "okvis2-x_amd"))
import okvisgpu as og  # noqa: E402

C = og.C
RATE = 5_000_000
SHAPES = [(n, s) for s in (12, 45) for n in (64, 1024, 16384)]
CHILD_WARM, CHILD_REPS = 3, 10
R_SA = np.array([0.05, -0.02, 0.1])


def params():
    ip = og.ImuParams()
    ip.a_max, ip.g_max = 176.0, 7.8
    ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c = 12.0e-4, 8.0e-3, 4.0e-6, 4.0e-5
    ip.g = 9.81007
    return ip


def make(n, ns, rng):
    """n factors of ns samples on a 200 Hz grid, t_k inside the first interval, t_g inside the last."""
    def unit(k):
        q = rng.normal(size=(k, 4))
        return q / np.linalg.norm(q, axis=1, keepdims=True)

    base = 1_000_000_000 + rng.integers(0, RATE, n)
    ts = (base[:, None] + np.arange(ns, dtype=np.int64)[None, :] * RATE).astype(np.int64)
    t_k = ts[:, 0] + rng.integers(0, RATE, n)
    t_g = ts[:, -1] - rng.integers(0, RATE, n)
    ga = np.concatenate([rng.uniform(-1, 1, (n, 1, 3)) + 0.2 * rng.normal(size=(n, ns, 3)),
                         np.array([0.0, 0.0, 9.81]) + 0.5 * rng.normal(size=(n, ns, 3))], axis=2)
    poses = np.hstack([rng.uniform(-5, 5, (n, 3)), unit(n)])
    sb = np.hstack([rng.uniform(-2, 2, (n, 3)), rng.uniform(-0.02, 0.02, (n, 3)), rng.uniform(-0.1, 0.1, (n, 3))])
    T_GW = np.hstack([rng.normal(0.0, 2.0, (2, 3)), unit(2)])
    info = np.zeros((n, 3, 3))
    info[:, [0, 1, 2], [0, 1, 2]] = rng.uniform(0.05, 0.5, (n, 3)) ** -2.0
    return dict(poses=poses, T_GW=T_GW, measurement=poses[:, :3] + rng.normal(0.0, 0.5, (n, 3)), information=info,
                speed_biases=sb, t_k=t_k, t_g=t_g, sample_begin=np.arange(n + 1, dtype=np.int32) * ns,
                sample_t=ts.reshape(-1), sample_ga=ga.reshape(-1, 6), gw_index=rng.integers(0, 2, n).astype(np.int32))


class Call:
    """One shape's batch, state and outputs, allocated once."""

    def __init__(self, ctx, a):
        self.ctx, self.n = ctx, len(a["poses"])
        self.state = np.zeros((self.n, og.GPS_STATE_DOUBLES))
        self.b, self.keep = og.gps_batch(params(), R_SA, state=self.state, **a)
        self.out = {k: np.zeros((self.n,) + shape, dtype=np.int32 if k == "steps" else np.float64)
                    for k, shape in og.GPS_OUTPUTS.items()}
        self.r = og.GpsResult()
        og._set_arrays(self.r, self.out)
        self.bytes_up = int(sum(v.nbytes for v in self.keep.values()))
        self.bytes_down = int(self.state.nbytes + sum(v.nbytes for v in self.out.values()))

    def __call__(self):
        self.state[:] = 0.0
        a = time.perf_counter()
        rc = og.lib().okvisgpu_gps_evaluate(self.ctx.h, C.byref(self.b), C.byref(self.r))
        ms = (time.perf_counter() - a) * 1e3
        assert rc == 0 and (self.state[:, 0] == 1).all()
        return ms


def write_port_input(path, a):
    n = len(a["poses"])
    ip = params()
    with open(path, "wb") as f:
        np.array([n, len(a["sample_t"])], np.int64).tofile(f)
        np.array([ip.a_max, ip.g_max, ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c, ip.g, *R_SA]).tofile(f)
        for v in (a["poses"], a["speed_biases"], a["T_GW"][a["gw_index"]], a["measurement"], a["information"]):
            np.ascontiguousarray(v, dtype=np.float64).tofile(f)
        for v in (a["t_k"], a["t_g"], a["sample_begin"], a["sample_t"]):
            np.ascontiguousarray(v, dtype=np.int64).tofile(f)
        np.ascontiguousarray(a["sample_ga"], dtype=np.float64).tofile(f)


def child():
    """The traced run: per shape CHILD_WARM + CHILD_REPS calls folded, then as many with four matrices."""
    rng = np.random.default_rng(16384)
    ctx = og.Context(0)
    for n, ns in SHAPES:
        call = Call(ctx, make(n, ns, rng))
        for four in ("0", "1"):
            os.environ["OKVISGPU_GPS_FOUR_P"] = four
            for _ in range(CHILD_WARM + CHILD_REPS):
                call()
    ctx.close()


def kernel_times(trace_dir):
    """The k_gps_async rows of the child's kernel trace, in launch order, cut into the child's groups."""
    env = dict(os.environ)
    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "-o", "run", "--",
                    sys.executable, os.path.abspath(__file__), "--child"], check=True, env=env, timeout=600)
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                  for r in csv.DictReader(open(files[0])) if "k_gps_async" in r["Kernel_Name"])
    per = CHILD_WARM + CHILD_REPS
    assert len(rows) == 2 * per * len(SHAPES), len(rows)
    out = {}
    for i, (n, ns) in enumerate(SHAPES):
        for j, variant in enumerate(("folded", "four_matrices")):
            grp = rows[(2 * i + j) * per + CHILD_WARM:(2 * i + j + 1) * per]
            assert all((", 1>" in name) == (variant == "folded") for _, _, name in grp), grp[0][2]
            d = [e - s for s, e, _ in grp]
            out.setdefault(f"{n}x{ns}", {})[variant] = {"calls": len(d), "avg_ns": int(np.mean(d)), "min_ns": min(d),
                                                         "max_ns": max(d)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "gps_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()

    port = os.path.join(HERE, "gps_port")
    if not os.path.exists(port):
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(HERE, "gps_port.cpp"), "-o", port], check=True)
    rng = np.random.default_rng(16384)
    ctx = og.Context(0)
    result = {"what": "scripts/gps_timing.py: okvisgpu_gps_evaluate, kind 0, fresh factors, state returned, every output",
              "reps": args.reps, "shapes": {}}
    for n, ns in SHAPES:
        a = make(n, ns, rng)
        call = Call(ctx, a)
        wall = np.sort([call() for _ in range(5 + args.reps)][5:])
        entry = {"factors": n, "samples": ns, "wall_ms_median": float(np.median(wall)), "wall_ms_q1": float(wall[len(wall) // 4]),
                 "wall_ms_q3": float(wall[(3 * len(wall)) // 4]), "bytes_up": call.bytes_up, "bytes_down": call.bytes_down,
                 "sum_r": float(call.out["r"].sum()),
                 "sum_J": float(call.out["J_pose"].sum() + call.out["J_speed_bias"].sum() + call.out["J_T_GW"].sum())}
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "in.bin")
            write_port_input(path, a)
            entry["cpu_port"] = json.loads(subprocess.run([port, path, "5" if n * ns < 200_000 else "3"], capture_output=True,
                                                          text=True, check=True).stdout)
        result["shapes"][f"{n}x{ns}"] = entry
    ctx.close()
    if not args.no_trace:
        with tempfile.TemporaryDirectory() as tmp:
            kt = kernel_times(args.trace_dir or tmp)
        folds = []
        for key, k in kt.items():
            e = result["shapes"][key]
            e["kernel_ns"] = k
            e["staging_ms"] = e["wall_ms_median"] - k["folded"]["avg_ns"] * 1e-6
            folds.append(k["four_matrices"]["avg_ns"] / k["folded"]["avg_ns"])
        result["fold"] = {"four_matrices_over_folded_kernel_time": {k: round(f, 3) for k, f in zip(kt, folds)},
                          "pays": bool(min(folds) > 1.0)}
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
