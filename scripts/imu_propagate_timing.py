"""Wall time of okvisgpu_imu_propagate for N items of S samples (default 2,048 x 21: one 0.1 s
keyframe interval at 200 Hz each), without and with the covariance and Jacobian: warm-up calls, then
the median (and the quartiles) of REPS calls, each timed by a host clock around the call, which
returns after a stream synchronise with the results in the caller's arrays. One JSON line. Kernel
(device) time comes from a kernel trace of this script in a run of its own (few REPS).
Usage: imu_propagate_timing.py [N [S [REPS]]]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "okvis2-x_amd"))
import okvisgpu as og  # noqa: E402

n, s, reps = (int(x) for x in (sys.argv[1:] + ["2048", "21", "50"][len(sys.argv) - 1:]))
rng = np.random.default_rng(2048)
ip = og.ImuParams()
ip.a_max, ip.g_max = 176.0, 7.8
ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c = 12.0e-4, 8.0e-3, 4.0e-6, 4.0e-5
ip.g = 9.81007
rate = 5_000_000
base = 1_000_000_000 + rng.integers(0, rate, n)
ts = (base[:, None] + np.arange(s, dtype=np.int64)[None, :] * rate).astype(np.int64)
t0 = ts[:, 0] + rng.integers(0, rate, n)
t1 = ts[:, -1] - rng.integers(0, rate, n)
ga = np.concatenate([rng.uniform(-1, 1, (n, 1, 3)) + 0.2 * rng.normal(size=(n, s, 3)),
                     np.array([0.0, 0.0, 9.81]) + 0.5 * rng.normal(size=(n, s, 3))], axis=2)
q = rng.normal(size=(n, 4))
poses0 = np.hstack([rng.uniform(-5, 5, (n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)])
sbs0 = np.hstack([rng.uniform(-2, 2, (n, 3)), rng.uniform(-0.02, 0.02, (n, 3)), rng.uniform(-0.1, 0.1, (n, 3))])
begin = np.arange(n + 1, dtype=np.int32) * s

ctx = og.Context(0)
out = {"items": n, "samples_per_item": s, "reps": reps}
for name, mats in (("pose_speed", False), ("covariance_jacobian", True)):
    P = np.zeros((n, 15, 15)) if mats else None
    J = np.zeros((n, 15, 15)) if mats else None
    b, keep = og.imu_propagate_batch(ip, poses0.copy(), sbs0.copy(), t0, t1, begin, ts.reshape(-1), ga.reshape(-1, 6), P, J)
    steps = np.zeros(n, np.int32)
    sp = steps.ctypes.data_as(og.C.POINTER(og.C.c_int32))
    wall = []
    for r in range(5 + reps):
        keep[-4][:] = poses0
        keep[-3][:] = sbs0
        a = time.perf_counter()
        rc = og.lib().okvisgpu_imu_propagate(ctx.h, og.C.byref(b), sp)
        wall.append((time.perf_counter() - a) * 1e3)
        assert rc == 0 and (steps == s - 1).all()
    w = np.sort(wall[5:])
    out[name] = {"wall_ms_median": float(np.median(w)), "wall_ms_q1": float(w[len(w) // 4]),
                 "wall_ms_q3": float(w[(3 * len(w)) // 4])}
ctx.close()
print(json.dumps(out))
