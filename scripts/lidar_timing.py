"""Wall time of okvisgpu_lidar_deskew and okvisgpu_voxel_downsample: warm-up calls, then the median (and
the quartiles) of REPS calls, each timed by a host clock around the C call, which returns after a stream
synchronise with the results in the caller's arrays (allocated once). Shapes: one scan of Q queries
(LiDAR points) over S IMU samples (default 65,536 x 41: 0.2 s at 200 Hz) with the deskewing outputs
(valid, float point) and with the getStates outputs (valid, pose, speed, omega_S; no rays); 64 such
scans in one call; the voxel downsampling of the first scan's deskewed points at 0.05 m. With each
shape the bytes staged up and down. Beside it the single-thread C++ port of the serial loop
(scripts/lidar_port.cpp, built with g++ -O3 when scripts/lidar_port is missing) on the same host: the
port, not the reference. One JSON line. Kernel (device) time comes from a kernel trace of this script
in a run of its own (few REPS).
Usage: lidar_timing.py [Q [S [REPS]]]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "okvis2-x_amd"))
import okvisgpu as og  # noqa: E402

nq, ns, reps = (int(x) for x in (sys.argv[1:] + ["65536", "41", "30"][len(sys.argv) - 1:]))
C = og.C
rate = 5_000_000


def make(n_scans, rng):
    base = 1_000_000_000 + rng.integers(0, rate, n_scans)
    ts = (base[:, None] + np.arange(ns, dtype=np.int64)[None, :] * rate).astype(np.int64)
    t0 = ts[:, 0] + 777
    qt = t0[:, None] + 1 + ((ts[0, -1] - ts[0, 0] - 778) * np.arange(nq, dtype=np.float64) / nq).astype(np.int64)[None, :]
    ga = np.concatenate([rng.uniform(-1, 1, (n_scans, 1, 3)) + 0.2 * rng.normal(size=(n_scans, ns, 3)),
                         np.array([0.0, 0.0, 9.81]) + 0.5 * rng.normal(size=(n_scans, ns, 3))], axis=2)

    def poses(reach):
        q = rng.normal(size=(n_scans, 4))
        return np.hstack([rng.uniform(-reach, reach, (n_scans, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)])

    sb = np.hstack([rng.uniform(-2, 2, (n_scans, 3)), rng.uniform(-0.02, 0.02, (n_scans, 3)),
                    rng.uniform(-0.1, 0.1, (n_scans, 3))])
    return dict(pose0=poses(300), speed_bias0=sb, t_start=t0, sample_begin=np.arange(n_scans + 1, dtype=np.int32) * ns,
                sample_t=ts.reshape(-1), sample_ga=ga.reshape(-1, 6), query_begin=np.arange(n_scans + 1, dtype=np.int32) * nq,
                query_t=qt.reshape(-1), ray=rng.uniform(-50, 50, (n_scans * nq, 3)), pose_live=poses(300), T_SL=poses(0.5))


def timed(call):
    wall = []
    for _ in range(5 + reps):
        a = time.perf_counter()
        rc = call()
        wall.append((time.perf_counter() - a) * 1e3)
        assert rc == 0
    w = np.sort(wall[5:])
    return {"wall_ms_median": float(np.median(w)), "wall_ms_q1": float(w[len(w) // 4]),
            "wall_ms_q3": float(w[(3 * len(w)) // 4])}


def deskew(ctx, a, outputs, rays):
    n = len(a["t_start"])
    args = dict(a)
    if not rays:
        for k in ("ray", "pose_live", "T_SL"):
            args.pop(k)
    b, keep = og.lidar_deskew_batch(**args)
    spec = {"valid": ((n * nq,), np.uint8), "point": ((n * nq, 3), np.float32), "pose": ((n * nq, 7), np.float64),
            "speed": ((n * nq, 3), np.float64), "omega_S": ((n * nq, 3), np.float64)}
    out = {k: np.zeros(*spec[k]) for k in outputs}
    r = og.LidarDeskewResult()
    og._set_arrays(r, out)
    res = timed(lambda: og.lib().okvisgpu_lidar_deskew(ctx.h, C.byref(b), C.byref(r)))
    assert out["valid"].all()
    res["bytes_up"] = int(sum(v.nbytes for v in keep.values()) + 4 * n * nq)  # + the scan of every query
    res["bytes_down"] = int(sum(v.nbytes for v in out.values()))
    return res, out


rng = np.random.default_rng(65536)
ctx = og.Context(0)
result = {"queries_per_scan": nq, "samples_per_scan": ns, "reps": reps}
one = make(1, rng)
result["deskew_1_scan"], out = deskew(ctx, one, ("valid", "point"), True)
result["states_1_scan"], _ = deskew(ctx, one, ("valid", "pose", "speed", "omega_S"), False)
result["deskew_64_scans"], _ = deskew(ctx, make(64, rng), ("valid", "point"), True)

cloud = out["point"]
vb, vkeep = og.voxel_downsample_batch([0, len(cloud)], cloud, [0.05])
vout = {"keep": np.zeros(len(cloud), np.uint8), "n_kept": np.zeros(1, np.int32)}
vr = og.VoxelDownsampleResult()
og._set_arrays(vr, vout)
result["voxel_1_cloud"] = timed(lambda: og.lib().okvisgpu_voxel_downsample(ctx.h, C.byref(vb), C.byref(vr)))
result["voxel_1_cloud"].update(bytes_up=int(cloud.nbytes + 4 * len(cloud) + 4), bytes_down=int(len(cloud) + 4 + 4),
                               kept=int(vout["n_kept"][0]))
ctx.close()

port = os.path.join(HERE, "lidar_port")
if not os.path.exists(port):
    subprocess.run(["g++", "-O3", "-std=c++17", os.path.join(HERE, "lidar_port.cpp"), "-o", port], check=True)
result["cpu_port"] = json.loads(subprocess.run([port, str(nq), str(ns), "11"], capture_output=True, text=True,
                                               check=True).stdout)
print(json.dumps(result))
