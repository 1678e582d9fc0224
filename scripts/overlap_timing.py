"""Wall time of okvisgpu_frame_overlap: warm-up calls, then the median (and the quartiles) of REPS calls,
each timed by a host clock around the C call, which returns after a stream synchronise with the results
in the caller's arrays (allocated once). Two shapes: the current frame against 40 keyframes, 2 cameras,
752 x 480 with 700 keypoints per image, and the same at 1440 x 1080 with 1,000. Per shape: the 40 kind-0
jobs of mostOverlappedStateId as one group, the same loop cut to 1, 2, 4, 8 and 16 keyframes (where the
call breaks even with the port), the 1 + 40 jobs of doWeNeedANewKeyframe (kinds 2 and 1), the kind-3 job
of trackingQuality, and all 82 jobs of a frame in one call; with each the bytes staged up and down.
Beside it the single-thread C++ port of the reference's loops (scripts/overlap_port.cpp, built with
g++ -O3 when scripts/overlap_port is missing) on the same host and the same inputs: the port, not the
reference; its results must equal the device's bit for bit. One JSON line. Kernel (device) time comes
from a kernel trace of this script in a run of its own (few REPS).
Usage: overlap_timing.py [REPS [KEYFRAMES]]"""
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

reps, n_key = (int(x) for x in (sys.argv[1:] + ["30", "40"][len(sys.argv) - 1:]))
C = og.C
FACTOR = 0.09


def make(rng, rows, cols, n_kp):
    """The current frame (0) and n_key keyframes, two images each. A keyframe shares, per image, a run of the
    current frame's landmarks (fewer the older it is), has ids of its own on a third of the others; a third of
    the current frame's keypoints carry no landmark."""
    n_frames, n_images = 1 + n_key, 2
    kp = np.stack([rng.uniform(0, cols, (n_frames, n_images, n_kp)), rng.uniform(0, rows, (n_frames, n_images, n_kp))],
                  axis=-1).astype(np.float32)
    lm = np.zeros((n_frames, n_images, n_kp), np.uint64)
    cur = 1 + np.arange(n_images * n_kp, dtype=np.uint64).reshape(n_images, n_kp)
    lm[0] = np.where(rng.random((n_images, n_kp)) < 2 / 3, cur, 0)
    for f in range(1, n_frames):
        shared = int(n_kp * (0.6 - 0.5 * f / n_frames))
        own = np.uint64(1_000_000 * f) + np.arange(n_images * n_kp, dtype=np.uint64).reshape(n_images, n_kp)
        lm[f] = np.where(rng.random((n_images, n_kp)) < 1 / 3, own, 0)
        for i in range(n_images):
            lm[f, i, :shared] = lm[0, i, rng.permutation(n_kp)[:shared]]
    flag = (lm != 0) & (rng.random(lm.shape) < 0.8)
    return dict(image_begin=np.arange(n_frames + 1) * n_images, rows=np.full(n_frames * n_images, rows),
                cols=np.full(n_frames * n_images, cols), kp_begin=np.arange(n_frames * n_images + 1) * n_kp,
                keypoint=kp.reshape(-1, 2), landmark=lm.reshape(-1), flag=flag.reshape(-1).astype(np.uint8))


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


def run(ctx, frames, jobs, groups):
    b, keep = og.frame_overlap_batch(job_kind=[j[0] for j in jobs], job_frame_a=[j[1] for j in jobs],
                                     job_frame_b=[j[2] for j in jobs], job_radius_factor=[FACTOR] * len(jobs),
                                     group_begin=groups, **frames)
    nj, ng = len(jobs), len(groups) - 1
    out = {"overlap": np.zeros(nj), "count": np.zeros((nj, 4), np.int32), "n_matched": np.zeros((nj, 2), np.int32),
           "n_keypoints": np.zeros(nj, np.int32), "group_best": np.zeros(ng, np.int32), "group_max": np.zeros(ng)}
    r = og.FrameOverlapResult()
    og._set_arrays(r, out)
    res = timed(lambda: og.lib().okvisgpu_frame_overlap(ctx.h, C.byref(b), C.byref(r)))
    res["jobs"] = nj
    res["bytes_up"] = int(sum(v.nbytes for v in keep.values()))
    res["bytes_down"] = int(sum(v.nbytes for k, v in out.items() if k != "n_keypoints"))
    return res, out


def shape(ctx, rng, rows, cols, n_kp):
    frames = make(rng, rows, cols, n_kp)
    pairs = [(0, k, 0) for k in range(1, n_key + 1)]  # overlapFraction(keyframe, current)
    keyframe = [(2, 0, 0)] + [(1, 0, k) for k in range(1, n_key + 1)]
    quality = [(3, 0, 0)]
    res = {"rows": rows, "cols": cols, "keypoints_per_image": n_kp, "keyframes": n_key, "factor": FACTOR}
    res["most_overlapped"], po = run(ctx, frames, pairs, [0, n_key])
    for n in (1, 2, 4, 8, 16):
        if n < n_key:
            res[f"most_overlapped_{n}"], _ = run(ctx, frames, pairs[:n], [0, n])
    res["new_keyframe"], ko = run(ctx, frames, keyframe, [0, 1, 1 + n_key])
    res["tracking_quality"], qo = run(ctx, frames, quality, [0, 1])
    res["whole_frame"], _ = run(ctx, frames, pairs + keyframe + quality, [0, n_key, n_key + 1, 2 * n_key + 1, 2 * n_key + 2])

    port = os.path.join(HERE, "overlap_port")
    if not os.path.exists(port):
        subprocess.run(["g++", "-O3", "-std=c++17", os.path.join(HERE, "overlap_port.cpp"), "-o", port], check=True)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(np.array([1 + n_key, 2, rows, cols, n_kp], np.int32).tobytes())
        kp, lm, fl = frames["keypoint"].reshape(-1, n_kp, 2), frames["landmark"].reshape(-1, n_kp), frames["flag"].reshape(-1, n_kp)
        for i in range(len(kp)):
            f.write(kp[i].tobytes() + lm[i].tobytes() + fl[i].tobytes())
        f.flush()
        cpu = json.loads(subprocess.run([port, f.name, repr(FACTOR), "7"], capture_output=True, text=True, check=True).stdout)
    same = lambda a, b: np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))
    res["port_agrees"] = bool(same(cpu.pop("pairs"), po["overlap"]) and same(cpu.pop("others"), ko["overlap"][1:]) and
                              same([cpu["current"]], ko["overlap"][:1]) and same([cpu["quality"]], qo["overlap"]) and
                              cpu["best"] - 1 == int(po["group_best"][0]))
    res["overlap_range"] = [float(po["overlap"].min()), float(po["overlap"].max())]
    res["cpu_port"] = cpu
    per_pair = cpu["most_overlapped_ms_median"] / n_key
    res["port_ms_per_pair"] = per_pair
    return res


rng = np.random.default_rng(752480)
ctx = og.Context(0)
result = {"reps": reps, "shapes": [shape(ctx, rng, 480, 752, 700), shape(ctx, rng, 1080, 1440, 1000)]}
ctx.close()
print(json.dumps(result))
