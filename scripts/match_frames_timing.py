"""Wall time of okvisgpu_match_frames at the reference's own shape: OLDER older keyframes x 2 cameras of K x K
keypoints in mode 0 (Frontend::matchMotionStereo; default OLDER = 8, K = 1,000) and one K x K stereo pair in
mode 1 (Frontend::matchStereo). About 40 % of every side 0 has a true partner on side 1 (the same point,
descriptor noise of up to 35 bits); the other keypoints of both sides see unrelated points with random
descriptors. Timed: one older frame (2 jobs: the adapter's call), all older frames in one call, the stereo
pair, and everything in one call. Warm-up calls, then the median (and the quartiles) of REPS calls, each
timed by a host clock around the call, which returns after a stream synchronise with the results in the
caller's arrays. One JSON line. Kernel (device) time comes from a kernel trace of this script in a run of its
own (few REPS).
Usage: match_frames_timing.py [K [OLDER [REPS]]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "okvis2-x_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import okvisgpu as og  # noqa: E402
import _match_frames as mf  # noqa: E402  (the scene builders)

K, older, reps = (int(x) for x in (sys.argv[1:] + ["1000", "8", "50"][len(sys.argv) - 1:]))
rng = np.random.default_rng(2000)
cams = [mf.pinhole(), mf.pinhole(1, (-0.28, 0.07, 2e-4, 1.8e-5))]
ext = [mf.at(0.0), mf.at(0.11, 0.01)]
current = mf.at(0.0, 0.0, 0.0)


def points(n):
    return np.column_stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(3.0, 10.0, n)])


def pair(mode, c0, c1, pose0, pose1):
    """One K x K job: 40 % of side 0 re-appears on side 1, in random order."""
    shared = int(0.4 * K)
    p0, d0 = points(K), rng.integers(0, 256, size=(K, 48), dtype=np.uint8)
    p1 = np.vstack([p0[:shared], points(K - shared)])
    d1 = np.vstack([[mf.flip_bits(rng, d, int(rng.integers(0, 36))) for d in d0[:shared]],
                    rng.integers(0, 256, size=(K - shared, 48), dtype=np.uint8)])
    order = rng.permutation(K)
    noise = dict(rng=rng, pixel_noise=0.5, ray_noise=0.3 / 400)
    return mf.job(mode, c0, c1, pose0, pose1, ext[c0], ext[c1],
                  mf.side(cams[c0], pose0, ext[c0], p0, d0, size=rng.uniform(6.0, 14.0, K), **noise),
                  mf.side(cams[c1], pose1, ext[c1], p1[order], d1[order], size=rng.uniform(6.0, 14.0, K), **noise))


jobs = [pair(0, c, c, mf.at(-0.12 * (f + 1), 0.01 * f, 0.02 * f), current) for f in range(older) for c in (0, 1)]
jobs.append(pair(1, 0, 1, current, current))
s = mf.scene(cams, jobs)


def camera(c):
    q = og.Camera()
    q.distortion, q.width, q.height = c["distortion"], c["width"], c["height"]
    q.fu, q.fv, q.cu, q.cv = c["fu"], c["fv"], c["cu"], c["cv"]
    for i in range(8):
        q.dist[i] = c["dist"][i]
    return q


ctx = og.Context(0)
out = {"keypoints_per_side": K, "older_frames": older, "reps": reps}
for name, sel in (("one_older_frame", [0, 1]), ("all_older_frames", list(range(2 * older))), ("stereo_pair", [2 * older]),
                  ("everything", list(range(2 * older + 1)))):
    t = mf.sub_scene(s, sel)
    b, keep = og.frame_match_batch(cameras=[camera(c) for c in cams], **{k: v for k, v in t.items() if k != "cameras"})
    res = ctx.match_frames(b)  # (allocates the outputs once; the timed calls re-use them)
    r = og.FrameMatchResult()
    for k, a in res.items():
        setattr(r, k, a.ctypes.data_as(og.C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype))))
    wall = []
    for _ in range(5 + reps):
        a = time.perf_counter()
        rc = og.lib().okvisgpu_match_frames(ctx.h, og.C.byref(b), og.C.byref(r))
        wall.append((time.perf_counter() - a) * 1e3)
        assert rc == 0
    ws = np.sort(wall[5:])
    out[name] = {"jobs": len(sel), "wall_ms_median": float(np.median(ws)), "wall_ms_q1": float(ws[len(ws) // 4]),
                 "wall_ms_q3": float(ws[(3 * len(ws)) // 4]), "matches": int((res["match"] >= 0).sum()),
                 "digest": int(np.int64(res["match"]).sum() * 31 + np.int64(res["distance"]).sum())}
ctx.close()
print(json.dumps(out))
