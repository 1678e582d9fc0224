"""Wall time of okvisgpu_place_match and okvisgpu_place_refine at a loop-closure frame's shape: CAND candidates
(default 12) against one new multiframe of 2 cameras x K keypoints (default 1,000). Match: every candidate
has 300 landmarks of 1-3 descriptors; 60 % of them re-appear in one of the images (descriptor noise of up to
35 bits), the others are unrelated. Refine: every candidate has 150 inlier observations over the two cameras
with half a pixel of noise, started a few centimetres off, at most 10 iterations. Timed: one candidate (the
serial adapter's call) and all candidates in one call. Warm-up calls, then the median (and the quartiles) of
REPS calls, each timed by a host clock around the call, which returns after a stream synchronise with the
results in the caller's arrays. One JSON line. Kernel (device) time comes from a kernel trace of this script in
a run of its own (few REPS).
Usage: place_timing.py [K [CAND [REPS]]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "okvis2-x_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import okvisgpu as og  # noqa: E402
import _place as pl  # noqa: E402  (the scene builders)

K, cand, reps = (int(x) for x in (sys.argv[1:] + ["1000", "12", "50"][len(sys.argv) - 1:]))
rng = np.random.default_rng(3000)
images = [rng.integers(0, 256, size=(K, 48), dtype=np.uint8) for _ in range(2)]


def landmarks(n):
    out = []
    for l in range(n):
        src = images[l % 2][rng.integers(K)] if rng.random() < 0.6 else rng.integers(0, 256, size=48, dtype=np.uint8)
        out.append(np.array([pl.flip_bits(rng, src, int(rng.integers(0, 36))) for _ in range(1 + l % 3)], np.uint8))
    return out


match = pl.match_scene(2, images, [((0, 1), landmarks(300)) for _ in range(cand)])
refine = pl.refine_scene([pl.refine_job(3000 + j, 150, noise=0.5) for j in range(cand)], max_num_iterations=10)


def timed(call):
    wall = []
    for _ in range(5 + reps):
        a = time.perf_counter()
        rc = call()
        wall.append((time.perf_counter() - a) * 1e3)
        assert rc == 0
    ws = np.sort(wall[5:])
    return {"wall_ms_median": float(np.median(ws)), "wall_ms_q1": float(ws[len(ws) // 4]),
            "wall_ms_q3": float(ws[(3 * len(ws)) // 4])}


def pointers(r, res):
    for k, a in res.items():
        setattr(r, k, a.ctypes.data_as(og.C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype))))
    return r


ctx = og.Context(0)
out = {"keypoints_per_image": K, "candidates": cand, "reps": reps}
for name, sel in (("one_candidate", [0]), ("all_candidates", list(range(cand)))):
    b, keep = og.place_match_batch(**pl.match_sub_scene(match, sel))
    res = ctx.place_match(b)  # (allocates the outputs once; the timed calls re-use them)
    r = pointers(og.PlaceMatchResult(), res)
    out["match_" + name] = {"jobs": len(sel), **timed(lambda: og.lib().okvisgpu_place_match(ctx.h, og.C.byref(b), og.C.byref(r))),
                            "matches": int(res["job_matches"].sum()),
                            "digest": int(np.int64(res["match_keypoint"]).sum() * 31 + np.int64(res["match_distance"]).sum())}
    t = pl.refine_sub_scene(refine, sel)
    start = t["pose"].copy()
    pose = start.copy()
    b2, keep2 = og.place_refine_batch(cameras=pl.cameras_of(t), extrinsics=t["extrinsics"], pose=pose, loss=t["loss"],
                                      max_num_iterations=t["max_num_iterations"],
                                      **{k: t[k] for k in ("obs_begin", "obs_camera", "obs_keypoint", "obs_sqrt_info",
                                                           "obs_point")})
    res2 = ctx.place_refine(b2)
    r2 = pointers(og.PlaceRefineResult(), res2)

    def call():
        pose[...] = start  # (every timed call solves from the RANSAC model again)
        return og.lib().okvisgpu_place_refine(ctx.h, og.C.byref(b2), og.C.byref(r2))

    out["refine_" + name] = {"jobs": len(sel), **timed(call), "iterations": [int(i) for i in res2["num_iterations"]],
                             "worst_pose_error": float(np.abs(pose - t["truth"]).max())}
ctx.close()
print(json.dumps(out))
