"""Wall time of okvisgpu_match_to_map for one realistic job pair: 2 cameras x K keypoints against a map
of L landmarks x 8 observations (default K = 1,000, L = 2,000: an 11-keyframe synthetic window whose
last frame is the current one), for the pass-0 pair, the pass-1 pair and all four jobs in one call.
Warm-up calls, then the median (and the quartiles) of REPS calls, each timed by a host clock around
the call, which returns after a stream synchronise with the results in the caller's arrays. One JSON
line. Kernel (device) time comes from a kernel trace of this script in a run of its own (few REPS).
Usage: match_to_map_timing.py [K [L [REPS]]]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "okvis2-x_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import okvisgpu as og  # noqa: E402
import _match as mt  # noqa: E402  (the scene builder)

K, L, reps = (int(x) for x in (sys.argv[1:] + ["1000", "2000", "50"][len(sys.argv) - 1:]))
w = og.SynthWindow(11, L, 8 * L, seed=2000)
p = w.problem
cams = [{"distortion": q.distortion, "width": q.width, "height": q.height, "fu": q.fu, "fv": q.fv, "cu": q.cu,
         "cv": q.cv, "dist": list(q.dist)} for q in (p.cameras[c] for c in range(p.n_cameras))]
gt_poses, gt_landmarks, _ = w.ground_truth()
arr = lambda ptr: np.ctypeslib.as_array(ptr, shape=(p.n_observations,)).copy()
s = mt.build_scene(gt_poses, gt_landmarks, w.true_extrinsics(), cams, arr(p.obs_pose), arr(p.obs_landmark),
                   arr(p.obs_camera), seed=2000, distractors=1.0)
# K keypoints per job: the job's own, repeated if it has fewer
jobs = []
for j in range(len(s["job_camera"])):
    a, b = int(s["kp_begin"][j]), int(s["kp_begin"][j + 1])
    jobs.append((int(s["job_camera"][j]), int(s["job_pass"][j]), a + np.arange(K) % (b - a), s["job_pose_prepare"][j],
                 s["job_pose_match"][j]))
s = mt.with_jobs(s, jobs)


def camera(c):
    q = og.Camera()
    q.distortion, q.width, q.height = c["distortion"], c["width"], c["height"]
    q.fu, q.fv, q.cu, q.cv = c["fu"], c["fv"], c["cu"], c["cv"]
    for i in range(8):
        q.dist[i] = c["dist"][i]
    return q


ctx = og.Context(0)
out = {"keypoints_per_job": K, "landmarks": L, "observations": int(s["obs_begin"][-1]), "reps": reps}
for name, sel in (("pass0_pair", [0, 1]), ("pass1_pair", [2, 3]), ("both_pairs", [0, 1, 2, 3])):
    t = mt.sub_scene(s, sel)
    b, keep = og.match_batch(cameras=[camera(c) for c in cams], **{k: v for k, v in t.items() if k != "cameras"})
    res = ctx.match_to_map(b)  # (allocates the outputs once; the timed calls re-use them)
    r = og.MatchResult()
    for k, a in res.items():
        setattr(r, k, a.ctypes.data_as(og.C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype))))
    wall = []
    for _ in range(5 + reps):
        a = time.perf_counter()
        rc = og.lib().okvisgpu_match_to_map(ctx.h, og.C.byref(b), og.C.byref(r))
        wall.append((time.perf_counter() - a) * 1e3)
        assert rc == 0
    ws = np.sort(wall[5:])
    out[name] = {"wall_ms_median": float(np.median(ws)), "wall_ms_q1": float(ws[len(ws) // 4]),
                 "wall_ms_q3": float(ws[(3 * len(ws)) // 4]), "matches": int((res["match_landmark"] >= 0).sum()),
                 "candidates": int((res["cand_n"] > 0).sum())}
ctx.close()
print(json.dumps(out))
