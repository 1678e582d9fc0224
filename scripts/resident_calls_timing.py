"""Outputs and wall time of the entry points that read the resident batch (csrc/resident_calls.cpp, and
okvisgpu_plan_window): a batch of WINDOWS (default 64) synthetic 10-keyframe windows (500 landmarks, 4,000
reprojections, 9 IMU factors each) is uploaded once; okvisgpu_update_landmarks and okvisgpu_covisibilities run
over the whole batch, the calls that take a window on window 0. Per entry point: the SHA-256 of every output
array of its first call, then warm-up calls and the median (and the quartiles) of REPS calls, each timed by a
host clock around the call, which returns after a stream synchronise with the results in the caller's arrays.
The batch-wide calls are timed through the C ABI with their output arrays allocated once. The calls that write
parameters (update_landmarks re-places landmarks, eval_imu re-integrates) go on from what the call before left:
the sequence is fixed, so two libraries that compute the same give the same digests. One JSON line.
OKVISGPU_LIB selects the library (an A/B against another build).
Usage: resident_calls_timing.py [WINDOWS [REPS]]"""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "okvis2-x_amd"))
import okvisgpu as og  # noqa: E402

n_win, reps = (int(x) for x in (sys.argv[1:] + ["64", "50"][len(sys.argv) - 1:]))
windows = [og.SynthWindow(10, 500, 4000, seed=20251015 + i) for i in range(n_win)]
probs = [w.problem for w in windows]
p0 = probs[0]
_up, _ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def timed(call):
    wall = []
    for _ in range(5 + reps):
        a = time.perf_counter()
        call()
        wall.append((time.perf_counter() - a) * 1e3)
    ws = np.sort(wall[5:])
    return {"wall_ms_median": float(np.median(ws)), "wall_ms_q1": float(ws[len(ws) // 4]),
            "wall_ms_q3": float(ws[(3 * len(ws)) // 4])}


def params():  # the caller's arrays a call may write, over the whole batch
    return {k: sha(np.concatenate([getattr(w, k)().ravel() for w in windows]))
            for k in ("poses", "speed_biases", "landmarks", "imu_state")}


ctx = og.Context(0)
ctx.set_problems(probs)
lib = og.lib()
out = {"windows": n_win, "reps": reps, "lib": os.path.basename(og.LIB_PATH)}

# ---- the batch-wide calls, through the C ABI with their arrays allocated once
ups = (og.LandmarkUpdate * n_win)()
lm = [{"quality": np.zeros(p.n_landmarks), "initialised": np.zeros(p.n_landmarks, np.uint8),
       "reset": np.zeros(p.n_landmarks, np.uint8), "obs_error": np.zeros(p.n_observations)} for p in probs]
for u, d in zip(ups, lm):
    u.quality, u.obs_error = og.dptr(d["quality"]), og.dptr(d["obs_error"])
    u.initialised, u.reset = d["initialised"].ctypes.data_as(_up), d["reset"].ctypes.data_as(_up)


def update_landmarks():
    assert lib.okvisgpu_update_landmarks(ctx.h, ups) == 0


vs = (og.Covisibility * n_win)()
cv = [{"counts": np.zeros((p.n_poses, p.n_poses), np.int32), "n_observed": np.zeros(p.n_poses, np.int32),
       "visible": np.zeros(p.n_poses, np.uint8)} for p in probs]
masks = [(np.arange(p.n_landmarks) % 3 == w % 3).astype(np.uint8) for w, p in enumerate(probs)]
for v, d in zip(vs, cv):
    v.counts, v.n_observed = d["counts"].ctypes.data_as(_ip), d["n_observed"].ctypes.data_as(_ip)
    v.visible = d["visible"].ctypes.data_as(_up)


def covisibilities():
    assert lib.okvisgpu_covisibilities(ctx.h, vs) == 0


def batch_digest(arrays, structs, scalars):
    d = {k: sha(np.concatenate([a[k].ravel() for a in arrays])) for k in arrays[0]}
    d["scalars"] = sha(np.array([[getattr(s, k) for k in scalars] for s in structs], np.int64))
    return d


update_landmarks()
out["update_landmarks"] = {"digest": {**batch_digest(lm, ups, ("n_initialised", "n_reset", "in_front")), **params()},
                           "n_reset": int(sum(u.n_reset for u in ups)), **timed(update_landmarks)}
covisibilities()
out["covisibilities"] = {"digest": batch_digest(cv, vs, ("n_pairs", "n_visible", "any", "path")), **timed(covisibilities)}
for v, m in zip(vs, masks):
    v.landmark_excluded = m.ctypes.data_as(_up)
covisibilities()
out["covisibilities_masked"] = {"digest": batch_digest(cv, vs, ("n_pairs", "n_visible", "any", "path")),
                                **timed(covisibilities)}


# ---- the calls on window 0, through the Python wrappers (which allocate their outputs per call)
def entry(name, call, extra=None):
    try:
        res = call()
    except og.OkvisGpuError as e:  # (a refusal is an output too: the status and the text)
        out[name] = {"digest": {"error": str(e)}}
        return
    res = res if isinstance(res, tuple) else (res,)
    d = {str(i): sha(np.asarray(a)) for i, a in enumerate(res)}
    if extra:
        d.update(extra())
    out[name] = {"digest": d, **timed(call)}


entry("evaluate", lambda: ctx.evaluate(0))
entry("linearize_reduce", lambda: ctx.linearize_reduce(0))
entry("linearize_reduce_mu_unscaled", lambda: ctx.linearize_reduce(0, jacobi_scaling=False, mu=1e-4))
entry("gauss_newton_step", lambda: ctx.gauss_newton_step(0))
entry("eval_reprojection", lambda: ctx.eval_reprojection(p0.n_observations, 0))
entry("eval_imu", lambda: ctx.eval_imu(p0.n_imu, 0), params)
entry("eval_imu_redo_always", lambda: ctx.eval_imu(p0.n_imu, 0, redo_always=True), params)
entry("eval_relpose", lambda: ctx.eval_relpose(p0.n_relpose, 0))
entry("eval_host", lambda: ctx.eval_host(p0.n_host, 0))

# ---- no device work to time: statistics, the kernels' work models, the host-side plan of window 0
out["get_stats"] = {"digest": {"stats": sha(np.array(list(ctx.stats().values()), np.int64))}}
ctx.solve(og.default_options(max_num_iterations=3))  # (time_kernel re-runs the kernels of a finished solve)
out["time_kernel"] = {"digest": {name: "%r %s" % ctx.time_kernel(name, reps=1)[1:] for name in og.kernel_names()}}
out["plan_window"] = {"digest": {f"nd{nd}.{k}": sha(np.asarray(v)) for nd in (0, 1)
                                 for k, v in og.plan_window(p0, nd).items()}}
ctx.close()
print(json.dumps(out))
