"""The two device-side parts of Frontend::verifyRecognisedPlace restated in numpy (test infrastructure for
okvisgpu_place_match and okvisgpu_place_refine; reference: okvis_frontend/src/Frontend.cpp:316-345 and
:434-598).

  match_literal(scene)   the serial loops of :317-345: per (landmark, camera) a running distMin over the
                         landmark's descriptors and, within a descriptor, the image's keypoints.
  match_ordered(scene)   the parallel formulation: the first minimum in (descriptor, keypoint) order, a match
                         if it is below the truncated threshold; otherwise, where the truncated threshold is
                         itself below the threshold, the reference's untouched (kMin, distMin) = (0, start).
  refine_literal(scene)  ::ceres::Solve with TRUST_REGION / LEVENBERG_MARQUARDT on the one pose block, built on
                         the oracle's primitives (oracle_eval_reprojection on a one-pose problem with constant
                         landmarks, oracle_loss_correct, oracle_pose_plus); the damped problem is solved by
                         numpy.linalg.lstsq on the augmented Jacobian, as DENSE_QR does. Then :565-598.
  refine_normal(scene)   the same with the 6x6 normal equations and a Cholesky factorisation.

A match scene is a dict with the arguments of okvisgpu.place_match_batch. A refine scene is a dict with the
arguments of okvisgpu.place_refine_batch, cameras as dicts (distortion, width, height, fu, fv, cu, cv,
dist[8]). Both refine functions also return `margin`, the smallest relative distance of any decision of the
loop from its threshold (the three tolerance tests, rel > 1e-3, model_cost_change > 0, |r| > 3)."""
import ctypes as C

import numpy as np

import okvisgpu as og
import _oracle
from _match import box_plus, flip_bits, hamming, pinhole, rotation  # noqa: F401
from _problem import OwnedProblem

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
MATCH_KEYS = ("match_keypoint", "match_distance", "job_matches")
REFINE_INT_KEYS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "termination_type", "n_outliers")
REFINE_REAL_KEYS = ("pose", "H", "initial_cost", "final_cost")
IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
DBL_MAX = np.finfo(np.float64).max


# ------------------------------------------------------------------------------------------ match
def _match_outputs(s):
    nj, nc = len(s["lm_begin"]) - 1, int(s["n_cameras"])
    nl = int(s["lm_begin"][-1])
    return {"match_keypoint": np.full((nl, nc), -1, np.int32), "match_distance": np.full((nl, nc), -1, np.int32),
            "job_matches": np.zeros(nj, np.int32)}


def _pairs(s):
    """(job, landmark, camera, the landmark's descriptors, the image's descriptors) of every pair with K > 0."""
    ji = np.asarray(s["job_image"], np.int32).reshape(-1, int(s["n_cameras"]))
    for j in range(len(s["lm_begin"]) - 1):
        for l in range(int(s["lm_begin"][j]), int(s["lm_begin"][j + 1])):
            olds = s["old_descriptor"][int(s["desc_begin"][l]):int(s["desc_begin"][l + 1])]
            for im in range(int(s["n_cameras"])):
                img = int(ji[j, im])
                if img < 0:
                    continue
                new = s["descriptor"][int(s["kp_begin"][img]):int(s["kp_begin"][img + 1])]
                if len(new) == 0:  # :320
                    continue
                yield j, l, im, olds, new


def match_literal(s):
    thr = float(s["matching_threshold"])
    out = _match_outputs(s)
    for j, l, im, olds, new in _pairs(s):
        if len(olds) == 0:  # (the reference has no landmark without a descriptor: defined as no match)
            continue
        table = hamming(olds, new)
        dist_min, k_min = int(thr), 0  # uint32_t distMin = briskMatchingThreshold_
        for d in range(len(olds)):
            for k in range(len(new)):
                if table[d, k] < dist_min:
                    dist_min, k_min = int(table[d, k]), k
        if float(dist_min) < thr:
            out["job_matches"][j] += 1
            out["match_keypoint"][l, im], out["match_distance"][l, im] = k_min, dist_min
    return out


def match_ordered(s):
    start = int(float(s["matching_threshold"]))
    out = _match_outputs(s)
    for j, l, im, olds, new in _pairs(s):
        if len(olds) == 0:
            continue
        table = hamming(olds, new)
        first = int(np.argmin(table))  # row-major: (descriptor, keypoint) order, the first minimum
        if table.flat[first] < start:
            out["job_matches"][j] += 1
            out["match_keypoint"][l, im], out["match_distance"][l, im] = first % len(new), table.flat[first]
        elif start < float(s["matching_threshold"]):  # :338 on the untouched (kMin, distMin) = (0, start)
            out["job_matches"][j] += 1
            out["match_keypoint"][l, im], out["match_distance"][l, im] = 0, start
    return out


def match_scene(n_cameras, images, jobs, matching_threshold=60.0):
    """images: list of [K, 48] descriptor arrays; jobs: list of (image per camera, list of landmarks), a
    landmark being a [D, 48] array of old descriptors."""
    kp_begin = np.concatenate([[0], np.cumsum([len(i) for i in images])]).astype(np.int32)
    lms = [lm for _, ls in jobs for lm in ls]
    return {"n_cameras": n_cameras, "matching_threshold": matching_threshold, "kp_begin": kp_begin,
            "descriptor": np.concatenate([np.asarray(i, np.uint8).reshape(-1, 48) for i in images] +
                                         [np.zeros((0, 48), np.uint8)]),
            "job_image": np.asarray([im for im, _ in jobs], np.int32).reshape(len(jobs), n_cameras),
            "lm_begin": np.concatenate([[0], np.cumsum([len(ls) for _, ls in jobs])]).astype(np.int32),
            "desc_begin": np.concatenate([[0], np.cumsum([len(lm) for lm in lms])]).astype(np.int32),
            "old_descriptor": np.concatenate([np.asarray(lm, np.uint8).reshape(-1, 48) for lm in lms] +
                                             [np.zeros((0, 48), np.uint8)])}


def match_sub_scene(s, jobs):
    """The scene with only the listed jobs (the images stay)."""
    lms = [l for j in jobs for l in range(int(s["lm_begin"][j]), int(s["lm_begin"][j + 1]))]
    olds = [s["old_descriptor"][int(s["desc_begin"][l]):int(s["desc_begin"][l + 1])] for l in lms]
    t = dict(s)
    t["job_image"] = np.asarray(s["job_image"]).reshape(-1, int(s["n_cameras"]))[list(jobs)].reshape(len(jobs), int(s["n_cameras"]))
    t["lm_begin"] = np.concatenate([[0], np.cumsum([int(s["lm_begin"][j + 1] - s["lm_begin"][j]) for j in jobs])]).astype(np.int32)
    t["desc_begin"] = np.concatenate([[0], np.cumsum([len(o) for o in olds])]).astype(np.int32)
    t["old_descriptor"] = np.concatenate(olds + [np.zeros((0, 48), np.uint8)])
    return t


def match_job_rows(s, out, j):
    a, b = int(s["lm_begin"][j]), int(s["lm_begin"][j + 1])
    return {"match_keypoint": out["match_keypoint"][a:b], "match_distance": out["match_distance"][a:b],
            "job_matches": out["job_matches"][j:j + 1]}


# ------------------------------------------------------------------------------------------ refine
class Margin:
    """The smallest relative distance of a decided comparison from its threshold."""

    def __init__(self):
        self.worst = np.inf

    def note(self, value, threshold, scale=None):
        if np.isnan(value) or np.isnan(threshold):
            return
        scale = abs(threshold) if scale is None else scale
        self.worst = min(self.worst, abs(value - threshold) / scale if scale > 0 else (np.inf if value != threshold else 0.0))

    def le(self, value, threshold):
        self.note(value, threshold)
        return value <= threshold

    def gt(self, value, threshold, scale=None):
        self.note(value, threshold, scale)
        return value > threshold


def _camera(c):
    q = og.Camera()
    q.distortion, q.width, q.height = c["distortion"], c["width"], c["height"]
    q.fu, q.fv, q.cu, q.cv = c["fu"], c["fv"], c["cu"], c["cv"]
    for i in range(8):
        q.dist[i] = c["dist"][i]
    return q


def cameras_of(s):
    return [_camera(c) for c in s["cameras"]]


def _loss(s):
    return og.Loss(*og.loss_array([s["loss"]])[0].tolist())


def pose_plus(x, delta):
    out = np.zeros(7)
    _oracle.lib().oracle_pose_plus(og.dptr(np.ascontiguousarray(x, np.float64)),
                                   og.dptr(np.ascontiguousarray(delta, np.float64)), og.dptr(out))
    return out


class _Job:
    """Job j as a one-pose problem with constant landmarks: ReprojectionError::EvaluateWithMinimalJacobians
    of every observation through the oracle, the loss through the oracle's Corrector."""

    def __init__(self, s, j):
        a, b = int(s["obs_begin"][j]), int(s["obs_begin"][j + 1])
        self.n, self.loss = b - a, _loss(s)
        P = OwnedProblem()
        P.cameras = cameras_of(s)
        P.extrinsics = np.asarray(s["extrinsics"], np.float64).reshape(-1, 7).copy()
        P.poses = np.asarray(s["pose"], np.float64).reshape(-1, 7)[j:j + 1].copy()
        P.pose_constant = np.zeros(1, np.uint8)
        P.landmarks = np.asarray(s["obs_point"], np.float64).reshape(-1, 4)[a:b].copy()
        P.landmark_constant = np.ones(self.n, np.uint8)
        P.obs_pose = np.zeros(self.n, np.int32)
        P.obs_landmark = np.arange(self.n, dtype=np.int32)
        P.obs_camera = np.asarray(s["obs_camera"], np.int32)[a:b].copy()
        P.obs_keypoint = np.asarray(s["obs_keypoint"], np.float64).reshape(-1, 2)[a:b].copy()
        P.obs_sqrt_info = np.asarray(s["obs_sqrt_info"], np.float64).reshape(-1, 4)[a:b].copy()
        P.obs_cauchy = np.zeros(self.n, np.uint8)
        self.P = P.bind()

    def raw(self, pose):
        """The weighted residuals without the loss [n, 2] and their minimal pose Jacobians [n, 2, 6]."""
        self.P.poses[0] = pose
        r, Jp, _ = _oracle.eval_reprojection(self.P.ptr(), self.n)
        return r, Jp

    def corrected(self, pose, jacobian=True):
        """(cost, r [2n], J [2n, 6]) with the Corrector applied block by block."""
        r, J = self.raw(pose)
        cost, c = 0.0, C.c_double()
        for i in range(self.n):
            _oracle.lib().oracle_loss_correct(C.byref(self.loss), 2, 6, og.dptr(r[i]), og.dptr(J[i]) if jacobian else None,
                                              C.byref(c))
            cost += c.value
        return cost, r.reshape(-1), J.reshape(-1, 6)


def _damped_solve(J, r, D, normal):
    """argmin |J y - r|^2 + |D y|^2, or None (a failed factorisation or a non-finite solution)."""
    try:
        if normal:
            L = np.linalg.cholesky(J.T @ J + np.diag(D * D))
            y = np.linalg.solve(L.T, np.linalg.solve(L, J.T @ r))
        else:
            y = np.linalg.lstsq(np.vstack([J, np.diag(D)]), np.concatenate([r, np.zeros(6)]), rcond=None)[0]
    except np.linalg.LinAlgError:
        return None
    return y if np.isfinite(y).all() else None


def _refine_job(s, j, normal):
    M = Margin()
    job = _Job(s, j)
    x = np.asarray(s["pose"], np.float64).reshape(-1, 7)[j].copy()
    out = {"pose": x.copy(), "H": np.zeros((6, 6)), "n_outliers": 0, "initial_cost": 0.0, "final_cost": 0.0,
           "num_iterations": 0, "num_successful_steps": 1, "num_unsuccessful_steps": 0, "termination_type": CONVERGENCE}
    if job.n == 0:
        return out, M.worst
    with np.errstate(all="ignore"):
        cost, r, J = job.corrected(x)
        out["initial_cost"] = cost
        if not (np.isfinite(cost) and np.isfinite(r).all() and np.isfinite(J).all()):
            out["termination_type"], out["final_cost"] = FAILURE, cost
        else:
            jscale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))

            def linearised(x, r, J):
                g = J.T @ r
                return J * jscale, float(np.abs(x - pose_plus(x, -g)).max()), float(np.linalg.norm(x))

            Js, gmax, x_norm = linearised(x, r, J)
            radius, decrease, reuse, diag = 1e4, 2.0, False, None
            min_cost, best = DBL_MAX, x.copy()
            it = succ = unsucc = invalid = 0
            ok, term = True, NO_CONVERGENCE
            while True:
                if ok:
                    succ += 1
                    if cost < min_cost:
                        min_cost, best = cost, x.copy()
                else:
                    unsucc += 1
                if it >= int(s["max_num_iterations"]):
                    term = NO_CONVERGENCE
                    break
                if M.le(gmax, 1e-10):
                    term = CONVERGENCE
                    break
                if radius <= 1e-32:
                    term = CONVERGENCE
                    break
                it += 1
                ok = False
                if not reuse:
                    diag = np.clip((Js * Js).sum(0), 1e-6, 1e32)
                reuse = True
                y = _damped_solve(Js, r, np.sqrt(diag / radius), normal)
                valid = False
                if y is not None:
                    step = -y
                    mr = Js @ step
                    mcc = -(mr @ (r + mr / 2.0))
                    valid = M.gt(mcc, 0.0, abs(mr @ r) + mr @ mr / 2.0)
                if not valid:
                    invalid += 1
                    if invalid >= 5:
                        term = FAILURE
                        it -= 1
                        break
                    radius /= decrease
                    decrease *= 2.0
                    continue
                invalid = 0
                cand = pose_plus(x, step * jscale)
                ccost = job.corrected(cand, jacobian=False)[0]
                if M.le(float(np.linalg.norm(x - cand)), 1e-8 * (x_norm + 1e-8)):
                    term = CONVERGENCE
                    it -= 1
                    break
                change = cost - ccost
                if M.le(abs(change), 1e-6 * cost):
                    term = CONVERGENCE
                    it -= 1
                    break
                rel = -DBL_MAX if ccost >= DBL_MAX else change / mcc
                if M.gt(rel, 1e-3):
                    x = cand
                    cost, r, J = job.corrected(x)
                    Js, gmax, x_norm = linearised(x, r, J)
                    ok = True
                    radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
                    decrease, reuse = 2.0, False
                else:
                    radius /= decrease
                    decrease *= 2.0
                    reuse = True
            out.update(pose=best if min_cost < DBL_MAX else x, final_cost=min(min_cost, cost), num_iterations=it,
                       num_successful_steps=succ, num_unsuccessful_steps=unsucc, termination_type=term)
        r, J = job.raw(out["pose"])  # :565-598
        for i in range(job.n):
            if M.gt(float(np.sqrt(r[i] @ r[i])), 3.0):
                out["n_outliers"] += 1
            else:
                out["H"] += J[i].T @ J[i]
    return out, M.worst


def _refine(s, normal):
    n = len(s["obs_begin"]) - 1
    jobs = [_refine_job(s, j, normal) for j in range(n)]
    out = {k: np.array([o[k] for o, _ in jobs], np.int32).reshape(n) for k in REFINE_INT_KEYS}
    out.update(pose=np.array([o["pose"] for o, _ in jobs]).reshape(n, 7), H=np.array([o["H"] for o, _ in jobs]).reshape(n, 6, 6),
               initial_cost=np.array([o["initial_cost"] for o, _ in jobs]).reshape(n),
               final_cost=np.array([o["final_cost"] for o, _ in jobs]).reshape(n),
               margin=min([m for _, m in jobs] + [np.inf]))
    return out


def refine_literal(s):
    return _refine(s, normal=False)


def refine_normal(s):
    return _refine(s, normal=True)


def refine_deviation(got, ref):
    """The largest deviation of the doubles: pose and costs scaled by max(1, |value|), H by its largest entry
    per job."""
    worst = 0.0
    with np.errstate(invalid="ignore"):
        for k in ("pose", "initial_cost", "final_cost"):
            a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
            same = (a == b) | (np.isnan(a) & np.isnan(b))
            d = np.where(same, 0.0, np.abs(a - b) / np.maximum(1.0, np.abs(b)))
            worst = max(worst, float(d.max()) if d.size else 0.0)
        for a, b in zip(np.asarray(got["H"]), np.asarray(ref["H"])):
            same = (a == b) | (np.isnan(a) & np.isnan(b))
            scale = np.abs(b[np.isfinite(b)]).max() if np.isfinite(b).any() else 1.0
            worst = max(worst, float(np.where(same, 0.0, np.abs(a - b) / (scale if scale > 0 else 1.0)).max()))
    return worst if not np.isnan(worst) else np.inf


RIG = [pinhole(1, (-0.12, 0.05, 4e-4, -3e-4)), pinhole(2, (0.02, -0.01, 0.004, -0.001)), pinhole(0)]
RIG_EXTRINSICS = np.array([[0.05, 0.0, 0.01, 0.0, 0.0, 0.0, 1.0],
                           [-0.06, 0.01, 0.0, 0.0, 0.008, 0.0, 1.0],
                           [0.0, -0.04, 0.02, 0.006, 0.0, -0.004, 1.0]])
RIG_EXTRINSICS[:, 3:] /= np.linalg.norm(RIG_EXTRINSICS[:, 3:], axis=1)[:, None]


def _project(cam, p):
    from _match import distort
    d = distort(cam, np.array([p[0] / p[2], p[1] / p[2]]))
    return np.array([cam["fu"] * d[0] + cam["cu"], cam["fv"] * d[1] + cam["cv"]])


def refine_job(seed, n, cams=(0, 1), noise=0.4, start=((0.02, -0.015, 0.01), (0.006, -0.004, 0.008)), outliers=0,
               truth=(0.3, -0.1, 0.2, 0.03, -0.05, 0.02)):
    """One candidate: n inlier observations alternating over `cams` of the rig, the points 2-8 m in front of
    their camera, keypoints with Gaussian pixel noise, sizes 6-12; the first `outliers` keypoints are moved by
    40-80 px. The pose starts at the ground truth T_Sold_Snew moved by `start` (position, small angle)."""
    rng = np.random.default_rng(seed)
    T = box_plus(IDENT, np.array(truth[:3]), np.array(truth[3:]))
    C_T = rotation(T[3:])
    job = {"pose": box_plus(T, np.array(start[0]), np.array(start[1])), "truth": T, "obs_camera": [], "obs_keypoint": [],
           "obs_sqrt_info": [], "obs_point": []}
    for i in range(n):
        c = cams[i % len(cams)]
        z = rng.uniform(2.0, 8.0)
        p_C = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z])
        p_new = rotation(RIG_EXTRINSICS[c, 3:]) @ p_C + RIG_EXTRINSICS[c, :3]
        kp = _project(RIG[c], p_C) + noise * rng.standard_normal(2)
        if i < outliers:
            kp += rng.uniform(40.0, 80.0) * np.array([np.cos(i), np.sin(i)])
        job["obs_camera"].append(c)
        job["obs_keypoint"].append(kp)
        job["obs_sqrt_info"].append(np.array([1.0, 0.0, 0.0, 1.0]) * 8.0 / rng.uniform(6.0, 12.0))
        job["obs_point"].append(np.array([*(C_T @ p_new + T[:3]), 1.0]))
    return job


def refine_scene(jobs, max_num_iterations=10, loss=("cauchy", 3.0)):
    cat = lambda k, w: np.concatenate([np.asarray(j[k], np.float64).reshape(-1, w) for j in jobs] + [np.zeros((0, w))])
    return {"cameras": RIG, "extrinsics": RIG_EXTRINSICS.copy(), "loss": loss, "max_num_iterations": max_num_iterations,
            "pose": np.array([j["pose"] for j in jobs]).reshape(len(jobs), 7),
            "truth": np.array([j["truth"] for j in jobs]).reshape(len(jobs), 7),
            "obs_begin": np.concatenate([[0], np.cumsum([len(j["obs_camera"]) for j in jobs])]).astype(np.int32),
            "obs_camera": np.concatenate([np.asarray(j["obs_camera"], np.int32) for j in jobs] + [np.zeros(0, np.int32)]),
            "obs_keypoint": cat("obs_keypoint", 2), "obs_sqrt_info": cat("obs_sqrt_info", 4), "obs_point": cat("obs_point", 4)}


def refine_sub_scene(s, jobs):
    t = dict(s)
    rows = [np.arange(int(s["obs_begin"][j]), int(s["obs_begin"][j + 1])) for j in jobs]
    idx = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
    t["pose"], t["truth"] = s["pose"][list(jobs)].copy(), s["truth"][list(jobs)].copy()
    t["obs_begin"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    for k in ("obs_camera", "obs_keypoint", "obs_sqrt_info", "obs_point"):
        t[k] = s[k][idx].copy()
    return t
