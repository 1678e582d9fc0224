"""The keypoint-against-keypoint matching of Frontend::matchMotionStereo (mode 0) and Frontend::matchStereo
(mode 1) restated in numpy (test infrastructure for okvisgpu_match_frames; reference:
okvis_frontend/src/Frontend.cpp:2057-2149 and :2259-2316, stereo_triangulation.cpp:30-112,
PinholeCamera.hpp:249-284 and 485-494).

  literal(scene)   the reference's loops as written: per side-0 keypoint a serial walk over the side-1
                   keypoints with a running best. Also returns the smallest margin of any floating-point
                   comparison it decided and the branch statistics the tests ask for.
  ordered(scene)   the parallel formulation: every candidate below the starting best is tested for
                   admissibility on its own; the match is the first minimum in order among the admissible
                   ones; mode 0's projection check runs on that winner only.
  scene(...)       a scene from a list of jobs; side(...) one side of a job from 3D points.

A scene is a dict with the arguments of okvisgpu.frame_match_batch, cameras as dicts (distortion, width,
height, fu, fv, cu, cv, dist[8]): cameras, matching_threshold, job_mode, job_camera0/1, job_pose0/1,
job_extrinsics0/1, kp0_begin, kp1_begin and per side keypoint, size, descriptor, ray, ray_valid, use.

Margins: every floating-point comparison that decides a branch goes through Margin (tests/_match.py).
Comparisons of Hamming distances with the threshold are comparisons of an integer with a constant and
cannot flip through rounding."""
import numpy as np

from _match import (Margin, compose, flip_bits, hamming, normalised, pinhole, project_homogeneous,  # noqa: F401
                    triangulate_fast, worst_relative)

INT_KEYS = ("match", "distance", "initialisable")
REAL_KEYS = ("point", "quality")
KEYS = INT_KEYS + REAL_KEYS
SIDE_KEYS = ("keypoint", "size", "descriptor", "ray", "ray_valid", "use")
MIN_DEPTH = (0.2, 0.1)


def _outputs(s):
    n = int(s["kp0_begin"][-1]) if len(s["kp0_begin"]) else 0
    return {"match": np.full(n, -1, np.int32), "distance": np.full(n, -1, np.int32), "point": np.zeros((n, 4)),
            "initialisable": np.zeros(n, np.uint8), "quality": np.zeros(n)}


def _job(s, j):
    """The job's mode, cameras, transforms, focal lengths, keypoint ranges and Hamming table."""
    c0, c1 = s["cameras"][int(s["job_camera0"][j])], s["cameras"][int(s["job_camera1"][j])]
    C0, r0 = compose(s["job_pose0"][j], s["job_extrinsics0"][j])
    C1, r1 = compose(s["job_pose1"][j], s["job_extrinsics1"][j])
    a0, b0, a1, b1 = (int(s[k][j + d]) for k in ("kp0_begin", "kp1_begin") for d in (0, 1))
    dist = hamming(s["descriptor0"][a0:b0], s["descriptor1"][a1:b1]) if b0 > a0 and b1 > a1 else \
        np.zeros((b0 - a0, b1 - a1), np.int32)
    return {"mode": int(s["job_mode"][j]), "cam1": c1, "C0": C0, "r0": r0, "C1": C1, "r1": r1,
            "f0": 0.5 * (c0["fu"] + c0["fv"]), "f1": 0.5 * (c1["fu"] + c1["fv"]), "a0": a0, "n0": b0 - a0, "a1": a1,
            "n1": b1 - a1, "dist": dist}


def _use(s, side, k):
    u = s.get(f"use{side}")
    return True if u is None else bool(u[k])


def _final_check(s, J, point, k1, M):
    """Mode 0's :2140-2147 on the record: (kept, projection status)."""
    hp_C = np.array([*(J["C1"].T @ (point[:3] - J["r1"] * point[3])), point[3]])
    status, px = project_homogeneous(J["cam1"], hp_C, M)
    if status != "ok":
        return False, status
    return (True, status) if M.lt(np.linalg.norm(s["keypoint1"][J["a1"] + k1] - px), 4.0) else (False, "far")


def literal(s):
    """The reference's loops. Returns the outputs of okvisgpu_match_frames plus 'margin' and 'stats'."""
    M = Margin()
    out = _outputs(s)
    thr = float(s["matching_threshold"])
    stats = {"matches": [0, 0], "rejected_geometry": 0, "parallel_winners": 0, "final_failures": []}
    for j in range(len(s["job_mode"])):
        J = _job(s, j)
        C0, r0, C1, r1, mode = J["C0"], J["r0"], J["C1"], J["r1"], J["mode"]
        for k0 in range(J["n0"]):
            g0 = J["a0"] + k0
            if not _use(s, 0, g0):
                continue
            if mode == 0:
                distances = int(np.uint32(thr)) if thr > 0 else 0  # uint32_t distances = briskMatchingThreshold_
                if not s["ray_valid0"][g0]:
                    continue
                e0 = normalised(C0 @ s["ray0"][g0])
                sigma = s["size0"][g0] / J["f0"] * 0.125
            else:
                distances = thr
            initialisable, quality, hps, k1_match = False, 0.0, np.zeros(4), None
            for k1 in range(J["n1"]):
                g1 = J["a1"] + k1
                if not _use(s, 1, g1):
                    continue
                dist = int(J["dist"][k0, k1])
                if not dist < distances:
                    continue
                if mode == 1:
                    sigma = max(s["size0"][g0] / J["f0"], s["size1"][g1] / J["f1"]) * 0.125
                    if not s["ray_valid0"][g0]:
                        continue
                if not s["ray_valid1"][g1]:
                    continue
                if mode == 1:
                    e0 = normalised(C0 @ s["ray0"][g0])
                e1 = normalised(C1 @ s["ray1"][g1])
                if mode == 0 and M.lt(e0 @ e1, 0.5):
                    stats["rejected_geometry"] += 1
                    continue
                p, valid, parallel = triangulate_fast(r0, e0, r1, e1, sigma, M)
                if mode == 0 and not valid:
                    stats["rejected_geometry"] += 1
                    continue
                depth0, depth1 = (C0.T @ (p - r0))[2], (C1.T @ (p - r1))[2]
                if M.lt(e0 @ e1, 0.8):
                    valid = False
                if M.lt(depth0, MIN_DEPTH[mode]):
                    valid = False
                if M.lt(depth1, MIN_DEPTH[mode]):
                    valid = False
                if not valid:
                    stats["rejected_geometry"] += 1
                    continue
                k1_match, distances, hps, initialisable = k1, dist, np.array([*p, 1.0]), not parallel
                if mode == 0:
                    quality = M.acos(normalised(p - r0) @ normalised(p - r1))
            if not distances < thr or k1_match is None:  # (no record: the reference projects a zero point, Invalid)
                continue
            if mode == 0:
                kept, status = _final_check(s, J, hps, k1_match, M)
                if not kept:
                    stats["final_failures"].append((j, k0, status))
                    continue
            out["match"][g0], out["distance"][g0], out["point"][g0] = k1_match, distances, hps
            out["initialisable"][g0], out["quality"][g0] = initialisable, quality
            stats["matches"][mode] += 1
            stats["parallel_winners"] += not initialisable
    out["margin"] = M.worst
    out["stats"] = stats
    return out


def ordered(s):
    """The parallel formulation: admissibility of every candidate below the starting best on its own, the
    first minimum in order among the admissible ones, then mode 0's check on that winner."""
    M = Margin()
    out = _outputs(s)
    thr = float(s["matching_threshold"])
    for j in range(len(s["job_mode"])):
        J = _job(s, j)
        C0, r0, C1, r1, mode = J["C0"], J["r0"], J["C1"], J["r1"], J["mode"]
        start = (int(np.uint32(thr)) if thr > 0 else 0) if mode == 0 else thr
        for k0 in range(J["n0"]):
            g0 = J["a0"] + k0
            if not _use(s, 0, g0) or not s["ray_valid0"][g0]:
                continue
            e0 = normalised(C0 @ s["ray0"][g0])
            admissible = {}
            for k1 in range(J["n1"]):
                g1 = J["a1"] + k1
                if not _use(s, 1, g1) or not s["ray_valid1"][g1] or not int(J["dist"][k0, k1]) < start:
                    continue
                e1 = normalised(C1 @ s["ray1"][g1])
                if mode == 0:
                    sigma = s["size0"][g0] / J["f0"] * 0.125
                    if e0 @ e1 < 0.5:
                        continue
                else:
                    sigma = max(s["size0"][g0] / J["f0"], s["size1"][g1] / J["f1"]) * 0.125
                p, valid, parallel = triangulate_fast(r0, e0, r1, e1, sigma, M)
                depth0, depth1 = (C0.T @ (p - r0))[2], (C1.T @ (p - r1))[2]
                if valid and not e0 @ e1 < 0.8 and not depth0 < MIN_DEPTH[mode] and not depth1 < MIN_DEPTH[mode]:
                    admissible[k1] = (p, parallel)
            if not admissible:
                continue
            best = min(int(J["dist"][k0, k1]) for k1 in admissible)
            k1 = min(k for k in admissible if int(J["dist"][k0, k]) == best)
            p, parallel = admissible[k1]
            hps = np.array([*p, 1.0])
            if mode == 0 and not _final_check(s, J, hps, k1, M)[0]:
                continue
            out["match"][g0], out["distance"][g0], out["point"][g0] = k1, best, hps
            out["initialisable"][g0] = not parallel
            if mode == 0:
                with np.errstate(invalid="ignore"):
                    out["quality"][g0] = np.arccos(normalised(p - r0) @ normalised(p - r1))
    return out


# ------------------------------------------------------------------------------------------ scenes
IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def at(x, y=0.0, z=0.0):
    """The pose at (x, y, z) with the identity rotation."""
    return np.array([x, y, z, 0.0, 0.0, 0.0, 1.0])


def side(cam, T_WS, T_SC, points, descriptors, rng=None, pixel_noise=0.0, ray_noise=0.0, size=8.0, valid=None,
         use=None):
    """One side of a job from 3D points in W: the (undistorted) back-projection p_C / p_C.z as ray, the
    camera's projection as keypoint (also where it falls outside the image), both with optional noise."""
    C, r = compose(np.asarray(T_WS, np.float64), np.asarray(T_SC, np.float64))
    n = len(points)
    kp, ray = np.zeros((n, 2)), np.zeros((n, 3))
    for i, p in enumerate(np.asarray(points, np.float64).reshape(-1, 3)):
        p_C = C.T @ (p - r)
        ray[i] = p_C / p_C[2]
        status, px = project_homogeneous(cam, np.array([*p_C, 1.0]))
        kp[i] = px if px is not None else 0.0
        if rng is not None:
            ray[i, :2] += rng.normal(0.0, ray_noise, 2)
            kp[i] += rng.normal(0.0, pixel_noise, 2)
    return {"keypoint": kp, "size": np.full(n, size) if np.isscalar(size) else np.asarray(size, np.float64),
            "descriptor": np.asarray(descriptors, np.uint8).reshape(n, 48), "ray": ray,
            "ray_valid": np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8),
            "use": np.ones(n, np.uint8) if use is None else np.asarray(use, np.uint8)}


def empty_side():
    return {"keypoint": np.zeros((0, 2)), "size": np.zeros(0), "descriptor": np.zeros((0, 48), np.uint8),
            "ray": np.zeros((0, 3)), "ray_valid": np.zeros(0, np.uint8), "use": np.zeros(0, np.uint8)}


def job(mode, camera0, camera1, pose0, pose1, ext0, ext1, side0, side1):
    return {"mode": mode, "camera0": camera0, "camera1": camera1, "pose0": pose0, "pose1": pose1, "ext0": ext0,
            "ext1": ext1, "side0": side0, "side1": side1}


def scene(cameras, jobs, matching_threshold=60.0):
    s = {"cameras": cameras, "matching_threshold": matching_threshold,
         "job_mode": np.array([j["mode"] for j in jobs], np.int32),
         "job_camera0": np.array([j["camera0"] for j in jobs], np.int32),
         "job_camera1": np.array([j["camera1"] for j in jobs], np.int32),
         "job_pose0": np.array([j["pose0"] for j in jobs], np.float64).reshape(-1, 7),
         "job_pose1": np.array([j["pose1"] for j in jobs], np.float64).reshape(-1, 7),
         "job_extrinsics0": np.array([j["ext0"] for j in jobs], np.float64).reshape(-1, 7),
         "job_extrinsics1": np.array([j["ext1"] for j in jobs], np.float64).reshape(-1, 7)}
    for sd in (0, 1):
        parts = [j[f"side{sd}"] for j in jobs] or [empty_side()]
        s[f"kp{sd}_begin"] = np.concatenate([[0], np.cumsum([len(j[f"side{sd}"]["size"]) for j in jobs])]).astype(np.int32)
        for k in SIDE_KEYS:
            s[f"{k}{sd}"] = np.ascontiguousarray(np.concatenate([p[k] for p in parts]))
    return s


def sub_scene(s, jobs):
    """The scene restricted to the given jobs (in the given order)."""
    t = {"cameras": s["cameras"], "matching_threshold": s["matching_threshold"]}
    for k in ("job_mode", "job_camera0", "job_camera1", "job_pose0", "job_pose1", "job_extrinsics0", "job_extrinsics1"):
        t[k] = np.ascontiguousarray(np.asarray(s[k])[list(jobs)])
    for sd in (0, 1):
        rng = [(int(s[f"kp{sd}_begin"][j]), int(s[f"kp{sd}_begin"][j + 1])) for j in jobs]
        t[f"kp{sd}_begin"] = np.concatenate([[0], np.cumsum([b - a for a, b in rng])]).astype(np.int32)
        for k in SIDE_KEYS:
            t[f"{k}{sd}"] = np.ascontiguousarray(np.concatenate([s[f"{k}{sd}"][a:b] for a, b in rng] or [s[f"{k}{sd}"][:0]]))
    return t


def job_rows(s, out, j):
    """Job j's part of every output."""
    a, b = int(s["kp0_begin"][j]), int(s["kp0_begin"][j + 1])
    return {k: out[k][a:b] for k in KEYS}
