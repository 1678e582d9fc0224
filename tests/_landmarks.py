"""Numpy restatement of ViGraph::updateLandmarks (okvis_ceres/src/ViGraph.cpp:1762-1841) and
ViGraph::areLandmarksInFrontOfCameras (:1621-1642) on the arrays of one okvisgpu_problem — TEST
INFRASTRUCTURE ONLY: the checker of okvisgpu_update_landmarks.

The per-observation norm of the weighted reprojection residual (`err`, no loss) is an input: the
oracle's oracle_eval_reprojection (or any other evaluation of ReprojectionError::Evaluate) supplies
it, so this file restates only the landmark logic.

Every threshold decision comes with its margin, the distance of the compared value from the
threshold; a decision with a margin below MARGIN can flip with rounding and says nothing about the
code under test. Per landmark, `margin` is the smallest of
    |err - 2.5|                       per observation (the error gate)
    |z - 0.1|, |z|                    per observation (behind, ray reversal; z of the divided point)
    | ||pos_C|| - 1e-4 |              per kept observation (4-vector norm, the best-fit gate)
    second-best err - best err        among the kept observations that pass that gate
    |quality - 0.04|
    |z_u| and |z_u / w - 0.05|        per observation with w != 0 (the in-front test on the undivided
                                      point: w is the landmark's own fourth coordinate, copied, so
                                      the sign of z_u * w turns only with z_u, and with w == 0 the
                                      product is an exact zero and the ratio is not formed)
The comparisons of |w| with 1e-12 and 1e-16 are exact for the same reason and have no margin.
"""
import numpy as np

MARGIN = 1e-9


def rot(q):
    """Eigen::Quaterniond(x, y, z, w).toRotationMatrix() of the normalised quaternion."""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def camera_frames(poses, extrinsics):
    """C_WC [n_poses, n_cam, 3, 3] and r_WC [n_poses, n_cam, 3] of T_WC = T_WS T_SC."""
    C = np.zeros((len(poses), len(extrinsics), 3, 3))
    r = np.zeros((len(poses), len(extrinsics), 3))
    for i, T_WS in enumerate(poses):
        C_WS = rot(T_WS[3:7])
        for c, T_SC in enumerate(extrinsics):
            C[i, c] = C_WS @ rot(T_SC[3:7])
            r[i, c] = C_WS @ T_SC[:3] + T_WS[:3]
    return C, r


def observation_order(obs_pose, obs_landmark, obs_camera, n_landmarks):
    """Per landmark, its observations in (pose, camera, index) order (the KeypointIdentifier map order)."""
    runs = [[] for _ in range(n_landmarks)]
    for o in np.lexsort((np.arange(len(obs_pose)), obs_camera, obs_pose)):
        runs[obs_landmark[o]].append(int(o))
    return runs


def update_landmarks(poses, extrinsics, landmarks, obs_pose, obs_landmark, obs_camera, err):
    """Returns a dict: quality, initialised, reset [n_lm]; landmarks [n_lm, 4] after the resets; skip
    [n_obs] (err > 2.5); n_initialised, n_reset, in_front; margin [n_lm]; reset_distance [n_lm] (the
    distance of a reset landmark from the camera it was re-placed in front of, else nan)."""
    poses, extrinsics = np.asarray(poses, dtype=np.float64), np.asarray(extrinsics, dtype=np.float64)
    landmarks = np.asarray(landmarks, dtype=np.float64)
    err = np.asarray(err, dtype=np.float64)
    n_lm = len(landmarks)
    C_WC, r_WC = camera_frames(poses, extrinsics)
    out = {"quality": np.zeros(n_lm), "initialised": np.zeros(n_lm, dtype=bool), "reset": np.zeros(n_lm, dtype=bool),
           "landmarks": landmarks.copy(), "skip": err > 2.5, "margin": np.full(n_lm, np.inf),
           "reset_distance": np.full(n_lm, np.nan), "in_front": True}
    for l, run in enumerate(observation_order(obs_pose, obs_landmark, obs_camera, n_lm)):
        hp = landmarks[l]
        behind = False
        best, best_err, second_err, best_dist = None, 1.0e12, np.inf, np.nan
        dirs = []
        margin = np.inf
        for o in run:
            C, r = C_WC[obs_pose[o], obs_camera[o]], r_WC[obs_pose[o], obs_camera[o]]
            w = hp[3]
            pos = C.T @ hp[:3] - (C.T @ r) * w
            # areLandmarksInFrontOfCameras, on the undivided point
            if pos[2] * w < 0.0:
                out["in_front"] = False
            if abs(w) > 1.0e-16 and pos[2] / w < 0.05:
                out["in_front"] = False
            if w != 0.0:
                margin = min(margin, abs(pos[2]), abs(pos[2] / w - 0.05))
            if abs(w) > 1.0e-12:
                pos = pos / w
                w = 1.0
            d = C @ pos
            n2 = d @ d
            if n2 > 0.0:
                d = d / np.sqrt(n2)
            z = pos[2]
            margin = min(margin, abs(z - 0.1), abs(z), abs(err[o] - 2.5))
            if z < 0.1:
                behind = True
            if z < 0.0:
                d = -d
            if err[o] > 2.5:
                continue
            n4 = np.sqrt(pos @ pos + w * w)
            margin = min(margin, abs(n4 - 1.0e-4))
            if n4 > 1.0e-4:
                if err[o] < best_err:
                    second_err = best_err
                    best_dist = max(0.1, n4)
                    best, best_err = r + best_dist * d, err[o]
                else:
                    second_err = min(second_err, err[o])
            dirs.append(d)
        q = 0.0
        if dirs:
            D = np.array(dirs)
            mean = D.sum(axis=0) / len(dirs)
            s = np.sqrt(((D - mean) ** 2).sum(axis=0))
            q = float(np.sqrt(s @ s))
        if run:
            margin = min(margin, abs(q - 0.04))
            if best is not None and second_err < 1.0e12:
                margin = min(margin, second_err - best_err)
        out["quality"][l] = q
        out["margin"][l] = margin
        if q > 0.04:
            out["initialised"][l] = True
        elif behind and best is not None:
            out["reset"][l] = True
            out["landmarks"][l] = [best[0], best[1], best[2], 1.0]
            out["reset_distance"][l] = best_dist
    out["n_initialised"] = int(out["initialised"].sum())
    out["n_reset"] = int(out["reset"].sum())
    return out


def decided(ref):
    """Landmarks whose every decision is clear of its threshold (the others are not compared)."""
    return ref["margin"] >= MARGIN
