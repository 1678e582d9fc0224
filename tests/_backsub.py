"""Windows shaped for the paths of k_lm_backsub_jv (kernels_backsub.hip) and the planner's grouping
restated with the observations of every group. Plain data only - no solver logic."""
import numpy as np

import okvisgpu as og
from test_lm_visit_paths import GROUP_PRODUCTS, _fixed, _full, _owned, _plain, _retry  # noqa: F401

STAGE_OBS = 512  # kernels_backsub.hip kBsStageObs: observations of a group that the LDS stage holds


def obs_groups(P, bounds):
    """The planner's landmark groups (plan.cpp WindowPlan::groups, as test_lm_visit_paths._groups
    restates them) of a window without variable extrinsics, as (first observation, observations,
    visits, landmarks) per group. Observations are ordered by (landmark, pose, camera) in the
    planner's landmark order, and a group is a range of whole landmarks, so its observations are
    one contiguous range: the first observation is the count of all groups before it."""
    max_visits, max_lms = bounds
    pose_free = P.pose_constant == 0
    per_lm, n_obs = {}, {}
    for l, p in zip(P.obs_landmark.tolist(), P.obs_pose.tolist()):
        n_obs[l] = n_obs.get(l, 0) + 1
        per_lm.setdefault(l, set()).add(p)
    order = sorted(range(len(P.landmarks)), key=lambda l: min(per_lm.get(l, [len(P.poses)])))
    out, first, no, nv, nl, npc = [], 0, 0, 0, 0, 0
    for l in order:
        poses = per_lm.get(l, ())
        nf = 0 if P.landmark_constant[l] else sum(1 for p in poses if pose_free[p])
        pcl = nf * (nf + 1) // 2
        if nl > 0 and (nv + len(poses) > max_visits or nl == max_lms or npc + pcl > GROUP_PRODUCTS):
            out.append((first, no, nv, nl))
            first, no, nv, nl, npc = first + no, 0, 0, 0, 0
        no += n_obs.get(l, 0)
        nv += len(poses)
        nl += 1
        npc += pcl
    if nl:
        out.append((first, no, nv, nl))
    return out


def _drop(P, drop):
    """Removes the observations of the mask (every landmark keeps at least one)."""
    from test_lm_visit_paths import _keep_observations
    n = len(P.landmarks)
    P = _keep_observations(P, ~drop)
    assert len(P.landmarks) == n
    return P


def full():
    """test_lm_visit_paths' full window (32 landmarks x 8 keyframes = 256 visits, then a landmark
    seen from one keyframe), every visit through both cameras but the last, which keeps camera 0:
    512 observations, then 1. The last landmark is held constant: one observation does not
    determine a point, and with it free the solve is so badly conditioned that device and oracle
    agree in the final cost to 1.3e-6 only (measured, before and after the stage alike); its
    observation remains a residual of its keyframe."""
    P = _full(og)
    P = _drop(P, (P.obs_landmark == 32) & (P.obs_camera == 1))
    P.landmark_constant[32] = 1
    return P.bind()


def mono():
    """An S10 window through camera 0 only: every visit has one observation."""
    P = _owned(og, 10, 500, 4000, seed=3301)
    return _drop(P, P.obs_camera != 0)


def three_cameras():
    """The full window with a third camera, a copy of camera 1 that repeats its observations: three
    observations per visit, 768 in a group of 256 visits."""
    P = full()
    cam = og.Camera()
    import ctypes as C
    C.pointer(cam)[0] = P.cameras[1]
    P.cameras = P.cameras + [cam]
    P.extrinsics = np.concatenate([P.extrinsics, P.extrinsics[1:2]])
    P.extrinsics_constant = np.ones(3, np.uint8)
    c1 = P.obs_camera == 1
    for k in ("obs_pose", "obs_landmark", "obs_keypoint", "obs_sqrt_info", "obs_cauchy"):
        setattr(P, k, np.concatenate([getattr(P, k), getattr(P, k)[c1]]))
    P.obs_camera = np.concatenate([P.obs_camera, np.full(int(c1.sum()), 2, np.int32)])
    return P.bind()


def fixed():
    return _fixed(og)


def plain():
    return _plain(og)


def retry():
    return _retry(og)
