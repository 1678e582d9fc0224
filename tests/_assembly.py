"""Helpers of tests/test_assembly_paths.py: the assembly record restated from the planner's separate
arrays, and small windows shaped by the observations they keep."""
import numpy as np

from _problem import _ARRAYS, OwnedProblem

LIGHT_MAX = 24  # device_problem.hpp kAsmLightMax


def expected_records(arrays):
    """What okvisgpu_plan_assembly's records must hold, from its `arrays` (the values the kernels
    used to fetch through asm_*_items, pair_*, fb_off, fb_kind, win_foff, win_fpad, win_soff)."""
    a = np.asarray(arrays, np.int64)
    k, w, cb, pb, ob, ce, fi, fj, offi, offj, ki, kj, foff, fpad, soff = (a[:, c] for c in range(15))
    dst = soff + offi * fpad + offj
    flags = (fi == fj).astype(np.int64) | (ki != 0).astype(np.int64) << 1 | (kj != 0).astype(np.int64) << 2
    rec = np.stack([w, cb, pb, ob, ce, foff + offi, foff + offj, fpad, dst & 0xFFFFFFFF, dst >> 32, flags,
                    np.zeros_like(k)], axis=1)
    rec[k < 0] = 0
    rec[k < 0, 0] = -1
    return (rec & 0xFFFFFFFF).astype(np.uint32).view(np.int32)  # (as the int32 words of the record)


def owned(og, kf, lm, obs, seed, **cfg):
    return OwnedProblem.copy_of(og.SynthWindow(kf, lm, obs, seed=seed, **cfg).problem)


def keep_observations(P, keep):
    """Keeps the observations of the mask and the landmarks that still have one (renumbered)."""
    for k, (_, _, cnt) in _ARRAYS.items():
        if cnt == "n_observations":
            setattr(P, k, getattr(P, k)[keep])
    used = np.unique(P.obs_landmark)
    remap = np.full(len(P.landmarks), -1, np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    P.obs_landmark = remap[P.obs_landmark]
    P.landmarks = P.landmarks[used]
    P.landmark_constant = P.landmark_constant[used]
    return P.bind()


def landmark_poses(P):
    """Per landmark the sorted poses that observe it."""
    per = [[] for _ in range(len(P.landmarks))]
    for l, p in sorted(set(zip(P.obs_landmark.tolist(), P.obs_pose.tolist()))):
        per[l].append(p)
    return per


def keep_landmarks_of(P, plan):
    """plan: list of (poses, count): keeps, for each entry, `count` landmarks (not used by an earlier
    entry) that every pose of `poses` observes, with their observations from those poses only.
    Returns the mask over observations."""
    per = landmark_poses(P)
    taken = np.zeros(len(P.landmarks), bool)
    keep = np.zeros(len(P.obs_landmark), bool)
    for poses, count in plan:
        cands = [l for l in range(len(per)) if not taken[l] and all(p in per[l] for p in poses)]
        assert len(cands) >= count, (poses, count, len(cands))
        for l in cands[:count]:
            taken[l] = True
            keep |= (P.obs_landmark == l) & np.isin(P.obs_pose, poses)
    return keep


CHAIN_COUNTS = (1, 7, 8, 9, 16, 17, 32, 33, 64, 65)


def chain_window(og, per_group, seed, counts=CHAIN_COUNTS, **cfg):
    """A window of 2 + len(counts) keyframes whose landmark groups hold `per_group` landmarks each
    (the planner's bound: 16 alone, 64 in a large batch): keyframes 0 and 1 see every landmark, keyframe
    2 + k sees one landmark (slot k % 2) of each of the first counts[k] groups. So the diagonal pair of
    keyframe 2 + k has counts[k] visit segments, its pairs with keyframes 0 and 1 have counts[k] partial
    blocks, and neighbouring keyframes from 2 on share no landmark (factor blocks only)."""
    n_kf, n_grp = 2 + len(counts), max(counts)
    n_lm = n_grp * per_group
    P = owned(og, n_kf, n_lm, 2 * n_kf * n_lm, seed=seed, max_obs_per_landmark=2 * n_kf, kf_dt_s=0.02, **cfg)
    assert len(P.landmarks) == n_lm and all(len(p) == n_kf for p in landmark_poses(P))
    keep = P.obs_pose < 2
    grp, slot = P.obs_landmark // per_group, P.obs_landmark % per_group
    for k, c in enumerate(counts):
        keep |= (P.obs_pose == 2 + k) & (grp < c) & (slot == k % 2)
    return keep_observations(P, keep)


def pair_runs(rec):
    """(visit segments, partial blocks, factor blocks, flags) per live record."""
    r = rec[rec[:, 0] >= 0].astype(np.int64)
    return r[:, 2] - r[:, 1], r[:, 3] - r[:, 2], r[:, 4] - r[:, 3], r[:, 10]


def with_sb_priors(P, blocks):
    """Adds one speed/bias prior per entry of `blocks` (repeats allowed: several priors on one
    block), each a scaled copy of the window's first prior around a shifted measurement."""
    n = len(blocks)
    scale = np.array([1.0, 0.5, 2.0, 0.25, 1.5])[np.arange(n) % 5][:, None]
    P.sb_prior_block = np.concatenate([P.sb_prior_block, blocks]).astype(np.int32)
    P.sb_prior_meas = np.concatenate([P.sb_prior_meas, P.speed_biases[blocks] + 0.01])
    P.sb_prior_sqrt_info = np.concatenate([P.sb_prior_sqrt_info, np.repeat(P.sb_prior_sqrt_info[:1], n, 0) * scale])
    return P.bind()


def retry_window(og, seed, j=5):
    """An S10 window with an extra state (index j) whose only residual is a constant host factor
    (test_lm_visit_paths._retry): its 15 columns of J are zero and its pivot is min_lm_diagonal * mu,
    so with a tiny min_lm_diagonal the Gauss-Newton step fails until mu has risen."""
    P = owned(og, 10, 500, 4000, seed=seed)
    P.poses = np.insert(P.poses, j, P.poses[j], axis=0)
    P.speed_biases = np.insert(P.speed_biases, j, P.speed_biases[j], axis=0)
    P.pose_constant = np.insert(P.pose_constant, j, 0)
    P.speed_bias_constant = np.insert(P.speed_bias_constant, j, 0)
    P.obs_pose = np.where(P.obs_pose >= j, P.obs_pose + 1, P.obs_pose)
    P.imu_blocks = np.where(P.imu_blocks >= j, P.imu_blocks + 1, P.imu_blocks)
    P.pose_prior_block = np.where(P.pose_prior_block >= j, P.pose_prior_block + 1, P.pose_prior_block)
    P.sb_prior_block = np.where(P.sb_prior_block >= j, P.sb_prior_block + 1, P.sb_prior_block)
    P.host_dim = np.array([1], np.int32)
    P.host_param_kind = np.array([[0, 1, -1, -1]], np.int32)
    P.host_param_index = np.array([[j, j, -1, -1]], np.int32)
    P.host_cauchy = np.zeros(1, np.uint8)
    P.host_fn = og.host_evaluate(lambda h, prm: (np.array([0.1]), [np.zeros((1, 7)), np.zeros((1, 9))]), [[7, 9]])
    return P.bind()
