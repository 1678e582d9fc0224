"""The landmark-group kernel body (kernels_schur.hip lmVisitGroup, shared by k_lm_visit<0|1|2>,
k_lm_prep_windows and k_lin_few) on small windows shaped to reach each of its paths, GPU against the
oracle: the reduced system through okvisgpu_linearize_reduce (S and rhs, 1e-11 relative to the
largest entry, the bound of test_gpu_parity.test_linearize_reduce_parity) and a 3-iteration solve
(the bounds of test_gpu_parity.test_solve_parity_s10).

Every shaped window runs twice, because the batch size decides the kernels and the group bounds
(plan.hpp, on the 256 CUs of an MI355X): alone, the groups hold at most 64 visits / 16 landmarks and
the linearisation and the GN prep are k_lin_few; in a batch of 66 windows the groups hold up to 256
visits / 64 landmarks, the linearisation is k_lm_visit<1> and the GN prep k_lm_prep_windows.

The shapes (each test first checks, from the context's statistics and the summaries, that its window
really has the property it is there for; `_groups` restates the planner's grouping rule, and the
statistics confirm its visit and segment counts):
  * wide    20 keyframes that all see the same 9 landmarks: groups of 20 segments (one in the batch,
            three alone), so the segment pass of 18 values per segment (360 sums on 256 threads)
            takes its strided second round;
  * spread  50 keyframes, 60 landmarks of 4 keyframes each: in the batch one group of >= 43 segments,
            so all three segment passes (9 values on three wavefronts, 18 and 6 on four) take a
            second round;
  * full    in the batch a group of exactly 256 visits (every thread a visit, every slot of every
            row taken) followed by a last group of a single visit; alone four groups of exactly 64;
  * fixed   two constant poses and every seventh landmark constant: visits without a slot, landmarks
            without an LLT, and observations masked because all their blocks are constant;
  * retry   a window whose Gauss-Newton step fails at the first values of mu (a state whose columns
            of J are zero, min_lm_diagonal small enough to underflow): the GN prep (mode 2) runs
            after the linearisation (mode 1) on the same buffers;
  * plain   an S10 window, also compared alone against in the batch.
"""
import numpy as np
import pytest

from _problem import _ARRAYS, OwnedProblem

pytestmark = pytest.mark.gpu

GROUP_PRODUCTS = 2048               # device_problem.hpp kLmPartStage
BIG, SMALL = (256, 64), (64, 16)    # group bounds (visits, landmarks): plan.cpp planOptions
S_TOL = 1e-11
N_BATCH = 66
MU_FLOOR = 1e-8                     # a solve without retries ends at this mu (Ceres: mu / 5 per step, floored)


def _owned(og, kf, lm, obs, seed, **cfg):
    return OwnedProblem.copy_of(og.SynthWindow(kf, lm, obs, seed=seed, **cfg).problem)


def _keep_observations(P, keep):
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


def _groups(P, bounds):
    """The planner's landmark groups (plan.cpp WindowPlan::groups: consecutive whole landmarks, at
    most bounds = (visits, landmarks) and 2,048 landmark-pair products) of a window without variable
    extrinsics, as (visits, landmarks, segments) per group; a segment is a free pose with a visit in
    the group."""
    max_visits, max_lms = bounds
    pose_free = P.pose_constant == 0
    per_lm = {}
    for l, p in sorted(set(zip(P.obs_landmark.tolist(), P.obs_pose.tolist()))):
        per_lm.setdefault(l, []).append(p)
    # (the planner's landmark order: by first observing pose, then the caller's)
    order = sorted(range(len(P.landmarks)), key=lambda l: min(per_lm.get(l, [len(P.poses)])))
    out, cur, nv, nl, npc = [], set(), 0, 0, 0
    for l in order:
        poses = per_lm.get(l, [])
        nf = 0 if P.landmark_constant[l] else sum(1 for p in poses if pose_free[p])
        pcl = nf * (nf + 1) // 2
        if nl > 0 and (nv + len(poses) > max_visits or nl == max_lms or npc + pcl > GROUP_PRODUCTS):
            out.append((nv, nl, len(cur)))
            cur, nv, nl, npc = set(), 0, 0, 0
        cur |= {p for p in poses if pose_free[p]}
        nv += len(poses)
        nl += 1
        npc += pcl
    if nl:
        out.append((nv, nl, len(cur)))
    return out


def _wide(og):
    return _owned(og, 20, 9, 360, seed=3101, max_obs_per_landmark=40, kf_dt_s=0.02)


def _spread(og):
    return _owned(og, 50, 60, 480, seed=3102, max_obs_per_landmark=8)


def _full(og):
    """32 landmarks x 8 keyframes = 256 visits, then one landmark seen from one keyframe."""
    P = _owned(og, 20, 40, 1600, seed=3103, max_obs_per_landmark=40, kf_dt_s=0.02)
    lm, pose = P.obs_landmark, P.obs_pose
    keep = np.zeros(len(lm), bool)
    for l in range(32):
        keep |= (lm == l) & np.isin(pose, [(l + 2 * j) % 20 for j in range(8)])
    last = (lm == 32) & (pose == 19)  # (the planner orders landmarks by first observing pose: this one stays last)
    assert last.any()
    return _keep_observations(P, keep | last)


def _fixed(og):
    P = _owned(og, 10, 500, 4000, seed=3104)
    P.pose_constant[0] = 1
    P.pose_constant[3] = 1
    P.speed_bias_constant[0] = 1
    P.landmark_constant[::7] = 1
    return P.bind()


def _retry(og, seed=3105, j=5):
    """An S10 window with an extra state (index j) whose only residual is a constant host factor:
    its 15 columns of J are zero, its pivot is min_lm_diagonal * mu."""
    P = _owned(og, 10, 500, 4000, seed=seed)
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


def _plain(og):
    return _owned(og, 10, 500, 4000, seed=3106)


SHAPES = {"wide": _wide, "spread": _spread, "full": _full, "fixed": _fixed, "retry": _retry, "plain": _plain}
# the retrying window's pivot min_lm_diagonal * mu underflows to 0 below mu = 1e-5; every other
# window of a solve with these options keeps its pivots (their diagonals are far above it)
RETRY_OPTS = dict(min_lm_diagonal=1e-318)


def _opts(og, **kw):
    return og.default_options(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0,
                              parameter_tolerance=0.0, **kw)


def _rot_err(q, q0):
    x1, y1, z1, w1 = q
    x0, y0, z0, w0 = -q0[0], -q0[1], -q0[2], q0[3]
    v = np.array([w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0,
                  w1 * y0 + y1 * w0 + z1 * x0 - x1 * z0,
                  w1 * z0 + z1 * w0 + x1 * y0 - y1 * x0])
    return 2 * np.linalg.norm(v)


class _Ref:
    """A shaped window with its oracle results, computed once per module and left unchanged:
    S, rhs, cost per mu from the initial estimate, and the 3-iteration solve."""

    def __init__(self, og, oracle, P, **opt_kw):
        self.P = P
        self.snap = P.snapshot()
        self.opts = _opts(og, **opt_kw)
        self.red = {mu: oracle.linearize_reduce(P.ptr(), True, mu) for mu in (0.0, 1e-2)}
        P.restore(self.snap)
        self.summary = oracle.solve(P.ptr(), self.opts)
        self.poses, self.landmarks = P.poses.copy(), P.landmarks.copy()
        P.restore(self.snap)


@pytest.fixture(scope="module")
def refs(og, oracle):
    return {name: _Ref(og, oracle, build(og), **(RETRY_OPTS if name == "retry" else {})) for name, build in SHAPES.items()}


@pytest.fixture(scope="module")
def fillers(og):
    return [_owned(og, 10, 500, 4000, seed=3200 + k) for k in range(N_BATCH - len(SHAPES))]


def _check_reduce(ctx, ref, parity, tag, window=0):
    for mu, (S0, rhs0, cost0, rc) in ref.red.items():
        assert rc == 0
        S, rhs, cost = ctx.linearize_reduce(window, True, mu)
        assert S.shape == S0.shape
        parity(f"{tag} initial cost (rel)", abs(cost - cost0) / cost0, 1e-12)
        parity(f"{tag} reduced system S, mu={mu} (max abs / max |S|)", np.abs(S - S0).max() / np.abs(S0).max(), S_TOL)
        parity(f"{tag} reduced rhs, mu={mu} (max abs / max |rhs|)", np.abs(rhs - rhs0).max() / np.abs(rhs0).max(), S_TOL)


def _check_solve(sg, ref, parity, tag):
    so, P0, L0 = ref.summary, ref.poses, ref.landmarks
    assert sg["num_iterations"] == so["num_iterations"] == 3, (sg, so)
    assert sg["num_successful_steps"] == so["num_successful_steps"], (sg, so)
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-10 * so["initial_cost"]
    Pg, Lg = ref.P.poses, ref.P.landmarks
    parity(f"{tag} 3-iteration solve final cost (rel)", abs(sg["final_cost"] - so["final_cost"]) / so["final_cost"], 1e-7)
    parity(f"{tag} 3-iteration solve positions (m)", np.abs(Pg[:, :3] - P0[:, :3]).max(), 1e-6)
    parity(f"{tag} 3-iteration solve rotations (rad)", max(_rot_err(Pg[i, 3:], P0[i, 3:]) for i in range(len(Pg))), 1e-6)
    parity(f"{tag} 3-iteration solve landmarks (m)", np.abs(Lg[:, :3] / Lg[:, 3:] - L0[:, :3] / L0[:, 3:]).max(), 1e-3)


def _check_property(name, g, bounds, ref, sg):
    """The path the shape is there for, from the restated groups (confirmed by the statistics) and
    the solve's summary."""
    segs = max(s for _, _, s in g)
    if name == "wide":
        assert segs == 20 and segs * 18 > 256 and len(g) == (1 if bounds == BIG else 3), g
    elif name == "spread" and bounds == BIG:
        assert len(g) == 1 and segs * 6 > 256 and segs * 9 > 192, g  # every segment pass takes a second round
    elif name == "full":
        want = [(256, 32), (1, 1)] if bounds == BIG else [(64, 8)] * 4 + [(1, 1)]
        assert [(v, l) for v, l, _ in g] == want, g
    elif name == "fixed":
        P = ref.P
        assert ((P.pose_constant[P.obs_pose] != 0) & (P.landmark_constant[P.obs_landmark] != 0)).sum() > 0
        assert np.array_equal(P.poses[0], ref.snap["poses"][0]) and np.array_equal(P.poses[3], ref.snap["poses"][3])
    elif name == "retry":
        # mu only rises by a retry: 1e-8 -> 1e-5 in the first iteration, / 5 after each accepted step
        assert sg["final_mu"] == ref.summary["final_mu"] > 10 * MU_FLOOR, (sg, ref.summary)
    else:
        assert sg["final_mu"] == MU_FLOOR


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shape_alone(og, gpu_ctx, refs, parity, name):
    """One window: small groups, the linearisation and the GN prep inside k_lin_few."""
    ref = refs[name]
    P = ref.P
    try:
        gpu_ctx.set_problems([P.struct])
        g = _groups(P, SMALL)
        st = gpu_ctx.stats()
        assert st["n_windows"] == 1 and st["n_visits"] == sum(v for v, _, _ in g), (st, g)
        assert st["n_visit_segments"] == sum(s for _, _, s in g), (st, g)
        if name == "fixed":
            assert st["n_landmarks_free"] == int((P.landmark_constant == 0).sum()) < st["n_landmarks"]
        _check_reduce(gpu_ctx, ref, parity, f"{name} alone")
        P.restore(ref.snap)
        gpu_ctx.update_params()
        sg = gpu_ctx.solve(ref.opts, 1)[0]
        _check_solve(sg, ref, parity, f"{name} alone")
        _check_property(name, g, SMALL, ref, sg)
    finally:
        P.restore(ref.snap)


@pytest.fixture(scope="module")
def batch(og, gpu_ctx, refs, fillers):
    """The shaped windows (in SHAPES order) in front of the S10 fillers: 66 windows, large groups."""
    names = sorted(SHAPES)
    ws = [refs[n].P for n in names] + fillers
    snaps = [w.snapshot() for w in ws]

    def reset():
        for w, s in zip(ws, snaps):
            w.restore(s)
    return names, ws, reset


def test_shapes_in_batch(og, gpu_ctx, refs, batch, parity):
    """66 windows: groups of up to 256 visits, k_lm_visit<0|1>; the default options, so every shaped
    window but the retrying one has its oracle solve."""
    names, ws, reset = batch
    try:
        gpu_ctx.set_problems([w.struct for w in ws])
        gs = [_groups(w, BIG) for w in ws]
        st = gpu_ctx.stats()
        assert st["n_windows"] == N_BATCH > 64
        assert st["n_visits"] == sum(v for g in gs for v, _, _ in g)
        assert st["n_visit_segments"] == sum(s for g in gs for _, _, s in g)
        for k, n in enumerate(names):
            _check_reduce(gpu_ctx, refs[n], parity, f"{n} in a batch of {N_BATCH}", window=k)
        reset()
        gpu_ctx.update_params()
        sg = gpu_ctx.solve(_opts(og), N_BATCH)
        for k, n in enumerate(names):
            if n != "retry":
                _check_solve(sg[k], refs[n], parity, f"{n} in a batch of {N_BATCH}")
                _check_property(n, gs[k], BIG, refs[n], sg[k])
        # the plain window alone against in the batch: the cross-regime bounds of
        # test_gpu_parity.test_window_alone_vs_large_batch
        k, P = names.index("plain"), refs["plain"].P
        Pb, sb = P.poses.copy(), sg[k]
        P.restore(refs["plain"].snap)
        gpu_ctx.set_problems([P.struct])
        s1 = gpu_ctx.solve(_opts(og), 1)[0]
        for f in ("num_iterations", "termination_type", "num_successful_steps"):
            assert s1[f] == sb[f], f
        parity(f"S10 alone vs in a batch of {N_BATCH}: cost (rel)", abs(s1["final_cost"] - sb["final_cost"]) / sb["final_cost"], 1e-9)
        parity(f"S10 alone vs in a batch of {N_BATCH}: positions (m)", float(np.abs(P.poses[:, :3] - Pb[:, :3]).max()), 1e-8)
    finally:
        reset()


def test_mu_retry_in_batch(og, gpu_ctx, refs, batch, parity):
    """66 windows, one of which retries mu: its GN prep is k_lm_prep_windows (mode 2 after
    k_lm_visit<1> on the same buffers); the windows beside it take no retry."""
    names, ws, reset = batch
    try:
        gpu_ctx.set_problems([w.struct for w in ws])
        assert gpu_ctx.stats()["n_windows"] == N_BATCH > 64
        sg = gpu_ctx.solve(_opts(og, **RETRY_OPTS), N_BATCH)
        k = names.index("retry")
        _check_solve(sg[k], refs["retry"], parity, f"retry in a batch of {N_BATCH}")
        assert sg[k]["final_mu"] == refs["retry"].summary["final_mu"] > 10 * MU_FLOOR, sg[k]
        assert all(s["final_mu"] == MU_FLOOR and s["num_iterations"] == 3 for i, s in enumerate(sg) if i != k)
    finally:
        reset()
