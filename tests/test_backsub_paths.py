"""The landmark back substitution (kernels_backsub.hip k_lm_backsub_jv) on small windows shaped to
reach each of its paths. A workgroup copies the A planes and flags of its group's observations to
LDS (the stage, 512 observations) and reads them there in both visit phases; a group with more
observations reads global memory. Each shaped window is checked twice:

  * okvisgpu_gauss_newton_step's y_f / y_l against tests/_linsolve.py, exactly as
    tests/test_gn_step.py does (its _check: eta and eta_l under 16 max(eta_ref, n u), eta_ref from
    numpy on the same system, landmark_backsub for eta_l);
  * a 3-iteration solve against the oracle under the bounds of
    test_gpu_parity.test_solve_parity_s10 (test_lm_visit_paths._check_solve): iterations and
    successful steps exact (the J*v forms of this kernel decide the model cost, hence acceptance
    and radius), and the termination.

Every shaped window runs alone and in a batch of 66. Alone is the few-window regime (plan.hpp
fewWindows): groups of at most 64 visits / 16 landmarks, and the kernel reads global memory in both
phases (the stage's barrier shows in a kernel of microseconds). In the batch the groups hold up to
256 visits / 64 landmarks and take the stage unless they exceed it. Each test first asserts, from the grouping restated in tests/_backsub.py (confirmed by
the context's statistics), that its window has the property it is there for:
  * full          in the batch a group of exactly 256 visits with two observations each - 512, the
                  stage filled exactly - followed by a group of one visit with one observation;
  * mono          one observation per visit, and a group whose range starts at an odd observation
                  (the copy moves 4-byte words: no 16-byte alignment to rely on);
  * fixed         two constant poses (visits without a free pose), every seventh landmark constant
                  (landmarks without a step) and observations masked by flags & 2;
  * three_cameras the full window with a third camera: 768 observations in the group of 256
                  visits, which therefore reads global memory in the batch too, beside staged
                  groups of the same launch;
  * plain         an S10 window, also compared alone against in the batch;
  * retry         a window of the batch whose Gauss-Newton step fails (gn_failed): its workgroups
                  leave early, and the windows beside it must not notice;
and y_l is stored on demand only: after a solve (which does not store it), gauss_newton_step on
the same context still returns a y_l that passes the bound.
"""
import numpy as np
import pytest

import _backsub as bs
from test_gn_step import _check as gn_check
from test_lm_visit_paths import BIG, MU_FLOOR, N_BATCH, RETRY_OPTS, SMALL, _check_solve, _opts, _owned

pytestmark = pytest.mark.gpu

# (batch order: the mono window first, so that its observations start at 0 in the batch as well)
SHAPES = {"mono": bs.mono, "full": bs.full, "fixed": bs.fixed, "three_cameras": bs.three_cameras, "plain": bs.plain}
# gauss_newton_step is checked at this mu: a landmark with a single observation (the mono window
# has some) has a singular block at mu = 0
GN_MU = 1e-2
TERMINATION = ("num_iterations", "termination_type", "num_successful_steps")


class _Ref:
    """A shaped window with its oracle 3-iteration solve, computed once per module and left unchanged."""

    def __init__(self, og, oracle, P):
        self.P = P
        self.snap = P.snapshot()
        self.opts = _opts(og)
        self.summary = oracle.solve(P.ptr(), self.opts)
        self.poses, self.landmarks = P.poses.copy(), P.landmarks.copy()
        P.restore(self.snap)


@pytest.fixture(scope="module")
def refs(og, oracle):
    return {name: _Ref(og, oracle, build()) for name, build in SHAPES.items()}


@pytest.fixture(scope="module")
def retrying(og):
    return bs.retry()


@pytest.fixture(scope="module")
def fillers(og):
    return [_owned(og, 10, 500, 4000, seed=3400 + k) for k in range(N_BATCH - len(SHAPES) - 1)]


@pytest.fixture(scope="module")
def systems():
    return {}


def _check_property(name, P, g):
    """The path the shape is there for, from the restated groups g = (first observation,
    observations, visits, landmarks); big: the batch's group bounds."""
    visits = set(zip(P.obs_landmark.tolist(), P.obs_pose.tolist()))
    per_visit = len(P.obs_pose) / len(visits)
    if name == "full":
        want = [(0, 512, 256, 32), (512, 1, 1, 1)] if len(g) == 2 else [(128 * k, 128, 64, 8) for k in range(4)] + [(512, 1, 1, 1)]
        assert g == want and want[0][1] <= bs.STAGE_OBS, g
        assert P.landmark_constant[32] and not P.landmark_constant[:32].any()
    elif name == "mono":
        assert per_visit == 1.0 and all(no == nv for _, no, nv, _ in g)
        assert any(first % 2 == 1 for first, _, _, _ in g), g
        assert max(no for _, no, _, _ in g) <= bs.STAGE_OBS
    elif name == "fixed":
        masked = (P.pose_constant[P.obs_pose] != 0) & (P.landmark_constant[P.obs_landmark] != 0)
        assert masked.sum() > 0 and (P.pose_constant != 0).sum() == 2 and P.landmark_constant[::7].all()
    elif name == "three_cameras":
        assert per_visit > 2 and len(P.cameras) == 3
        if len(g) == 2:
            assert g[0] == (0, 768, 256, 32) and g[0][1] > bs.STAGE_OBS, g
        else:
            assert max(no for _, no, _, _ in g) == 192, g
    else:
        assert max(no for _, no, _, _ in g) <= bs.STAGE_OBS


@pytest.mark.parametrize("name", list(SHAPES))
def test_shape_alone(og, gpu_ctx, refs, systems, parity, name):
    ref = refs[name]
    P = ref.P
    try:
        gpu_ctx.set_problems([P.struct])
        g = bs.obs_groups(P, SMALL)
        st = gpu_ctx.stats()
        assert st["n_windows"] == 1 and st["n_visits"] == sum(v for _, _, v, _ in g), (st, g)
        assert st["n_observations"] == sum(no for _, no, _, _ in g)
        _check_property(name, P, g)
        gn_check(og, gpu_ctx, parity, systems, P, f"backsub {name} alone", 0, mu=GN_MU)
        sg = gpu_ctx.solve(ref.opts, 1)[0]
        _check_solve(sg, ref, parity, f"backsub {name} alone")
        assert sg["termination_type"] == ref.summary["termination_type"]
    finally:
        P.restore(ref.snap)


@pytest.fixture(scope="module")
def batch(refs, retrying, fillers):
    """The shaped windows (in SHAPES order), the retrying window, then the S10 fillers: 66 windows."""
    names = list(SHAPES) + ["retry"]
    ws = [refs[n].P for n in SHAPES] + [retrying] + fillers
    snaps = [w.snapshot() for w in ws]

    def reset():
        for w, s in zip(ws, snaps):
            w.restore(s)
    return names, ws, reset


def test_shapes_in_batch(og, gpu_ctx, refs, batch, systems, parity):
    names, ws, reset = batch
    try:
        gpu_ctx.set_problems([w.struct for w in ws])
        gs = [bs.obs_groups(w, BIG) for w in ws]
        st = gpu_ctx.stats()
        assert st["n_windows"] == N_BATCH > 64
        assert st["n_visits"] == sum(v for g in gs for _, _, v, _ in g)
        for k, n in enumerate(SHAPES):
            _check_property(n, ws[k], gs[k])
            gn_check(og, gpu_ctx, parity, systems, ws[k], f"backsub {n} in a batch of {N_BATCH}", 0, mu=GN_MU, window=k)
        sg = gpu_ctx.solve(_opts(og), N_BATCH)
        for k, n in enumerate(SHAPES):
            _check_solve(sg[k], refs[n], parity, f"backsub {n} in a batch of {N_BATCH}")
            assert sg[k]["termination_type"] == refs[n].summary["termination_type"]
        # the plain window alone against in the batch: the cross-regime bounds of
        # test_gpu_parity.test_window_alone_vs_large_batch
        k, P = names.index("plain"), refs["plain"].P
        Pb, sb = P.poses.copy(), sg[k]
        P.restore(refs["plain"].snap)
        gpu_ctx.set_problems([P.struct])
        s1 = gpu_ctx.solve(_opts(og), 1)[0]
        for f in TERMINATION:
            assert s1[f] == sb[f], f
        parity(f"backsub S10 alone vs in a batch of {N_BATCH}: cost (rel)", abs(s1["final_cost"] - sb["final_cost"]) / sb["final_cost"], 1e-9)
        parity(f"backsub S10 alone vs in a batch of {N_BATCH}: positions (m)", float(np.abs(P.poses[:, :3] - Pb[:, :3]).max()), 1e-8)
    finally:
        reset()


def test_retrying_window_leaves_the_others_alone(og, gpu_ctx, batch):
    """One window of the batch fails its Gauss-Newton step at the first values of mu; the other
    windows match, bit for bit, the batch that does not contain it."""
    names, ws, reset = batch
    k = names.index("retry")
    others = [w for i, w in enumerate(ws) if i != k]
    fields = ("poses", "speed_biases", "landmarks")
    try:
        gpu_ctx.set_problems([w.struct for w in ws])
        assert gpu_ctx.stats()["n_windows"] == N_BATCH > 64
        sg = gpu_ctx.solve(_opts(og, **RETRY_OPTS), N_BATCH)
        # mu only rises by a retry (a failed Gauss-Newton step): 1e-8 -> 1e-5 in the first iteration
        assert sg[k]["final_mu"] > 10 * MU_FLOOR and sg[k]["num_iterations"] == 3, sg[k]
        assert all(s["final_mu"] == MU_FLOOR for i, s in enumerate(sg) if i != k)
        with_retry = [{f: getattr(w, f).copy() for f in fields} for w in others]
        s_with = [s for i, s in enumerate(sg) if i != k]
        reset()
        gpu_ctx.set_problems([w.struct for w in others])
        assert gpu_ctx.stats()["n_windows"] == N_BATCH - 1 > 64
        s_without = gpu_ctx.solve(_opts(og, **RETRY_OPTS), N_BATCH - 1)
        for i, w in enumerate(others):
            for f in fields:
                assert np.array_equal(getattr(w, f), with_retry[i][f]), (i, f)
            for f in TERMINATION + ("initial_cost", "final_cost", "final_mu", "final_radius"):
                assert s_with[i][f] == s_without[i][f], (i, f)
    finally:
        reset()


def test_y_l_is_stored_on_demand(og, gpu_ctx, systems, parity):
    """The iteration does not store y_l; okvisgpu_gauss_newton_step asks for it. A window no other
    test uses is solved first, so nothing this context computed before equals its y_l."""
    P = _owned(og, 10, 500, 4000, seed=3499)
    snap = P.snapshot()
    gpu_ctx.set_problems([P.struct])
    sg = gpu_ctx.solve(_opts(og), 1)[0]
    assert sg["num_iterations"] == 3 and sg["num_successful_steps"] > 0
    P.restore(snap)  # (the checker's Jacobi scales take the priors at their measurement: the initial state)
    gpu_ctx.update_params()
    _, s = gn_check(og, gpu_ctx, parity, systems, P, "backsub y_l after a solve", 0, mu=GN_MU)
    _, y_l = gpu_ctx.gauss_newton_step(0, None, GN_MU)
    assert np.abs(y_l).max() > 0
