"""The Gauss-Newton linear solve as what it is, a linear solver: the tile-sparse FP64 Cholesky
(chol_tiles.hpp, kernels_chol.hip, kernels_chol_pipe.hip) with its back substitution (backSubstitute /
k_chol_bsub) and the landmarks' back substitution (k_lm_backsub_jv), through
okvisgpu_gauss_newton_step, against the device's own S and rhs (okvisgpu_linearize_reduce), so the
check isolates the solver from the Schur kernels:

  eta   = |rhs - S y_f|_inf / (|S|_inf |y_f|_inf + |rhs|_inf)            (tests/_linsolve.py, longdouble)
  eta_l = max_l |s g_l - s sum J_l^T J_p s_p y_p - V' y_l|_inf / (...)   (plain windows)

each held to 16 max(eta_ref, n u): eta_ref is the backward error of np.linalg.solve on the same
system (of a float64 numpy back substitution for eta_l, n = 3), u = 2^-53. No bound comes from the
device's output. The forward error against a refined solve is recorded, never asserted (it scales
with cond(S)). Every case first asserts, from the host-only plan or the context's statistics, the
tile-shape property it is there for.

Windows are SynthWindow(kf, 40 kf, 300 kf) unless stated: the smallest at which the tile code can
still go wrong."""
import sys

import numpy as np
import pytest

import _linsolve as ls
from _problem import OwnedProblem

pytestmark = pytest.mark.gpu

SEED = 20251015
NOT_ASSERTED = sys.float_info.max  # bound of a row that is recorded only
ERR_INVALID_ARGUMENT, ERR_NUMERICAL = 1, 6  # include/okvisgpu.h okvisgpu_status
# Smallest keyframe count whose SynthWindow(kf, 40 kf, 300 kf, seed=SEED) has a nested-dissection
# plan with a split and gap rows (og.plan_window(p, 1): split_tL, split_tS and gap_rows all > 0),
# found on the CPU by trying kf = 4, 5, ...: 29 keyframes and fewer keep the natural order.
KF_SPLIT = 30


def _owned(og, kf, lm=None, obs=None, seed=SEED, **cfg):
    return OwnedProblem.copy_of(og.SynthWindow(kf, lm or 40 * kf, obs or 300 * kf, seed=seed, **cfg).problem)


def _tracking(og):
    """The tracking solve: only the newest state free."""
    P = _owned(og, 4)
    P.pose_constant[:-1] = 1
    P.speed_bias_constant[:-1] = 1
    return P.bind()


def _nq(rows):
    """chol_tiles.hpp tileBlocks: 16-column blocks of a diagonal tile before its identity tail."""
    return max(1, -(-rows // 16))


class _System:
    """One window's device S and rhs at (scaling, mu) with everything numpy derives from them,
    computed once per module and left unchanged."""

    def __init__(self, ctx, P, window, scaling, mu, landmarks):
        p = P.struct
        self.S, self.rhs, _ = ctx.linearize_reduce(window, scaling, mu)
        self.n = len(self.rhs)
        self.y_ref = np.linalg.solve(self.S, self.rhs)
        self.eta_ref = ls.backward_error(self.S, self.rhs, self.y_ref)
        self.y_star = ls.refined_solve(self.S, self.rhs)
        self.lm = None
        if landmarks:
            r, Jp, Jl = ctx.eval_reprojection(p.n_observations, window)
            Ji = ctx.eval_imu(p.n_imu, window)[1] if scaling else None
            scale = ls.jacobi_scales(p, r, Jp, Jl, J_imu=Ji, scaling=scaling)
            self.lm = (p, r, Jp, Jl, scale, mu)
            y_l = ls.landmark_backsub(*self.lm, self.y_ref)
            self.eta_l_ref = ls.landmark_eta(*ls.landmark_residual(*self.lm, self.y_ref, y_l))


@pytest.fixture(scope="module")
def systems():
    return {}


def _check(og, ctx, parity, systems, P, tag, sched, mu=0.0, scaling=True, window=0, landmarks=True, **opt_kw):
    """eta (and eta_l) of one gauss_newton_step against the bound; returns (y_f, system)."""
    k = (tag, window, scaling, mu)
    if k not in systems:
        systems[k] = _System(ctx, P, window, scaling, mu, landmarks)
    s = systems[k]
    opts = og.default_options(jacobi_scaling=int(scaling), cholesky_schedule=sched, **opt_kw)
    y_f, y_l = ctx.gauss_newton_step(window, opts, mu)
    assert y_f.shape == (s.n,) and y_l.shape == (P.struct.n_landmarks, 3)
    row = f"gn {tag} dim={s.n} schedule={sched} mu={mu:g} scaling={int(scaling)}"
    parity(f"{row}: eta of LAPACK", s.eta_ref, ls.bound(s.eta_ref, s.n))
    parity(f"{row}: forward error vs refined solve (recorded)", ls.forward_error(y_f, s.y_star), NOT_ASSERTED)
    eta = ls.backward_error(s.S, s.rhs, y_f)
    eta_l = bound_l = None
    if s.lm is not None:
        assert not y_l[P.landmark_constant != 0].any()
        eta_l, bound_l = ls.landmark_eta(*ls.landmark_residual(*s.lm, y_f, y_l)), ls.bound(s.eta_l_ref, 3)
        print(f"parity {row}: eta_l {eta_l:.3e}, of the numpy back substitution {s.eta_l_ref:.3e}")
    # both figures are printed before either is asserted
    print(f"parity {row}: eta {eta:.3e}, of LAPACK {s.eta_ref:.3e}")
    failures = []
    for name, got, bnd in ((f"{row}: eta", eta, ls.bound(s.eta_ref, s.n)), (f"{row}: eta_l", eta_l, bound_l)):
        if got is not None:
            try:
                parity(name, got, bnd)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "; ".join(failures)
    return y_f, s


# ---- the identity tail of the last diagonal tile (tileBlocks, potrfTile's nq) ---------------------
#        name: (builder, reduced dim, tiles, rows in the last tile)
TAILS = {
    "tracking": (_tracking, 15, 1, 15),
    "kf4": (lambda og: _owned(og, 4), 60, 1, 60),     # nq = 4, 4 identity rows inside the last 16-block
    "kf5": (lambda og: _owned(og, 5), 75, 2, 11),     # nq = 1
    "kf6": (lambda og: _owned(og, 6), 90, 2, 26),     # nq = 2
    "kf7": (lambda og: _owned(og, 7), 105, 2, 41),    # nq = 3
    "kf8": (lambda og: _owned(og, 8), 120, 2, 56),    # nq = 4, 8 identity rows
    "kf13": (lambda og: _owned(og, 13), 195, 4, 3),   # T = 4, 3 rows in the last tile
    # 15 * 12 + 6 * 2 = 192 = 3 * 64: no padding row at all
    "kf12+extrinsics": (lambda og: _owned(og, 12, do_extrinsics=1), 192, 3, 64),
}
TAIL_NQ = {"tracking": 1, "kf4": 4, "kf5": 1, "kf6": 2, "kf7": 3, "kf8": 4, "kf13": 1, "kf12+extrinsics": 4}


@pytest.fixture(scope="module")
def tails(og):
    return {name: build(og) for name, (build, _, _, _) in TAILS.items()}


@pytest.mark.parametrize("sched", [0, 1, 2, 4])
@pytest.mark.parametrize("name", list(TAILS))
def test_identity_tail(og, gpu_ctx, parity, systems, tails, name, sched):
    P = tails[name]
    _, dim, T, rows = TAILS[name]
    plan = og.plan_window(P.struct, 1)  # (a window alone is planned with the nested-dissection chooser)
    assert (plan["reduced_dim"], plan["tiles"], plan["s_dim"]) == (dim, T, 64 * T), plan
    assert plan["gap_rows"] == 0 and dim - 64 * (T - 1) == rows and _nq(rows) == TAIL_NQ[name]
    if name == "tracking":
        assert P.pose_constant[:-1].all() and not P.pose_constant[-1] and not P.speed_bias_constant[-1]
    if name == "kf12+extrinsics":
        assert plan["reduced_dim"] == plan["s_dim"] and not P.extrinsics_constant.any()
    gpu_ctx.set_problems([P.struct])
    st = gpu_ctx.stats()
    assert st["n_windows"] == 1 and st["reduced_dim"] == dim
    assert st["n_extrinsics_free"] == (2 if name == "kf12+extrinsics" else 0)
    _check(og, gpu_ctx, parity, systems, P, name, sched, landmarks=name != "kf12+extrinsics")


# ---- mu and scaling --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kf10(og):
    return _owned(og, 10)


@pytest.mark.parametrize("sched", [1, 2, 4])
@pytest.mark.parametrize("scaling,mu", [(True, 0.0), (True, 1e-8), (True, 1e-2), (False, 0.0)])
def test_mu_and_scaling(og, gpu_ctx, parity, systems, kf10, scaling, mu, sched):
    """scaling = 0 is the badly scaled system, where the explicit tile inverses are least forgiving."""
    plan = og.plan_window(kf10.struct, 1)
    assert (plan["reduced_dim"], plan["tiles"]) == (150, 3)
    gpu_ctx.set_problems([kf10.struct])
    _, s = _check(og, gpu_ctx, parity, systems, kf10, "kf10", sched, mu=mu, scaling=scaling)
    if not scaling:  # (what makes it the hard case)
        d = np.diag(s.S)
        assert d.max() / d.min() > 1e4


# ---- fill outside the band --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop(og):
    return _owned(og, 30, n_relpose=5, relpose_stride=25, relpose_kind=1)


def _structural_tiles(P):
    """Lower tiles (diagonal included) of the natural order that hold an entry of S before any
    elimination fill. Blocks: pose i = rows 15 i .. 15 i + 5, speed/bias i = rows 15 i + 6 .. 15 i + 14
    (every state free). Coupled: every block with itself, the four blocks of an IMU factor with each
    other, the two poses of a pose-graph edge, and two poses that share a landmark."""
    n = len(P.poses)
    pose = lambda i: (15 * int(i), 15 * int(i) + 5)
    sb = lambda i: (15 * int(i) + 6, 15 * int(i) + 14)
    pairs = {(pose(i), pose(i)) for i in range(n)} | {(sb(i), sb(i)) for i in range(n)}
    for pa, sa, pb, sbb in P.imu_blocks:
        four = [pose(pa), sb(sa), pose(pb), sb(sbb)]
        pairs |= {(x, y) for x in four for y in four}
    pairs |= {(pose(a), pose(b)) for a, b in P.relpose_blocks}
    seen = np.zeros((len(P.landmarks), n), np.int64)
    seen[P.obs_landmark, P.obs_pose] = 1
    pairs |= {(pose(i), pose(j)) for i, j in zip(*np.nonzero(seen.T @ seen))}
    tiles = set()
    for (a0, a1), (b0, b1) in pairs:
        for a in {a0 // 64, a1 // 64}:
            for b in {b0 // 64, b1 // 64}:
                tiles.add((max(a, b), min(a, b)))
    return tiles


@pytest.mark.parametrize("sched", [1, 2, 4])
def test_fill_outside_the_band(og, gpu_ctx, parity, systems, loop, sched):
    """Loop-closure edges from keyframes 0..4 to 25..29: non-zero tiles far below the diagonal, and
    tiles that only the elimination fills."""
    plan = og.plan_window(loop.struct, 1)
    nz, T = plan["tile_nz"], plan["tiles"]
    assert plan["split_tS"] == 0 and np.array_equal(plan["natural"][:450], np.arange(450))  # (natural order)
    assert max(i - j for i in range(T) for j in range(T) if nz[i, j]) > 2
    structural = _structural_tiles(loop)
    assert all(nz[i, j] for i, j in structural) and plan["nonzero_tiles"] > len(structural)
    gpu_ctx.set_problems([loop.struct])
    assert gpu_ctx.stats()["n_relpose"] == 5
    _check(og, gpu_ctx, parity, systems, loop, "kf30+loop", sched, landmarks=False)


# ---- nested-dissection order with a split and gap rows ----------------------------------------------
@pytest.fixture(scope="module")
def split(og):
    return {"kf%d" % KF_SPLIT: _owned(og, KF_SPLIT), "S50": _owned(og, 50, 2000, 16000)}


@pytest.fixture(scope="module")
def fillers(og):
    """(3, 40, 200) windows: what fills a batch beyond 64 windows and beyond one window per CU."""
    return [_owned(og, 3, 40, 200, seed=4000 + k) for k in range(260)]


@pytest.mark.parametrize("sched", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["kf%d" % KF_SPLIT, "S50"])
def test_split_order(og, gpu_ctx, parity, systems, split, name, sched):
    """Alone, the batch is below one window per CU: the window is held in its nested-dissection
    order (two independent parts, gap rows that end the left part on a tile boundary, the separator
    last); the natural-order export undoes it."""
    P = split[name]
    plan = og.plan_window(P.struct, 1)
    assert plan["split_tL"] > 0 and plan["split_tS"] > 0 and plan["gap_rows"] > 0, plan
    if name != "S50":
        smaller = _owned(og, KF_SPLIT - 1)
        small = og.plan_window(smaller.struct, 1)
        assert small["split_tS"] == 0 and small["gap_rows"] == 0
    else:
        assert (plan["reduced_dim"], plan["tiles"]) == (750, 12)
    gpu_ctx.set_problems([P.struct])
    assert gpu_ctx.stats()["cholesky_split_windows"] == 1
    _check(og, gpu_ctx, parity, systems, P, name + " split order", sched)


def test_split_order_agrees_with_natural_order(og, gpu_ctx, parity, systems, split, fillers):
    """The same window in a batch of more than one window per CU keeps the natural order; y_f of
    the two orders is compared in the natural order (recorded, not asserted: two factorisation
    orders differ by what cond(S) allows)."""
    P = split["kf%d" % KF_SPLIT]
    gpu_ctx.set_problems([P.struct])
    y_split, _ = gpu_ctx.gauss_newton_step(0, None, 0.0)
    batch = [P] + fillers
    gpu_ctx.set_problems([w.struct for w in batch])
    st = gpu_ctx.stats()
    assert st["n_windows"] == len(batch) > 256 and st["cholesky_split_windows"] == 0
    y_nat, _ = _check(og, gpu_ctx, parity, systems, P, f"kf{KF_SPLIT} natural order in a batch of {len(batch)}", 0)
    parity(f"gn kf{KF_SPLIT}: y_f of the split order vs of the natural order (recorded)",
           ls.forward_error(y_split, y_nat), NOT_ASSERTED)


# ---- ragged batches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", [0, 1, 4])
def test_ragged_batch(og, gpu_ctx, parity, systems, tails, split, sched):
    """kf = 13, 4 and 50 in one batch: a window's padded dimension differs from the batch's largest
    (the dynamic LDS and the tile loops are sized by the largest)."""
    ws = [tails["kf13"], tails["kf4"], split["S50"]]
    dims = [og.plan_window(w.struct, 1)["s_dim"] for w in ws]
    assert dims == [256, 64, 768]
    gpu_ctx.set_problems([w.struct for w in ws])
    st = gpu_ctx.stats()
    assert st["n_windows"] == 3 and st["reduced_dim"] == 195 + 60 + 750
    for k, (w, name) in enumerate(zip(ws, ("kf13", "kf4", "S50"))):
        _check(og, gpu_ctx, parity, systems, w, f"{name} in a batch of 3", sched, window=k)


@pytest.mark.parametrize("sched", [0, 1])
def test_many_windows(og, gpu_ctx, parity, systems, tails, fillers, sched):
    """66 windows (large landmark groups, k_lm_visit<1> and k_lm_prep_windows, the many-window
    layouts): the first two and the last window."""
    ws = [tails["kf5"], tails["kf13"]] + fillers[:64]
    gpu_ctx.set_problems([w.struct for w in ws])
    st = gpu_ctx.stats()
    assert st["n_windows"] == 66 > 64
    for k, name in ((0, "kf5"), (1, "kf13"), (65, "kf3 filler")):
        _check(og, gpu_ctx, parity, systems, ws[k], f"{name} in a batch of 66", sched, window=k)


# ---- numerical failure is reported, not returned as numbers ------------------------------------------------
@pytest.mark.parametrize("sched", [1, 2, 4])
def test_numerical_failure_is_reported(og, gpu_ctx, parity, systems, sched):
    """The retrying window of tests/test_lm_visit_paths.py: a state whose columns of J are zero has
    the pivot min_lm_diagonal * mu, which underflows to 0 at mu = 1e-8 and is a denormal at 1e-5.
    (Its rows of S and rhs are zero but for that diagonal entry, so the system linearize_reduce
    exports with the default min_lm_diagonal has the same solution: zero in those rows.)"""
    from test_lm_visit_paths import RETRY_OPTS, _retry
    P = _retry(og)
    assert RETRY_OPTS["min_lm_diagonal"] * 1e-8 == 0.0 < RETRY_OPTS["min_lm_diagonal"] * 1e-5
    gpu_ctx.set_problems([P.struct])
    opts = og.default_options(cholesky_schedule=sched, **RETRY_OPTS)
    with pytest.raises(og.OkvisGpuError, match=rf"\({ERR_NUMERICAL}\)"):
        gpu_ctx.gauss_newton_step(0, opts, 1e-8)
    y_f, s = _check(og, gpu_ctx, parity, systems, P, "retry", sched, mu=1e-5, landmarks=False, **RETRY_OPTS)
    assert s.n == 165 and not y_f[15 * 5:15 * 6].any()


def test_refused_inside_a_solve(og, gpu_ctx, kf10):
    gpu_ctx.set_problems([kf10.struct])
    snap = kf10.snapshot()
    try:
        gpu_ctx.solve_begin(og.default_options(max_num_iterations=1))
        with pytest.raises(og.OkvisGpuError, match=rf"\({ERR_INVALID_ARGUMENT}\)"):
            gpu_ctx.gauss_newton_step(0, None, 0.0)
        gpu_ctx.solve_end(1)
    finally:
        kf10.restore(snap)
