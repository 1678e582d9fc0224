"""The linear-solve checker of tests/_linsolve.py, on the CPU: LAPACK's own solution of the oracle's
reduced system passes the bound that tests/test_gn_step.py holds the device to, and three subtly
wrong solves (the mistakes a tile Cholesky can make without a whole trust-region solve noticing)
miss it by at least a factor 100; the same for the landmarks' back substitution, against the dense
numpy restatement of tests/test_oracle_solver.py."""
import numpy as np
import pytest

import _linsolve as ls
from test_oracle_solver import full_system, reduce_numpy

WINDOWS = {"kf6": (6, 150, 1000), "S10": (10, 500, 4000)}
MUS = (0.0, 1e-2)
CAUGHT = 100.0  # a mutation must miss the bound by at least this factor


@pytest.fixture(scope="module")
def systems(og, oracle):
    """(S, rhs, y of np.linalg.solve) per window and mu, computed once and left unchanged."""
    out = {}
    for name, shape in WINDOWS.items():
        w = og.SynthWindow(*shape, seed=20251015)
        for mu in MUS:
            S, rhs, _, rc = oracle.linearize_reduce(w.problem_ptr(), True, mu)
            assert rc == 0
            S = np.tril(S) + np.tril(S, -1).T
            out[name, mu] = (S, rhs, np.linalg.solve(S, rhs))
            w.reset()
    return out


def _block_of_largest(y):
    b = int(np.abs(y).argmax()) // 64
    return slice(64 * b, min(64 * b + 64, len(y)))


@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_lapack_passes_and_mutations_are_caught(systems, name, mu):
    S, rhs, y = systems[name, mu]
    n = len(rhs)
    assert n > 64  # (a tile (1, 0) exists)
    eta_ref = ls.backward_error(S, rhs, y)
    bound = ls.bound(eta_ref, n)
    assert eta_ref <= bound and bound <= 16 * max(eta_ref, n * 2.0 ** -53)
    # the refined solution is a tighter solution still, and LAPACK's forward error is what cond(S) allows
    y_star = ls.refined_solve(S, rhs)
    assert ls.backward_error(S, rhs, y_star) <= eta_ref
    print(f"{name} mu={mu}: n {n}, eta_ref {eta_ref:.2e}, bound {bound:.2e}, forward error of LAPACK "
          f"{ls.forward_error(y, y_star):.2e}, cond {np.linalg.cond(S):.1e}")

    # (a) one 64-row block of y scaled by 1 + 1e-9 (the block holding the largest entry)
    ya = y.copy()
    ya[_block_of_largest(y)] *= 1.0 + 1e-9
    # (b) the solution of a system whose tile (1, 0) differs by 1e-9 relative
    Sb = S.copy()
    Sb[64:128, 0:64] *= 1.0 + 1e-9
    Sb[0:64, 64:128] = Sb[64:128, 0:64].T
    yb = np.linalg.solve(Sb, rhs)
    # (c) rhs rows 60..63 shifted by one row (the tail rows of the last 16-block of a tile)
    rc_ = rhs.copy()
    rc_[60:64] = rhs[61:65]
    yc = np.linalg.solve(S, rc_)
    for tag, ym in (("a: block of y scaled", ya), ("b: tile (1, 0) perturbed", yb), ("c: rhs rows shifted", yc)):
        factor = ls.backward_error(S, rhs, ym) / bound
        print(f"  mutation {tag}: eta / bound = {factor:.3g}")
        assert factor >= CAUGHT, f"{name} mu={mu}, mutation {tag}: eta is only {factor:.3g} x the bound"


@pytest.mark.parametrize("mu", MUS)
def test_landmark_residual(og, oracle, mu):
    """The dense numpy full step (J^T J of the whole window, Schur complement, per-landmark solves)
    satisfies the per-observation restatement within the bound; one component of y_l off by 1e-9
    relative does not."""
    w = og.SynthWindow(*WINDOWS["kf6"], seed=20251015)
    p = w.problem
    r, Jp, Jl = oracle.eval_reprojection(w.problem_ptr(), p.n_observations)
    _, Ji = oracle.eval_imu(w.problem_ptr(), p.n_imu)
    w.reset()
    J, res, nf = full_system(w, oracle)
    w.reset()
    # the restated Jacobi rule against the columns of the full Jacobian
    s_full = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))
    sp, sl = ls.jacobi_scales(p, r, Jp, Jl, J_imu=Ji)
    assert np.abs(sp / s_full[:nf].reshape(-1, 15)[:, :6] - 1).max() <= 1e-14
    assert np.abs(sl / s_full[nf:].reshape(-1, 3) - 1).max() <= 1e-14
    # the full step, dense: y_f from the reduced system, y_l = V'^-1 (g_l' - W'^T y_f)
    S, rhs = reduce_numpy(J, res, nf, True, mu)
    y_f = ls.refined_solve(S, rhs).astype(np.float64)
    Js = J * s_full
    H, g = Js.T @ Js, Js.T @ res
    if mu > 0:
        H = H + np.diag(np.clip((Js * Js).sum(0), 1e-6, 1e32) * mu)
    y_l = np.zeros((p.n_landmarks, 3))
    for l in range(p.n_landmarks):
        sl3 = slice(nf + 3 * l, nf + 3 * l + 3)
        y_l[l] = np.linalg.solve(H[sl3, sl3], g[sl3] - H[sl3, :nf] @ y_f)
    eta_ref = ls.landmark_eta(*ls.landmark_residual(p, r, Jp, Jl, (sp, sl), mu, y_f,
                                                    ls.landmark_backsub(p, r, Jp, Jl, (sp, sl), mu, y_f)))
    bound = ls.bound(eta_ref, 3)
    eta = ls.landmark_eta(*ls.landmark_residual(p, r, Jp, Jl, (sp, sl), mu, y_f, y_l))
    print(f"mu={mu}: eta_l {eta:.2e}, eta_l of the float64 back substitution {eta_ref:.2e}, bound {bound:.2e}")
    assert eta <= bound
    bad = y_l.copy()
    l, a = np.unravel_index(np.abs(y_l).argmax(), y_l.shape)
    bad[l, a] *= 1.0 + 1e-9
    factor = ls.landmark_eta(*ls.landmark_residual(p, r, Jp, Jl, (sp, sl), mu, y_f, bad)) / bound
    print(f"  one component of y_l off by 1e-9 relative: eta_l / bound = {factor:.3g}")
    assert factor >= CAUGHT, f"eta_l is only {factor:.3g} x the bound"


def test_constant_blocks_are_honoured(og, oracle):
    """pose_offsets follows the reduced ordering; a constant landmark has no residual."""
    from _problem import OwnedProblem
    P = OwnedProblem.copy_of(og.SynthWindow(*WINDOWS["kf6"], seed=20251015).problem)
    P.pose_constant[1] = 1
    P.speed_bias_constant[0] = 1
    P.landmark_constant[::5] = 1
    P.bind()
    assert ls.pose_offsets(P.struct).tolist() == [0, -1, 6 + 9, 6 + 9 + 15, 6 + 9 + 30, 6 + 9 + 45]
    S, rhs, _, rc = oracle.linearize_reduce(P.ptr(), True, 0.0)
    assert rc == 0 and len(rhs) == 6 * 15 - 6 - 9
    r, Jp, Jl = oracle.eval_reprojection(P.ptr(), P.struct.n_observations)
    res, den = ls.landmark_residual(P.struct, r, Jp, Jl, ls.jacobi_scales(P.struct, r, Jp, Jl, scaling=False), 0.0,
                                    np.zeros(len(rhs)), np.zeros((len(P.landmarks), 3)))
    assert len(res) == int((P.landmark_constant == 0).sum()) < len(P.landmarks)
