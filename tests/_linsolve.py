"""A plain high-precision checker of one Gauss-Newton solve (numpy only, no solver of the project's):

  backward_error     the normwise backward error of y as a solution of S y = rhs,
  refined_solve      a forward reference y* (LAPACK + iterative refinement with longdouble residuals),
  landmark_residual  the residual of the landmarks' back substitution, per free landmark,
  jacobi_scales      the Jacobi column scales 1 / (1 + sqrt(diag(J^T J))) of the poses and landmarks,
  bound              the bound the tests assert: 16 max(eta_ref, n u).

The backward error does not depend on the condition number of S (about 1e8 for these windows), so it
can be held near unit roundoff where a forward comparison cannot. Residuals and norms are accumulated
in np.longdouble (64-bit significand on x86-64; where longdouble is double the checks still hold,
with less margin)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53  # unit roundoff of float64
MIN_LM_DIAGONAL, MAX_LM_DIAGONAL = 1e-6, 1e32  # okvisgpu_default_options (Ceres' defaults)


def bound(eta_ref, n):
    """16 max(eta_ref, n u): eta_ref is LAPACK's (numpy's) backward error on the same system, n the
    dimension; 16 allows for another summation order and for products with explicit tile inverses
    where LAPACK solves triangular systems."""
    return 16.0 * max(float(eta_ref), n * U)


def _norm_inf_matrix(A):
    return np.abs(A).sum(axis=1).max()


def backward_error(S, rhs, y):
    """eta = |rhs - S y|_inf / (|S|_inf |y|_inf + |rhs|_inf), everything accumulated in longdouble."""
    S, rhs, y = np.asarray(S, LD), np.asarray(rhs, LD), np.asarray(y, LD)
    res = rhs - S @ y
    den = _norm_inf_matrix(S) * np.abs(y).max() + np.abs(rhs).max()
    return float(np.abs(res).max() / den)


def refined_solve(S, rhs, rounds=5, tol=1e-30):
    """np.linalg.solve followed by iterative refinement with longdouble residuals (the solution is
    kept in longdouble): stops when the correction falls below tol relative, or after `rounds`."""
    S64, Sl, bl = np.asarray(S, np.float64), np.asarray(S, LD), np.asarray(rhs, LD)
    y = np.linalg.solve(S64, np.asarray(rhs, np.float64)).astype(LD)
    for _ in range(rounds):
        d = np.linalg.solve(S64, (bl - Sl @ y).astype(np.float64)).astype(LD)
        y = y + d
        if np.abs(d).max() <= tol * np.abs(y).max():
            break
    return y


def forward_error(y, y_star):
    """|y - y*|_inf / |y*|_inf (recorded by the tests, never asserted: it scales with cond(S))."""
    y, y_star = np.asarray(y, LD), np.asarray(y_star, LD)
    return float(np.abs(y - y_star).max() / np.abs(y_star).max())


# ---- the landmarks' back substitution ------------------------------------------------------------
def _arr(p, name, shape, dtype):
    ptr = getattr(p, name)
    n = int(np.prod(shape))
    if n == 0 or not ptr:
        return np.zeros(shape, dtype)
    return np.ctypeslib.as_array(ptr, shape=shape).astype(dtype)


def _structure(p):
    """(obs_pose, obs_landmark, pose_constant, sb_constant, landmark_constant) of an okvisgpu_problem."""
    nO = p.n_observations
    return (_arr(p, "obs_pose", (nO,), np.int64), _arr(p, "obs_landmark", (nO,), np.int64),
            _arr(p, "pose_constant", (p.n_poses,), bool), _arr(p, "speed_bias_constant", (p.n_speed_biases,), bool),
            _arr(p, "landmark_constant", (p.n_landmarks,), bool))


def _check_plain(p):
    if p.n_cameras and p.extrinsics_constant and not all(p.extrinsics_constant[c] for c in range(p.n_cameras)):
        raise ValueError("landmark_residual covers windows without variable extrinsics")


def pose_offsets(p):
    """Offset of every pose's 6 rows in the reduced (natural) ordering, -1 for a constant pose: for
    i = 0 ..: pose i (6, if variable) then speed/bias i (9, if variable)."""
    _, _, pc, sc, _ = _structure(p)
    off, k = np.full(p.n_poses, -1, np.int64), 0
    for i in range(max(p.n_poses, p.n_speed_biases)):
        if i < p.n_poses and not pc[i]:
            off[i] = k
            k += 6
        if i < p.n_speed_biases and not sc[i]:
            k += 9
    return off


def cauchy_weight(r):
    """The Cauchy(1) corrector's weight rho' = 1 / (1 + |r|^2): rho'' < 0, so Ceres scales residual
    and Jacobian by sqrt(rho')."""
    r = np.asarray(r, LD)
    return 1.0 / (1.0 + (r * r).sum(1))


def jacobi_scales(p, r, Jp, Jl, J_imu=None, scaling=True):
    """The Jacobi scales of the pose columns [n_poses, 6] and the landmark columns [n_landmarks, 3]:
    1 / (1 + sqrt(diag(J^T J))) over the robustified Jacobian (Ceres' rule), the squares summed in
    longdouble. Pose columns collect the reprojections, the IMU factors (J_imu [n_imu, 15, 30],
    columns 0..5 and 15..20) and the pose priors, which must sit at their measurement (Jacobian
    -sqrt_info: the synthetic windows' initial state); windows with relative-pose edges or
    host-evaluated factors are refused. scaling = False: all ones."""
    nP, nL = p.n_poses, p.n_landmarks
    if not scaling:
        return np.ones((nP, 6)), np.ones((nL, 3))
    if p.n_host or p.n_relpose:
        raise ValueError("jacobi_scales covers no relative-pose edges and no host-evaluated factors")
    op, ol, _, _, _ = _structure(p)
    w = cauchy_weight(r)
    dp, dl = np.zeros((nP, 6), LD), np.zeros((nL, 3), LD)
    Jp, Jl = np.asarray(Jp, LD), np.asarray(Jl, LD)
    np.add.at(dp, op, w[:, None] * (Jp * Jp).sum(1))
    np.add.at(dl, ol, w[:, None] * (Jl * Jl).sum(1))
    if p.n_imu:
        blocks = _arr(p, "imu_blocks", (p.n_imu, 4), np.int64)
        Ji = np.asarray(J_imu, LD)
        np.add.at(dp, blocks[:, 0], (Ji[:, :, 0:6] ** 2).sum(1))
        np.add.at(dp, blocks[:, 2], (Ji[:, :, 15:21] ** 2).sum(1))
    if p.n_pose_priors:
        n = p.n_pose_priors
        blk = _arr(p, "pose_prior_block", (n,), np.int64)
        meas = _arr(p, "pose_prior_meas", (n, 7), np.float64)
        if not np.array_equal(meas, _arr(p, "poses", (nP, 7), np.float64)[blk]):
            raise ValueError("jacobi_scales covers pose priors at their measurement")
        L = _arr(p, "pose_prior_sqrt_info", (n, 6, 6), LD)
        np.add.at(dp, blk, (L * L).sum(1))
    return (1.0 / (1.0 + np.sqrt(dp))).astype(np.float64), (1.0 / (1.0 + np.sqrt(dl))).astype(np.float64)


class _LandmarkTerms:
    """The operands of the landmark rows of the scaled, damped normal equations, per landmark:
    sg = s g_l, c = s sum_obs J_l^T J_p s_p y_p, Vd = s V s + mu clip(diag(s V s)) (all longdouble)."""

    def __init__(self, p, r, Jp, Jl, scale, mu, y_f, min_lm_diagonal, max_lm_diagonal):
        _check_plain(p)
        op, ol, _, _, lc = _structure(p)
        sp, sl = (np.asarray(a, LD) for a in scale)
        w = cauchy_weight(r)
        r, Jp, Jl, y_f = np.asarray(r, LD), np.asarray(Jp, LD), np.asarray(Jl, LD), np.asarray(y_f, LD)
        off = pose_offsets(p)
        yp = np.zeros((p.n_poses, 6), LD)  # s_p y_p, zero for a constant pose
        free_p = np.flatnonzero(off >= 0)
        yp[free_p] = sp[free_p] * y_f[off[free_p, None] + np.arange(6)]
        nL = p.n_landmarks
        g, c, V = np.zeros((nL, 3), LD), np.zeros((nL, 3), LD), np.zeros((nL, 3, 3), LD)
        np.add.at(g, ol, w[:, None] * np.einsum("oki,ok->oi", Jl, r))
        np.add.at(c, ol, w[:, None] * np.einsum("oki,ok->oi", Jl, np.einsum("okj,oj->ok", Jp, yp[op])))
        np.add.at(V, ol, w[:, None, None] * np.einsum("oki,okj->oij", Jl, Jl))
        Vs = sl[:, :, None] * V * sl[:, None, :]
        d2 = np.clip(np.einsum("lii->li", Vs), min_lm_diagonal, max_lm_diagonal) * LD(mu) if mu > 0 else np.zeros((nL, 3), LD)
        self.free = np.flatnonzero(~lc)
        self.sg, self.c = (sl * g)[self.free], (sl * c)[self.free]
        self.Vd = (Vs + d2[:, :, None] * np.eye(3, dtype=LD))[self.free]


def landmark_residual(p, r, Jp, Jl, scale, mu, y_f, y_l, min_lm_diagonal=MIN_LM_DIAGONAL,
                      max_lm_diagonal=MAX_LM_DIAGONAL):
    """The residual of the landmarks' back substitution in the scaled and damped form of the
    kernels_backsub.hip header, one 3-vector per free landmark (in the caller's order):
        res_l = s g_l - s sum_obs J_l^T J_p s_p y_p - V' y_l,
    formed in longdouble from the raw per-observation r [n_obs, 2], J_pose [n_obs, 2, 6], J_landmark
    [n_obs, 2, 3] and the Cauchy corrector weight; scale = (s_p [n_poses, 6], s_l [n_landmarks, 3]) from
    jacobi_scales, y_f the reduced solution (natural order), y_l [n_landmarks, 3]. Returns (res, den),
    den_l = |V'_l|_inf |y_l|_inf + |s g_l|_inf + |coupling term|_inf, so that
    eta_l = max_l |res_l|_inf / den_l (landmark_eta).

    Covers plain windows: radial-tangential cameras as the evaluation entry points linearise them,
    Cauchy(1) on every reprojection, no variable extrinsics; constant poses (no rows in y_f, no coupling) and constant landmarks (no
    residual) are honoured."""
    t = _LandmarkTerms(p, r, Jp, Jl, scale, mu, y_f, min_lm_diagonal, max_lm_diagonal)
    yl = np.asarray(y_l, LD).reshape(-1, 3)[t.free]
    res = t.sg - t.c - np.einsum("lij,lj->li", t.Vd, yl)
    den = np.abs(t.Vd).sum(2).max(1) * np.abs(yl).max(1) + np.abs(t.sg).max(1) + np.abs(t.c).max(1)
    return res, den


def landmark_eta(res, den):
    return float((np.abs(res).max(1) / den).max()) if len(res) else 0.0


def landmark_backsub(p, r, Jp, Jl, scale, mu, y_f, min_lm_diagonal=MIN_LM_DIAGONAL, max_lm_diagonal=MAX_LM_DIAGONAL):
    """The reference back substitution in float64 (numpy's batched LAPACK solve of V' y_l = s g_l -
    coupling, operands rounded to float64 first): y_l [n_landmarks, 3], zero for constant landmarks."""
    t = _LandmarkTerms(p, r, Jp, Jl, scale, mu, y_f, min_lm_diagonal, max_lm_diagonal)
    y = np.zeros((p.n_landmarks, 3))
    if len(t.free):
        y[t.free] = np.linalg.solve(t.Vd.astype(np.float64), (t.sg - t.c).astype(np.float64)[:, :, None])[:, :, 0]
    return y
