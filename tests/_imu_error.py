"""ImuError::redoPreintegration (okvis_ceres/src/ImuError.cpp:258-466) restated in np.longdouble, the
crafted sample layouts of tests/test_imu_error_paths.py and the error measures they are held to.

`chain` is the high-precision reference of the ImuError kernel's preintegration state: the
reference's formulas and branch thresholds (ode::sinc takes its series below 1e-6, rightJacobian its
constants below 1e-4), the reference's running `time`. dt, the interval and the interpolation
ratios start from Duration::toSec evaluated in double: that quantisation is input, not error.
tests/_gps_error.redo_preintegration is the float64 model of the same loop; `restatement` below is
that model with switches for the mutations of the tests.

Conventions as tests/_imu_propagate.py: quaternions (x, y, z, w), integer nanoseconds, the error state
ordered [r, alpha, v, b_g, b_a], matrices row-major. State offsets are include/okvisgpu.h's
(OKVISGPU_IMU_STATE_DOUBLES)."""
import numpy as np

import okvisgpu as og
from _imu_propagate import cross_mx, dur_to_sec, qinv, qmul, qrot, right_jacobian, sinc
from _problem import OwnedProblem

LD = np.longdouble
U53 = 2.0 ** -53
EPS = 2.0 ** -52

# state offsets (include/okvisgpu.h)
S_COUNTER, S_FLAG, S_REF, S_U, S_STEPS, S_CROSS, S_P = 0, 1, 57, 66, 291, 292, 301
INCREMENTS = (("Delta_q", 2, 4), ("C_integral", 6, 9), ("C_doubleintegral", 15, 9), ("acc_integral", 24, 3),
              ("acc_doubleintegral", 27, 3), ("dalpha_db_g", 30, 9), ("dv_db_g", 39, 9), ("dp_db_g", 48, 9))

SIZES = (2, 3, 4, 5, 16, 17, 22, 33, 49, 50, 64)
GRID_NS = 5_000_000
JITTER_NS = 400_000


def _ld(a):
    return np.asarray(a, dtype=LD)


def _qmul(a, b):
    return _ld(qmul(a, b))


def _sinc_ld(x):
    if abs(x) > 1.0e-6:
        return np.sin(x) / x
    x2 = x * x
    return LD(1) - x2 / LD(6) + x2 * x2 / LD(120) - x2 * x2 * x2 / LD(5040)


def _right_jacobian_ld(p):
    phi = np.sqrt(p @ p)
    X = _ld(cross_mx(p))
    I = np.eye(3, dtype=LD)
    if phi < 1.0e-4:
        return I - LD(0.5) * X + X @ X / LD(6)
    return I - (LD(1) - np.cos(phi)) / (phi * phi) * X + (phi - np.sin(phi)) / (phi * phi * phi) * X @ X


def chain(ts, ga, ip, sb, t0, t1, init=None):
    """One factor in np.longdouble. Returns a dict: the increments (INCREMENTS' names), "cross",
    "P" (the symmetrised P_delta_), "steps" and "state" (a longdouble vector in the layout of
    imu_state with [2..56], [292..300] and [301..525] filled); None when the samples do not reach t1
    (:270-273). With `init` (an earlier result) it is ImuError::append (:63-255): the loop continues from
    init's members at t0 (the old t1) over the given samples with the bias `sb`; "steps" counts the appended."""
    ts = np.asarray(ts, dtype=np.int64)
    ga = _ld(np.asarray(ga, dtype=np.float64).reshape(-1, 6))
    sb = _ld(sb)
    N = len(ts)
    if not ts[-1] >= t1:
        return None
    one, half, quarter = LD(1), LD(0.5), LD(0.25)
    time = int(t0)
    Dq = _ld([0, 0, 0, 1])
    C_int, C_dint = np.zeros((3, 3), LD), np.zeros((3, 3), LD)
    a_int, a_dint = np.zeros(3, LD), np.zeros(3, LD)
    cross = np.zeros((3, 3), LD)
    dalpha_db_g, dv_db_g, dp_db_g = np.zeros((3, 3), LD), np.zeros((3, 3), LD), np.zeros((3, 3), LD)
    dPdsigma = [np.zeros((15, 15), LD) for _ in range(4)]
    I3 = np.eye(3, dtype=LD)
    if init is not None:                                       # :93-94: all left, not reset
        Dq, C_int, C_dint, a_int, a_dint, dalpha_db_g, dv_db_g, dp_db_g = (init[name].copy() for name, _, _ in INCREMENTS)
        cross = init["cross"].copy()
        dPdsigma = [m.copy() for m in init["dPdsigma"]]
    started = False
    steps = 0
    for k in range(N):
        om0, ac0 = ga[k, :3].copy(), ga[k, 3:].copy()
        om1, ac1 = (ga[k + 1, :3].copy(), ga[k + 1, 3:].copy()) if k + 1 < N else (om0.copy(), ac0.copy())
        nexttime = int(t1) if k + 1 == N else int(ts[k + 1])   # :310-315
        dt = LD(dur_to_sec(nexttime - time))
        if t1 < nexttime:                                      # :317-324
            interval = LD(dur_to_sec(nexttime - int(ts[k])))
            nexttime = int(t1)
            dt = LD(dur_to_sec(nexttime - time))
            r = dt / interval
            om1 = (one - r) * om0 + r * om1
            ac1 = (one - r) * ac0 + r * ac1
        if dt <= 0:                                            # :326-328
            continue
        if not started:                                        # :330-335
            started = True
            r = dt / LD(dur_to_sec(nexttime - int(ts[k])))
            om0 = r * om0 + (one - r) * om1
            ac0 = r * ac0 + (one - r) * ac1
        gyr_sat_mult = acc_sat_mult = one                      # :338-358
        if max(np.abs(om0).max(), np.abs(om1).max()) > ip.g_max:
            gyr_sat_mult = LD(100)
        if max(np.abs(ac0).max(), np.abs(ac1).max()) > ip.a_max:
            acc_sat_mult = LD(100)
        w_true = half * (om0 + om1) - sb[3:6]                  # :362-392
        theta_half = np.sqrt(w_true @ w_true) * half * dt
        dq = np.concatenate([_sinc_ld(theta_half) * w_true * half * dt, [np.cos(theta_half)]])
        Dq1 = _qmul(Dq, dq)
        C, C1 = _ld(qrot(Dq)), _ld(qrot(Dq1))
        a_true = half * (ac0 + ac1) - sb[6:9]
        C_int1 = C_int + half * (C + C1) * dt
        a_int1 = a_int + half * (C + C1) @ a_true * dt
        dp_step = a_int * dt + quarter * (C + C1) @ a_true * dt * dt
        F012 = -C_int * dt + quarter * (C + C1) * dt * dt
        C_dint = C_dint + C_int * dt + quarter * (C + C1) * dt * dt
        a_dint = a_dint + dp_step
        Jr = _right_jacobian_ld(w_true * dt)
        dalpha_db_g = dalpha_db_g + C1 @ Jr * dt
        dqi = np.array([-dq[0], -dq[1], -dq[2], dq[3]]) / (dq @ dq)
        cross1 = _ld(qrot(dqi)) @ cross + Jr * dt
        ax = _ld(cross_mx(a_true))
        X = C @ ax @ cross + C1 @ ax @ cross1
        dv_db_g1 = dv_db_g + half * dt * X
        dp_db_g_step = dt * dv_db_g + quarter * dt * dt * X
        dp_db_g = dp_db_g + dp_db_g_step
        F = np.eye(15, dtype=LD)                               # :395-410
        F[0:3, 3:6] = -_ld(cross_mx(dp_step))
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = dp_db_g_step
        F[0:3, 12:15] = F012
        F[3:6, 9:12] = -dt * C1
        F[6:9, 3:6] = -_ld(cross_mx(half * (C + C1) @ a_true * dt))
        F[6:9, 9:12] = half * dt * X
        F[6:9, 12:15] = -half * (C + C1) * dt
        K = [np.zeros((15, 15), LD) for _ in range(4)]         # :413-426
        K[0][3:6, 3:6] = gyr_sat_mult * dt * I3
        K[1][0:3, 0:3] = half * dt * dt * dt * acc_sat_mult * acc_sat_mult * acc_sat_mult * I3
        K[1][6:9, 6:9] = acc_sat_mult * dt * I3
        K[2][9:12, 9:12] = dt * I3
        K[3][12:15, 12:15] = dt * I3
        for j in range(4):
            dPdsigma[j] = F @ dPdsigma[j] @ F.T + K[j]
        Dq, C_int, a_int, cross, dv_db_g, time = Dq1, C_int1, a_int1, cross1, dv_db_g1, nexttime  # :434-439
        steps += 1
        if nexttime == t1:                                     # :443-444
            break
    for j in range(4):                                         # :453-459
        dPdsigma[j] = half * dPdsigma[j] + half * dPdsigma[j].T
    P = dPdsigma[0] * LD(ip.sigma_g_c) * LD(ip.sigma_g_c)
    P = P + dPdsigma[1] * LD(ip.sigma_a_c) * LD(ip.sigma_a_c)
    P = P + dPdsigma[2] * LD(ip.sigma_gw_c) * LD(ip.sigma_gw_c)
    P = P + dPdsigma[3] * LD(ip.sigma_aw_c) * LD(ip.sigma_aw_c)
    out = {"Delta_q": Dq, "C_integral": C_int, "C_doubleintegral": C_dint, "acc_integral": a_int,
           "acc_doubleintegral": a_dint, "dalpha_db_g": dalpha_db_g, "dv_db_g": dv_db_g, "dp_db_g": dp_db_g,
           "cross": cross, "P": P, "steps": steps, "dPdsigma": dPdsigma}
    state = np.zeros(og.IMU_STATE_DOUBLES, LD)
    for name, off, n in INCREMENTS:
        state[off:off + n] = out[name].reshape(-1)
    state[S_CROSS:S_CROSS + 9] = cross.reshape(-1)
    state[S_P:S_P + 225] = P.reshape(-1)
    out["state"] = state
    return out


def restatement(ts, ga, ip, sb, t0, t1, mutation=None):
    """The float64 loop of tests/_gps_error.redo_preintegration (:258-466, the same loop as
    GpsErrorAsynchronous's) with cross_ kept, into an imu_state-shaped vector; returns (state, steps).
    `mutation` makes it subtly wrong, one way a chunked, lane-parallel kernel can be:
      "step_start_ts"   a step after the first starts at max(t0, min(ts[k], t1)), not at the running time;
      "dup_prev_dt"     a step with dt <= 0 is integrated with the previous step's dt, not skipped;
      "no_saturation"   the saturation multipliers stay 1;
      "restart_chunk"   the first integrated step of the chunk of four holding step 8 is interpolated
                        again as if none had been integrated before it."""
    ts = np.asarray(ts, dtype=np.int64)
    ga = np.asarray(ga, dtype=np.float64).reshape(-1, 6)
    sb = np.asarray(sb, dtype=np.float64)
    N = len(ts)
    assert ts[-1] >= t1
    time = int(t0)
    Dq = np.array([0.0, 0.0, 0.0, 1.0])
    C_int, C_dint = np.zeros((3, 3)), np.zeros((3, 3))
    a_int, a_dint = np.zeros(3), np.zeros(3)
    cross = np.zeros((3, 3))
    dalpha_db_g, dv_db_g, dp_db_g = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
    dPdsigma = [np.zeros((15, 15)) for _ in range(4)]
    started = False
    steps = 0
    prev_dt = 0.0
    restarted = False
    for k in range(N):
        om0, ac0 = ga[k, :3].copy(), ga[k, 3:].copy()
        om1, ac1 = (ga[k + 1, :3].copy(), ga[k + 1, 3:].copy()) if k + 1 < N else (om0.copy(), ac0.copy())
        nexttime = int(t1) if k + 1 == N else int(ts[k + 1])
        if mutation == "step_start_ts" and k > 0:
            time = max(int(t0), min(int(ts[k]), int(t1)))
        dt = dur_to_sec(nexttime - time)
        if t1 < nexttime:
            interval = dur_to_sec(nexttime - int(ts[k]))
            nexttime = int(t1)
            dt = dur_to_sec(nexttime - time)
            r = dt / interval
            om1 = (1.0 - r) * om0 + r * om1
            ac1 = (1.0 - r) * ac0 + r * ac1
        if dt <= 0.0:
            if not (mutation == "dup_prev_dt" and started and nexttime < t1 and prev_dt > 0.0):
                continue
            dt = prev_dt
        first = not started
        if mutation == "restart_chunk" and started and not restarted and k >= 8:
            first = restarted = True
        if first:
            started = True
            r = dt / dur_to_sec(nexttime - int(ts[k]))
            om0 = r * om0 + (1.0 - r) * om1
            ac0 = r * ac0 + (1.0 - r) * ac1
        gyr_sat_mult = acc_sat_mult = 1.0
        if mutation != "no_saturation":
            if max(np.abs(om0).max(), np.abs(om1).max()) > ip.g_max:
                gyr_sat_mult *= 100
            if max(np.abs(ac0).max(), np.abs(ac1).max()) > ip.a_max:
                acc_sat_mult *= 100
        w_true = 0.5 * (om0 + om1) - sb[3:6]
        theta_half = np.linalg.norm(w_true) * 0.5 * dt
        dq = np.concatenate([sinc(theta_half) * w_true * 0.5 * dt, [np.cos(theta_half)]])
        Dq1 = qmul(Dq, dq)
        C, C1 = qrot(Dq), qrot(Dq1)
        a_true = 0.5 * (ac0 + ac1) - sb[6:9]
        C_int1 = C_int + 0.5 * (C + C1) * dt
        a_int1 = a_int + 0.5 * (C + C1) @ a_true * dt
        dp_step = a_int * dt + 0.25 * (C + C1) @ a_true * dt * dt
        F012 = -C_int * dt + 0.25 * (C + C1) * dt * dt
        C_dint = C_dint + C_int * dt + 0.25 * (C + C1) * dt * dt
        a_dint = a_dint + dp_step
        Jr = right_jacobian(w_true * dt)
        dalpha_db_g = dalpha_db_g + C1 @ Jr * dt
        cross1 = qrot(qinv(dq)) @ cross + Jr * dt
        ax = cross_mx(a_true)
        X = C @ ax @ cross + C1 @ ax @ cross1
        dv_db_g1 = dv_db_g + 0.5 * dt * X
        dp_db_g_step = dt * dv_db_g + 0.25 * dt * dt * X
        dp_db_g = dp_db_g + dp_db_g_step
        F = np.eye(15)
        F[0:3, 3:6] = -cross_mx(dp_step)
        F[0:3, 6:9] = np.eye(3) * dt
        F[0:3, 9:12] = dp_db_g_step
        F[0:3, 12:15] = F012
        F[3:6, 9:12] = -dt * C1
        F[6:9, 3:6] = -cross_mx(0.5 * (C + C1) @ a_true * dt)
        F[6:9, 9:12] = 0.5 * dt * X
        F[6:9, 12:15] = -0.5 * (C + C1) * dt
        K = [np.zeros((15, 15)) for _ in range(4)]
        K[0][3:6, 3:6] = gyr_sat_mult * dt * np.eye(3)
        K[1][0:3, 0:3] = 0.5 * dt * dt * dt * acc_sat_mult * acc_sat_mult * acc_sat_mult * np.eye(3)
        K[1][6:9, 6:9] = acc_sat_mult * dt * np.eye(3)
        K[2][9:12, 9:12] = dt * np.eye(3)
        K[3][12:15, 12:15] = dt * np.eye(3)
        for j in range(4):
            dPdsigma[j] = F @ dPdsigma[j] @ F.T + K[j]
        Dq, C_int, a_int, cross, dv_db_g, time = Dq1, C_int1, a_int1, cross1, dv_db_g1, nexttime
        prev_dt = dt
        steps += 1
        if nexttime == t1:
            break
    for j in range(4):
        dPdsigma[j] = 0.5 * dPdsigma[j] + 0.5 * dPdsigma[j].T
    P = dPdsigma[0] * ip.sigma_g_c * ip.sigma_g_c
    P = P + dPdsigma[1] * ip.sigma_a_c * ip.sigma_a_c
    P = P + dPdsigma[2] * ip.sigma_gw_c * ip.sigma_gw_c
    P = P + dPdsigma[3] * ip.sigma_aw_c * ip.sigma_aw_c
    state = np.zeros(og.IMU_STATE_DOUBLES)
    for (_, off, n), v in zip(INCREMENTS, (Dq, C_int, C_dint, a_int, a_dint, dalpha_db_g, dv_db_g, dp_db_g)):
        state[off:off + n] = np.asarray(v).reshape(-1)
    state[S_CROSS:S_CROSS + 9] = cross.reshape(-1)
    state[S_P:S_P + 225] = P.reshape(-1)
    state[S_REF:S_REF + 9] = sb
    state[S_STEPS] = steps
    return state, steps


# ---- the square-root information at high precision --------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def _to_mp(A):
    mp = _mp()
    A = _ld(A)
    # (a longdouble is the exact sum of its two double halves)
    return mp.matrix([[mp.mpf(float(x)) + mp.mpf(float(x - LD(float(x)))) for x in row] for row in A])


def _from_mp(M):
    out = np.zeros((M.rows, M.cols), LD)
    for i in range(M.rows):
        for j in range(M.cols):
            hi = float(M[i, j])
            out[i, j] = LD(hi) + LD(float(M[i, j] - hi))
    return out


def zero_walk(ip):
    return ip.sigma_gw_c == 0.0 and ip.sigma_aw_c == 0.0


def clamp_tol(P_ld):
    """PseudoInverse.hpp:138: max(eps, 15 eps lambda_max)."""
    mp = _mp()
    lam = mp.eigsy(_to_mp(P_ld), eigvals_only=True)
    return max(EPS, 15.0 * EPS * float(max(lam)))


def information(P_ld, ip):
    """squareRootInformation_^T squareRootInformation_ of PseudoInverse::symmSqrtU (PseudoInverse.hpp:132-158)
    for the covariance P_ld, as a longdouble matrix: the inverse, or with zero bias random-walk densities
    (the bias rows of P are then exactly zero and their eigenvalues clamped to tol) blockdiag(inverse of the
    leading 9x9, I / tol)."""
    mp = _mp()
    if not zero_walk(ip):
        return _from_mp(mp.inverse(_to_mp(P_ld)))
    P_ld = _ld(P_ld)
    assert not P_ld[9:, :].any() and not P_ld[:, 9:].any()
    out = np.zeros((15, 15), LD)
    out[:9, :9] = _from_mp(mp.inverse(_to_mp(P_ld[:9, :9])))
    out[9:, 9:] = np.eye(6, dtype=LD) / LD(clamp_tol(P_ld))
    return out


# ---- error measures ---------------------------------------------------------------------------------
def err_increments(state, ref):
    """max over [2..56] of |x - ref| / max(1, |ref|)."""
    d = np.abs(_ld(state[2:57]) - ref["state"][2:57]) / np.maximum(1, np.abs(ref["state"][2:57]))
    return float(d.max())


def err_cross(state, ref):
    d = np.abs(_ld(state[S_CROSS:S_CROSS + 9]) - ref["state"][S_CROSS:S_CROSS + 9])
    return float((d / np.maximum(1, np.abs(ref["state"][S_CROSS:S_CROSS + 9]))).max())


def err_P(state, ref, nonzero=15):
    """max |P - ref| / sqrt(P_ii P_jj) over the leading `nonzero` rows and columns; what lies outside must be 0."""
    P = _ld(state[S_P:S_P + 225]).reshape(15, 15)
    R = ref["P"]
    n = nonzero
    if n < 15:
        assert not P[n:, :].any() and not P[:, n:].any()
    d = np.sqrt(np.diag(R)[:n])
    return float((np.abs(P[:n, :n] - R[:n, :n]) / np.outer(d, d)).max())


def err_U(state, ref):
    """|U P_ld U^T - I|_max in longdouble (any orthogonal basis of the square root passes)."""
    U = _ld(state[S_U:S_U + 225]).reshape(15, 15)
    return float(np.abs(U @ ref["P"] @ U.T - np.eye(15, dtype=LD)).max())


def err_info_blocks(state, info):
    """U^T U against information(): leading 9x9, bias block, cross block, each relative to the Frobenius
    norm of its reference (the zero cross block: to that of the two diagonal blocks' geometric mean)."""
    U = _ld(state[S_U:S_U + 225]).reshape(15, 15)
    A = U.T @ U
    fro = lambda M: np.sqrt((M * M).sum())
    lead = fro(A[:9, :9] - info[:9, :9]) / fro(info[:9, :9])
    bias = fro(A[9:, 9:] - info[9:, 9:]) / fro(info[9:, 9:])
    crs = fro(A[:9, 9:] - info[:9, 9:]) / np.sqrt(fro(info[:9, :9]) * fro(info[9:, 9:]))
    return float(lead), float(bias), float(crs)


def bound(e_ref, floor_u):
    """16 max(e_ref, floor_u u): the factor _linsolve.bound allows another summation order (here the
    phase-split running sums, the block-sparse F_delta and the half-angle right Jacobian)."""
    return 16.0 * max(e_ref, floor_u * U53)


# ---- the layouts --------------------------------------------------------------------------------------
def imu_params(zero_walk_densities=False):
    """The generator's (synth.cpp) limits and noise densities."""
    ip = og.ImuParams()
    ip.a_max, ip.g_max = 176.0, 7.8
    ip.sigma_g_c, ip.sigma_a_c = 20.0e-4, 20.0e-3
    ip.sigma_gw_c, ip.sigma_aw_c = (0.0, 0.0) if zero_walk_densities else (20.0e-5, 20.0e-3)
    ip.g = 9.81007
    return ip


def samples(rng, n, sb, gyro_sigma=0.3):
    """n samples on the 5 ms grid, interior stamps jittered; (t0, t1) strictly inside the first and the last
    interval."""
    ts = 1_000_000_000 + GRID_NS * np.arange(n, dtype=np.int64)
    if n > 2:
        ts[1:-1] += rng.integers(-JITTER_NS, JITTER_NS + 1, n - 2)
    ga = np.concatenate([gyro_sigma * rng.standard_normal((n, 3)),
                         np.array([0.0, 0.0, 9.81]) + rng.standard_normal((n, 3))], axis=1)
    if n == 2:
        t0 = int(ts[0] + rng.integers(500_000, 2_000_000))
        t1 = int(ts[1] - rng.integers(500_000, 2_000_000))
    else:
        t0 = int(ts[0] + rng.integers(500_000, ts[1] - ts[0] - 500_000))
        t1 = int(ts[-1] - rng.integers(500_000, ts[-1] - ts[-2] - 500_000))
    return ts, ga, t0, t1


def speed_bias(rng):
    return np.concatenate([rng.standard_normal(3), 0.01 * rng.standard_normal(3), 0.05 * rng.standard_normal(3)])


def layouts(rng, ip):
    """The named factors of the first crafted window: {name: (ts, ga, t0, t1, sb)}, in the window's order."""
    out = {}
    for n in SIZES:
        sb = speed_bias(rng)
        out[f"N{n}"] = samples(rng, n, sb) + (sb,)

    def make(name, n, edit, **kw):
        sb = speed_bias(rng)
        ts, ga, t0, t1 = samples(rng, n, sb, **kw)
        out[name] = tuple(edit(ts, ga, t0, t1, sb)) + (sb,)

    make("on_stamps", 12, lambda ts, ga, t0, t1, sb: (ts, ga, int(ts[0]), int(ts[-1])))

    def dup_mid(ts, ga, t0, t1, sb):
        ts[9] = ts[8]
        return ts, ga, t0, t1
    make("dup_mid", 14, dup_mid)
    make("early", 14, lambda ts, ga, t0, t1, sb: (ts, ga, int(ts[5] + (ts[6] - ts[5]) // 3), t1))
    make("late", 20, lambda ts, ga, t0, t1, sb: (ts, ga, t0, int(ts[12] + (ts[13] - ts[12]) // 3)))
    make("early_late_on", 14, lambda ts, ga, t0, t1, sb: (ts, ga, int(ts[4]), int(ts[8])))

    def saturated(ts, ga, t0, t1, sb):
        ga[5, 1] = 2.0 * ip.g_max
        ga[9, 5] = -1.5 * ip.a_max
        return ts, ga, t0, t1
    make("saturated", 14, saturated)

    def still(ts, ga, t0, t1, sb):  # (the two interpolated end steps round r b + (1 - r) b: theta_half ~ 1e-19)
        ga[:, :3] = sb[3:6]
        return ts, ga, t0, t1
    make("still", 12, still)

    def slow(ts, ga, t0, t1, sb):
        ga[:, :3] = sb[3:6] + 1e-7 * np.array([0.6, -0.64, 0.48])
        return ts, ga, t0, t1
    make("slow", 12, slow)

    def phi(ts, ga, t0, t1, sb):
        ga[:, :3] += sb[3:6]
        return ts, ga, t0, t1
    make("phi_1e-4", 22, phi, gyro_sigma=0.015)

    def backwards(ts, ga, t0, t1, sb):
        ts[6] = ts[4] + 1_000_000
        return ts, ga, t0, t1
    make("backwards", 12, backwards)

    # (the same two samples later, so that the step taking up the running time, step 8, is the first of a
    # chunk of four. Only there does the first-step interpolation of a chunk that forgot `started` differ
    # from the identity: where a step starts at its own stamp its ratio is dt / dt = 1.)
    def backwards_8(ts, ga, t0, t1, sb):
        ts[8] = ts[6] + 1_000_000
        return ts, ga, t0, t1
    make("backwards_8", 12, backwards_8)
    make("uncovered", 12, lambda ts, ga, t0, t1, sb: (ts, ga, t0, int(ts[-1] + 1_000_000)))
    assert len(out) % 4 != 0  # a workgroup of four factors then holds factors of both crafted windows
    return out


def zero_walk_layouts(rng):
    """The second crafted window (zero bias random-walk densities): N = 5 and N = 22."""
    out = {}
    for n in (5, 22):
        sb = speed_bias(rng)
        out[f"zero_walk_N{n}"] = samples(rng, n, sb) + (sb,)
    return out


def problem(factors, ip, rng):
    """An OwnedProblem of IMU factors only: len(factors) + 1 poses and speed/biases, factor f on the blocks
    (f, f, f + 1, f + 1) with the layout's speed/bias at state f, fresh functor states, no observations."""
    factors = list(factors)
    n = len(factors)
    p = OwnedProblem()
    q = rng.standard_normal((n + 1, 4))
    p.poses = np.concatenate([rng.standard_normal((n + 1, 3)), q / np.linalg.norm(q, axis=1)[:, None]], axis=1)
    p.pose_constant = np.zeros(n + 1, np.uint8)
    p.speed_biases = np.array([f[4] for f in factors] + [speed_bias(rng)])
    p.speed_bias_constant = np.zeros(n + 1, np.uint8)
    p.imu_blocks = np.array([[f, f, f + 1, f + 1] for f in range(n)], np.int32)
    p.imu_t0_ns = np.array([f[2] for f in factors], np.int64)
    p.imu_t1_ns = np.array([f[3] for f in factors], np.int64)
    p.imu_sample_begin = np.concatenate([[0], np.cumsum([len(f[0]) for f in factors])]).astype(np.int32)
    p.imu_sample_t_ns = np.concatenate([f[0] for f in factors])
    p.imu_sample_gyr_acc = np.concatenate([f[1] for f in factors])
    p.imu_state = np.zeros((n, og.IMU_STATE_DOUBLES))
    p.imu_params = ip
    return p.bind()
