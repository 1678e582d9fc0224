"""GpsErrorAsynchronous (okvis_ceres/src/GpsErrorAsynchronous.cpp:98-507) and GpsErrorSynchronous
(GpsErrorSynchronous.cpp:41-144) restated in numpy: the reference of tests/test_gps_error.py for
okvisgpu_gps_evaluate. A literal restatement: four dPdsigma matrices, the full 15x15 Jprop and T, the
products in the reference's order.

Conventions are the reference's: quaternions (x, y, z, w) with the Hamilton product, times in integer
nanoseconds (okvis::Time differences go through Duration::toSec), the error state ordered
[r, alpha, v, b_g, b_a], matrices row-major. The functor's mutable members live in a `state` vector
of OKVISGPU_GPS_STATE_DOUBLES entries (include/okvisgpu.h). Line numbers cite GpsErrorAsynchronous.cpp
unless a file is named."""
import numpy as np

from _gps import lift
from _imu_propagate import cross_mx, delta_q, dur_to_sec, qinv, qmul, qrot, right_jacobian, sinc

STATE = 292
S_COUNTER, S_FLAG, S_DQ, S_CI, S_CDI, S_AI, S_ADI, S_DADBG, S_DVDBG, S_DPDBG, S_REF, S_STEPS, S_P = (
    0, 1, 2, 6, 15, 24, 27, 30, 39, 48, 57, 66, 67)
OUTPUTS = ("r", "error", "sqrt_info", "J_pose", "J_speed_bias", "J_T_GW", "J_pose_ambient", "J_T_GW_ambient", "steps")


def llt_upper(A):
    """Eigen::LLT(A).matrixL().transpose()."""
    return np.linalg.cholesky(np.asarray(A, dtype=np.float64)).T


def redo_preintegration(state, ts, ga, ip, sb, t_k, t_g, use_imu_covariance):
    """:303-507 into `state`; returns the integrated steps. The samples cover [t_k, t_g] (the device
    refuses the rest: deviation 2); with t_g == t_k nothing is integrated (deviation 3)."""
    ts = np.asarray(ts, dtype=np.int64)
    ga = np.asarray(ga, dtype=np.float64).reshape(-1, 6)
    N = len(ts)
    assert N > 0 and ts[0] <= t_k, ":311"
    assert ts[-1] >= t_g and t_g >= t_k, ":312 / ViGraph.cpp:976-982"
    time = int(t_k)
    Dq = np.array([0.0, 0.0, 0.0, 1.0])                        # :316-337
    C_int, C_dint = np.zeros((3, 3)), np.zeros((3, 3))
    a_int, a_dint = np.zeros(3), np.zeros(3)
    cross = np.zeros((3, 3))
    dalpha_db_g, dv_db_g, dp_db_g = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
    P_delta = np.zeros((15, 15))
    dPdsigma = [np.zeros((15, 15)) for _ in range(4)]
    started = False
    steps = 0
    for k in range(N):
        om0, ac0 = ga[k, :3].copy(), ga[k, 3:].copy()
        # (past the end the reference reads nothing it uses: such a step has dt <= 0)
        om1, ac1 = (ga[k + 1, :3].copy(), ga[k + 1, 3:].copy()) if k + 1 < N else (om0.copy(), ac0.copy())
        nexttime = int(t_g) if k + 1 == N else int(ts[k + 1])   # :350-355
        dt = dur_to_sec(nexttime - time)
        if t_g < nexttime:                                     # :357-364
            interval = dur_to_sec(nexttime - int(ts[k]))
            nexttime = int(t_g)
            dt = dur_to_sec(nexttime - time)
            r = dt / interval
            om1 = (1.0 - r) * om0 + r * om1
            ac1 = (1.0 - r) * ac0 + r * ac1
        if dt <= 0.0:                                          # :366-368
            continue
        if not started:                                        # :370-375
            started = True
            r = dt / dur_to_sec(nexttime - int(ts[k]))
            om0 = r * om0 + (1.0 - r) * om1
            ac0 = r * ac0 + (1.0 - r) * ac1
        gyr_sat_mult = acc_sat_mult = 1.0                      # :378-398
        if max(np.abs(om0).max(), np.abs(om1).max()) > ip.g_max:
            gyr_sat_mult *= 100
        if max(np.abs(ac0).max(), np.abs(ac1).max()) > ip.a_max:
            acc_sat_mult *= 100
        w_true = 0.5 * (om0 + om1) - sb[3:6]                   # :402-432
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
        if use_imu_covariance:
            F = np.eye(15)                                     # :437-452
            F[0:3, 3:6] = -cross_mx(dp_step)
            F[0:3, 6:9] = np.eye(3) * dt
            F[0:3, 9:12] = dp_db_g_step
            F[0:3, 12:15] = F012
            F[3:6, 9:12] = -dt * C1
            F[6:9, 3:6] = -cross_mx(0.5 * (C + C1) @ a_true * dt)
            F[6:9, 9:12] = 0.5 * dt * X
            F[6:9, 12:15] = -0.5 * (C + C1) * dt
            K = [np.zeros((15, 15)) for _ in range(4)]         # :455-463
            K[0][3:6, 3:6] = gyr_sat_mult * dt * np.eye(3)
            K[1][0:3, 0:3] = 0.5 * dt * dt * dt * acc_sat_mult * acc_sat_mult * acc_sat_mult * np.eye(3)
            K[1][6:9, 6:9] = acc_sat_mult * dt * np.eye(3)
            K[2][9:12, 9:12] = dt * np.eye(3)
            K[3][12:15, 12:15] = dt * np.eye(3)
            for j in range(4):                                 # :464-467
                dPdsigma[j] = F @ dPdsigma[j] @ F.T + K[j]
        Dq, C_int, a_int, cross, dv_db_g, time = Dq1, C_int1, a_int1, cross1, dv_db_g1, nexttime  # :473-478
        steps += 1
        if nexttime == t_g:                                    # :482-483
            break
    if use_imu_covariance:                                     # :494-500
        for j in range(4):
            dPdsigma[j] = 0.5 * dPdsigma[j] + 0.5 * dPdsigma[j].T
        P_delta = dPdsigma[0] * ip.sigma_g_c * ip.sigma_g_c
        P_delta = P_delta + dPdsigma[1] * ip.sigma_a_c * ip.sigma_a_c
        P_delta = P_delta + dPdsigma[2] * ip.sigma_gw_c * ip.sigma_gw_c
        P_delta = P_delta + dPdsigma[3] * ip.sigma_aw_c * ip.sigma_aw_c
    state[S_DQ:S_DQ + 4] = Dq
    state[S_CI:S_CI + 9] = C_int.reshape(-1)
    state[S_CDI:S_CDI + 9] = C_dint.reshape(-1)
    state[S_AI:S_AI + 3] = a_int
    state[S_ADI:S_ADI + 3] = a_dint
    state[S_DADBG:S_DADBG + 9] = dalpha_db_g.reshape(-1)
    state[S_DVDBG:S_DVDBG + 9] = dv_db_g.reshape(-1)
    state[S_DPDBG:S_DPDBG + 9] = dp_db_g.reshape(-1)
    state[S_REF:S_REF + 9] = sb                                # :488
    state[S_STEPS] = steps
    state[S_P:S_P + 225] = P_delta.reshape(-1)
    return steps


def _finish(S, z, T_WS_in, T_GW, C_GW, r_tg, a_tg, J0_min, J1_min, steps):
    """:200-294 / GpsErrorSynchronous.cpp:80-140 from the antenna position on."""
    p_G = C_GW @ (r_tg + a_tg)
    error = z - (p_G + T_GW[:3])
    J2_min = np.hstack([-np.eye(3), cross_mx(p_G)])
    J0, J2 = S @ J0_min, S @ J2_min
    return {"r": S @ error, "error": error, "sqrt_info": S, "J_pose": J0, "J_speed_bias": S @ J1_min, "J_T_GW": J2,
            "J_pose_ambient": J0 @ lift(T_WS_in), "J_T_GW_ambient": J2 @ lift(T_GW), "steps": steps}


def evaluate_async(ts, ga, ip, r_SA, T_WS, sb, T_GW, z, information, t_k, t_g, state=None, use_imu_covariance=True,
                   redo_propagation_always=False):
    """GpsErrorAsynchronous::EvaluateWithMinimalJacobians (:98-300) of one factor; `state` (None: a fresh
    functor) is updated in place. Returns the dict of OUTPUTS."""
    T_WS, sb, T_GW = (np.asarray(a, dtype=np.float64) for a in (T_WS, sb, T_GW))
    r_SA, z, information = (np.asarray(a, dtype=np.float64) for a in (r_SA, z, information))
    information = information.reshape(3, 3)
    state = np.zeros(STATE) if state is None else state
    r_WS = T_WS[:3]
    q_WS = T_WS[3:] / np.linalg.norm(T_WS[3:])                 # Transformation's constructor normalises
    C_GW = qrot(T_GW[3:])                                      # :117-118, as stored
    C_WS_tk = qrot(q_WS)
    Delta_t = dur_to_sec(int(t_g) - int(t_k))                  # :129
    Delta_b = sb[3:9] - state[S_REF + 3:S_REF + 9]             # :134-142
    redo = bool(state[S_FLAG]) or np.sqrt(Delta_b[:3] @ Delta_b[:3]) > 0.0003
    if redo_propagation_always or (redo and len(ts) < 50) or state[S_COUNTER] == 0:
        redo_preintegration(state, ts, ga, ip, sb, t_k, t_g, use_imu_covariance)
        state[S_COUNTER] += 1
        Delta_b = np.zeros(6)
        redo = False
    state[S_FLAG] = 1.0 if redo else 0.0
    Dq = state[S_DQ:S_DQ + 4]
    C_int, C_dint = state[S_CI:S_CI + 9].reshape(3, 3), state[S_CDI:S_CDI + 9].reshape(3, 3)
    a_int, a_dint = state[S_AI:S_AI + 3], state[S_ADI:S_ADI + 3]
    dalpha_db_g, dv_db_g, dp_db_g = (state[o:o + 9].reshape(3, 3) for o in (S_DADBG, S_DVDBG, S_DPDBG))
    P_delta = state[S_P:S_P + 225].reshape(15, 15)
    g_W = np.array([0.0, 0.0, ip.g])                           # :147
    r_tg = (r_WS + sb[:3] * Delta_t - 0.5 * g_W * Delta_t * Delta_t
            + C_WS_tk @ (a_dint + dp_db_g @ Delta_b[:3] - C_dint @ Delta_b[3:]))  # :151-152
    q_tg = qmul(qmul(q_WS, Dq), delta_q(-dalpha_db_g @ Delta_b[:3]))
    q_tg = q_tg / np.linalg.norm(q_tg)                         # Transformation::set normalises
    C_tg = qrot(q_tg)
    Jprop = np.eye(15)                                         # :156-166
    Jprop[0:3, 3:6] = -cross_mx(C_WS_tk @ a_dint)
    Jprop[0:3, 6:9] = np.eye(3) * Delta_t
    Jprop[0:3, 9:12] = C_WS_tk @ dp_db_g
    Jprop[0:3, 12:15] = -C_WS_tk @ C_dint
    Jprop[3:6, 9:12] = -C_WS_tk @ dalpha_db_g
    Jprop[6:9, 3:6] = -cross_mx(C_WS_tk @ a_int)
    Jprop[6:9, 9:12] = C_WS_tk @ dv_db_g
    Jprop[6:9, 12:15] = -C_WS_tk @ C_int
    gps_covariance = np.linalg.inv(information)                # :87
    if use_imu_covariance:                                     # :173-187
        T = np.eye(15)
        T[0:3, 0:3] = T[3:6, 3:6] = T[6:9, 6:9] = C_WS_tk
        P = T @ P_delta @ T.T
        Jws = np.hstack([C_GW, -C_GW @ cross_mx(C_WS_tk @ r_SA)])
        cov_overall = gps_covariance + Jws @ P[0:6, 0:6] @ Jws.T
        S = llt_upper(np.linalg.inv(cov_overall))
    else:                                                      # :192-193
        S = llt_upper(np.linalg.inv(gps_covariance))
    a_tg = C_tg @ r_SA
    J_tg = np.hstack([-C_GW, C_GW @ cross_mx(a_tg)])           # :215-218, :246-249
    J0_min = J_tg @ Jprop[0:6, 0:6]                            # :221-224
    J1_min = J_tg @ Jprop[0:6, 6:15]                           # :252-255
    return _finish(S, z, T_WS, T_GW, C_GW, r_tg, a_tg, J0_min, J1_min, int(state[S_STEPS]))


def evaluate_sync(r_SA, T_WS, T_GW, z, information):
    """GpsErrorSynchronous::EvaluateWithMinimalJacobians (GpsErrorSynchronous.cpp:41-144) of one factor."""
    T_WS, T_GW, r_SA, z = (np.asarray(a, dtype=np.float64) for a in (T_WS, T_GW, r_SA, z))
    S = llt_upper(np.asarray(information, dtype=np.float64).reshape(3, 3))  # :44-47
    C_WS, C_GW = qrot(T_WS[3:]), qrot(T_GW[3:])                # :67-73, as stored
    a = C_WS @ r_SA
    J0_min = np.hstack([-C_GW, C_GW @ cross_mx(a)])            # :96-99
    return _finish(S, z, T_WS, T_GW, C_GW, T_WS[:3], a, J0_min, np.zeros((3, 9)), 0)


def evaluate_batch(ip, r_SA, poses, T_GW, measurement, information, speed_biases=None, t_k=None, t_g=None,
                   sample_begin=None, sample_t=None, sample_ga=None, gw_index=None, state=None, kind=0,
                   use_imu_covariance=True, redo_propagation_always=False):
    """The batch form of okvisgpu_gps_evaluate (the arguments of okvisgpu.gps_batch): dict of stacked
    OUTPUTS; `state` [n, STATE] is updated in place (None: fresh factors, nothing kept)."""
    n = len(poses)
    T_GW = np.asarray(T_GW, dtype=np.float64).reshape(-1, 7)
    information = np.asarray(information, dtype=np.float64).reshape(n, 3, 3)
    rows = []
    for i in range(n):
        G = T_GW[0 if gw_index is None else gw_index[i]]
        if kind == 1:
            rows.append(evaluate_sync(r_SA, poses[i], G, measurement[i], information[i]))
            continue
        a, b = sample_begin[i], sample_begin[i + 1]
        rows.append(evaluate_async(sample_t[a:b], sample_ga[a:b], ip, r_SA, poses[i], speed_biases[i], G, measurement[i],
                                   information[i], t_k[i], t_g[i], None if state is None else state[i],
                                   use_imu_covariance, redo_propagation_always))
    out = {k: np.array([row[k] for row in rows]) for k in OUTPUTS}
    out["steps"] = out["steps"].astype(np.int32)
    return out
