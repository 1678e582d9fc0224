"""ImuError::propagation (okvis_ceres/src/ImuError.cpp:537-759) restated in numpy, with the 15x15
covariance and Jacobian: the reference of tests/test_imu_propagate.py for okvisgpu_imu_propagate.

Conventions are the reference's: quaternions (x, y, z, w) with the Hamilton product, times in integer
nanoseconds (okvis::Time differences go through Duration::toSec), the error state ordered
[r, alpha, v, b_g, b_a], matrices row-major. Line numbers cite ImuError.cpp."""
import numpy as np


def dur_to_sec(dns):
    """okvis::Duration::toSec of a signed nanosecond difference (Duration.hpp:107-109)."""
    dns = int(dns)
    sec, nsec = divmod(dns, 1_000_000_000)  # floor division: nsec in [0, 1e9), as the normalised Duration
    return float(sec) + 1e-9 * float(nsec)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def qrot(q):
    """Eigen::QuaternionBase::toRotationMatrix (no normalisation)."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def qinv(q):
    """Eigen Quaternion::inverse (conjugate / squared norm)."""
    return np.array([-q[0], -q[1], -q[2], q[3]]) / np.dot(q, q)


def cross_mx(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def sinc(x):
    """ode::sinc (ode.hpp:34-46): the series below 1e-6."""
    if abs(x) > 1.0e-6:
        return np.sin(x) / x
    x2 = x * x
    return 1.0 - x2 / 6.0 + x2 * x2 / 120.0 - x2 * x2 * x2 / 5040.0


def right_jacobian(p):
    """okvis::kinematics::rightJacobian (Transformation.hpp:55-67)."""
    phi = np.linalg.norm(p)
    X = cross_mx(p)
    if phi < 1.0e-4:
        return np.eye(3) - 0.5 * X + X @ X / 6.0
    return np.eye(3) - (1.0 - np.cos(phi)) / (phi * phi) * X + (phi - np.sin(phi)) / (phi ** 3) * X @ X


def delta_q(a):
    """okvis::kinematics::deltaQ (Transformation.hpp:45-52)."""
    h = 0.5 * np.linalg.norm(a)
    return np.concatenate([sinc(h) * 0.5 * np.asarray(a, float), [np.cos(h)]])


def propagate(ts, ga, ip, T_WS, sb, t_start, t_end, covariance=True):
    """One item. ts [N] int ns, ga [N, 6] (gyro, accelerometer), ip the ImuParams, T_WS [7], sb [9].
    Returns (steps, T_WS_1, sb_1, P, F). steps = -1 (uncovered, :552-553): the rest is None. With 0
    steps the pose and speed/bias are returned as given (bit for bit), F = I, P = 0. covariance=False
    skips the covariance recursion (as a NULL covariance does in the reference): P is None."""
    ts = np.asarray(ts, dtype=np.int64)
    ga = np.asarray(ga, dtype=np.float64).reshape(-1, 6)
    T_WS = np.asarray(T_WS, dtype=np.float64)
    sb = np.asarray(sb, dtype=np.float64)
    N = len(ts)
    assert N > 0 and ts[0] <= t_start, "ImuError.cpp:550"
    if not ts[-1] >= t_end:
        return -1, None, None, None, None
    time = int(t_start)
    Dq = np.array([0.0, 0.0, 0.0, 1.0])
    C_int, C_dint = np.zeros((3, 3)), np.zeros((3, 3))
    a_int, a_dint = np.zeros(3), np.zeros(3)
    cross = np.zeros((3, 3))
    dalpha_db_g, dv_db_g, dp_db_g = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3))
    P = np.zeros((15, 15))
    Dt = 0.0
    started = False
    steps = 0
    for k in range(N):
        om0, ac0 = ga[k, :3].copy(), ga[k, 3:].copy()
        # (past the end the reference reads nothing it uses: such a step has dt <= 0)
        om1, ac1 = (ga[k + 1, :3].copy(), ga[k + 1, 3:].copy()) if k + 1 < N else (om0.copy(), ac0.copy())
        nexttime = int(t_end) if k + 1 == N else int(ts[k + 1])
        dt = dur_to_sec(nexttime - time)
        if t_end < nexttime:                                   # :598-605
            interval = dur_to_sec(nexttime - int(ts[k]))
            nexttime = int(t_end)
            dt = dur_to_sec(nexttime - time)
            r = dt / interval
            om1 = (1.0 - r) * om0 + r * om1
            ac1 = (1.0 - r) * ac0 + r * ac1
        if dt <= 0.0:                                          # :607-609
            continue
        Dt += dt
        if not started:                                        # :612-617
            started = True
            r = dt / dur_to_sec(nexttime - int(ts[k]))
            om0 = r * om0 + (1.0 - r) * om1
            ac0 = r * ac0 + (1.0 - r) * ac1
        sigma_g_c, sigma_a_c = ip.sigma_g_c, ip.sigma_a_c      # :619-640
        if max(np.abs(om0).max(), np.abs(om1).max()) > ip.g_max:
            sigma_g_c *= 100
        if max(np.abs(ac0).max(), np.abs(ac1).max()) > ip.a_max:
            sigma_a_c *= 100
        w_true = 0.5 * (om0 + om1) - sb[3:6]                   # :644-668
        theta_half = np.linalg.norm(w_true) * 0.5 * dt
        dq = np.concatenate([sinc(theta_half) * w_true * 0.5 * dt, [np.cos(theta_half)]])
        Dq1 = qmul(Dq, dq)
        C, C1 = qrot(Dq), qrot(Dq1)
        a_true = 0.5 * (ac0 + ac1) - sb[6:9]
        CC = C + C1
        C_int1 = C_int + 0.5 * CC * dt
        a_int1 = a_int + 0.5 * (CC @ a_true) * dt
        dp_step = a_int * dt + 0.25 * (CC @ a_true) * dt * dt
        C_dint = C_dint + C_int * dt + 0.25 * CC * dt * dt
        a_dint = a_dint + dp_step
        dalpha_db_g = dalpha_db_g + dt * C1
        cross1 = qrot(qinv(dq)) @ cross + right_jacobian(w_true * dt) * dt
        ax = cross_mx(a_true)
        X = C @ ax @ cross + C1 @ ax @ cross1
        dv_db_g1 = dv_db_g + 0.5 * dt * X
        dp_db_g_step = dt * dv_db_g + 0.25 * dt * dt * X
        dp_db_g = dp_db_g + dp_db_g_step
        if covariance:
            F = np.eye(15)                                     # :672-682
            F[0:3, 3:6] = -cross_mx(dp_step)
            F[0:3, 6:9] = np.eye(3) * dt
            F[0:3, 9:12] = dp_db_g_step
            F[0:3, 12:15] = -C_int * dt + 0.25 * CC * dt * dt
            F[3:6, 9:12] = -dt * C1
            F[6:9, 3:6] = -cross_mx(0.5 * (CC @ a_true) * dt)
            F[6:9, 9:12] = 0.5 * dt * X
            F[6:9, 12:15] = -0.5 * CC * dt
            P = F @ P @ F.T                                    # :684-707
            s2_dalpha = dt * sigma_g_c * sigma_g_c
            s2_v = dt * sigma_a_c * ip.sigma_a_c
            s2_p = 0.5 * dt * dt * s2_v
            s2_bg = dt * ip.sigma_gw_c * ip.sigma_gw_c
            s2_ba = dt * ip.sigma_aw_c * ip.sigma_aw_c
            P[np.arange(15), np.arange(15)] += np.repeat([s2_p, s2_dalpha, s2_v, s2_bg, s2_ba], 3)
        Dq, C_int, a_int, cross, dv_db_g, time = Dq1, C_int1, a_int1, cross1, dv_db_g1, nexttime
        steps += 1
        if nexttime == t_end:                                  # :720-721
            break
    if steps == 0:
        return 0, T_WS.copy(), sb.copy(), np.zeros((15, 15)) if covariance else None, np.eye(15)
    q0 = T_WS[3:] / np.linalg.norm(T_WS[3:])
    C0 = qrot(q0)
    g_W = np.array([0.0, 0.0, ip.g])                           # :726-732
    r1 = T_WS[:3] + sb[:3] * Dt + C0 @ a_dint - 0.5 * g_W * Dt * Dt
    q1 = qmul(q0, Dq)
    q1 = q1 / np.linalg.norm(q1)                               # Transformation::set normalises
    sb1 = sb.copy()
    sb1[:3] += C0 @ a_int - g_W * Dt
    J = np.eye(15)                                             # :735-746
    J[0:3, 3:6] = -cross_mx(C0 @ a_dint)
    J[0:3, 6:9] = np.eye(3) * Dt
    J[0:3, 9:12] = C0 @ dp_db_g
    J[0:3, 12:15] = -C0 @ C_dint
    J[3:6, 9:12] = -C0 @ dalpha_db_g
    J[6:9, 3:6] = -cross_mx(C0 @ a_int)
    J[6:9, 9:12] = C0 @ dv_db_g
    J[6:9, 12:15] = -C0 @ C_int
    T = np.eye(15)                                             # :749-757
    T[0:3, 0:3] = T[3:6, 3:6] = T[6:9, 6:9] = C0
    return steps, np.concatenate([r1, q1]), sb1, T @ P @ T.T if covariance else None, J


def propagate_batch(ip, poses, sbs, t_start, t_end, sample_begin, sample_t, sample_ga):
    """The batch form of okvisgpu_imu_propagate: (steps [n], poses [n, 7], sbs [n, 9], P [n, 15, 15],
    J [n, 15, 15]); rows of uncovered items (steps -1) hold the inputs and NaN matrices."""
    n = len(t_start)
    poses, sbs = np.array(poses, dtype=np.float64), np.array(sbs, dtype=np.float64)
    steps = np.zeros(n, np.int32)
    P, J = np.full((n, 15, 15), np.nan), np.full((n, 15, 15), np.nan)
    for i in range(n):
        a, b = sample_begin[i], sample_begin[i + 1]
        s, T1, sb1, Pi, Ji = propagate(sample_t[a:b], sample_ga[a:b], ip, poses[i], sbs[i], t_start[i], t_end[i])
        steps[i] = s
        if s >= 0:
            poses[i], sbs[i], P[i], J[i] = T1, sb1, Pi, Ji
    return steps, poses, sbs, P, J


def box_minus(T1, sb1, T0, sb0):
    """The 15-vector error state between two (pose, speed/bias) pairs: delta r additive, the
    orientation as 2 vec(q1 (x) q0^-1), then speed and biases."""
    dq = qmul(T1[3:], qinv(T0[3:]))
    if dq[3] < 0:
        dq = -dq
    return np.concatenate([T1[:3] - T0[:3], 2.0 * dq[:3], sb1 - sb0])


def box_plus(T, sb, d):
    """(pose, speed/bias) perturbed by the error state d: r + dr, q <- deltaQ(dalpha) (x) q."""
    q = qmul(delta_q(d[3:6]), T[3:])
    return np.concatenate([T[:3] + d[:3], q]), sb + d[6:15]


def random_items(rng, n, lo=2, hi=45, rate_ns=5_000_000):
    """n random items of lo..hi samples at 200 Hz: stamps on the grid, t_start inside the first
    interval, t_end inside the last (or on a sample), moderate rotation rates and accelerations.
    Returns (poses, sbs, t_start, t_end, sample_begin, sample_t, sample_ga)."""
    poses, sbs, t0s, t1s, begin, ts, ga = [], [], [], [], [0], [], []
    for _ in range(n):
        N = int(rng.integers(lo, hi + 1))
        base = int(rng.integers(1, 1000)) * 1_000_000_000 + int(rng.integers(0, rate_ns))
        t = base + np.arange(N, dtype=np.int64) * rate_ns
        t_start = int(t[0] + rng.integers(0, rate_ns))
        t_end = int(t[-1] - rng.integers(0, rate_ns)) if rng.random() < 0.7 else int(t[-1])
        if N == 2:
            t_start, t_end = min(t_start, t_end), max(t_start, t_end)
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        poses.append(np.concatenate([rng.uniform(-5, 5, 3), q]))
        sbs.append(np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.1, 0.1, 3)]))
        w = rng.uniform(-1.0, 1.0, 3) + 0.2 * rng.normal(size=(N, 3))
        a = np.array([0.0, 0.0, 9.81]) + rng.uniform(-2, 2, 3) + 0.5 * rng.normal(size=(N, 3))
        t0s.append(t_start)
        t1s.append(t_end)
        ts.append(t)
        ga.append(np.hstack([w, a]))
        begin.append(begin[-1] + N)
    return (np.array(poses), np.array(sbs), np.array(t0s, np.int64), np.array(t1s, np.int64),
            np.array(begin, np.int32), np.concatenate(ts), np.concatenate(ga))
