"""The LiDAR pre-processing of ThreadedSlam::processFrame (ThreadedSlam.cpp:785-818) restated in numpy:
the references of tests/test_lidar.py for okvisgpu_lidar_deskew and okvisgpu_voxel_downsample.

Two forms of LidarMotionUndistortion::deskew (LidarMotionUndistortion.cpp:27-85) over the
BatchedLidarPropagator (ViInterface.cpp:635-798):

 (i)  LiteralPropagator / deskew_literal: the reference's own shape. One propagator per scan with its
      persistent IMU iterator, t_end_, the per-call hasStarted and every bias-Jacobian member, driven
      point by point as deskew() drives it.
 (ii) committed_chain / query_state / deskew_scan: the per-query form of include/okvisgpu.h. The chain
      of committed steps is a table that depends on the samples, t_start and the biases only; a query
      takes row k and one step.

They differ only in operations that are exact on finite inputs (terms multiplied by Delta_b = 0, the
blend with r = 1), so they agree to the last bit. Conventions are _imu_propagate's: quaternions
(x, y, z, w), Hamilton product, integer nanosecond stamps through Duration::toSec. Line numbers cite
ViInterface.cpp unless a file is named."""
import numpy as np

from _imu_propagate import cross_mx, delta_q, dur_to_sec, qinv, qmul, qrot, right_jacobian, sinc

G = 9.81  # hard-coded in the reference (:768)


def normalized(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


# ---------------------------------------------------------------------------------------- (i)
class RanOffTheDeque(RuntimeError):
    """The reference's sample loop dereferenced the element past the IMU deque's end."""


class LiteralPropagator:
    """BatchedLidarPropagator (:635-798), member for member."""

    def __init__(self, t_start, ts, ga):
        self.ts = np.asarray(ts, dtype=np.int64)
        self.ga = np.asarray(ga, dtype=np.float64).reshape(-1, 6)
        self.t_start_ = int(t_start)
        self.t_end_ = int(t_start)
        self.it = 0  # imu_iterator_
        z = lambda: np.zeros((3, 3))
        self.Delta_q_ = np.array([0.0, 0.0, 0.0, 1.0])
        self.C_integral_, self.C_doubleintegral_ = z(), z()
        self.acc_integral_, self.acc_doubleintegral_ = np.zeros(3), np.zeros(3)
        self.cross_, self.dalpha_db_g_, self.dv_db_g_, self.dp_db_g_ = z(), z(), z(), z()
        self.omega_S_ = np.zeros(3)
        self.sb_ref_ = np.zeros(9)
        self.Delta_t_ = 0.0
        # the *_interp_ members
        self.Delta_q_interp_ = self.Delta_q_.copy()
        self.C_integral_interp_, self.C_doubleintegral_interp_ = z(), z()
        self.acc_integral_interp_, self.acc_doubleintegral_interp_ = np.zeros(3), np.zeros(3)
        self.cross_interp_, self.dalpha_db_g_interp_, self.dv_db_g_interp_, self.dp_db_g_interp_ = z(), z(), z(), z()
        self.omega_S_interp_ = np.zeros(3)

    def append_to(self, sb, t_end):
        ts, ga, N = self.ts, self.ga, len(self.ts)
        time, end = self.t_end_, int(t_end)  # re-start from the previous end (:643)
        assert ts[0] <= time
        if not ts[-1] >= end:                # :653
            return False
        self.sb_ref_ = np.array(sb, dtype=np.float64)
        has_started = False
        while self.it != N:                  # :659
            k = self.it
            if k + 1 == N:
                raise RanOffTheDeque(f"query {end}: the loop reads sample {N} of {N}")
            om0, ac0 = ga[k, :3].copy(), ga[k, 3:].copy()
            om1, ac1 = ga[k + 1, :3].copy(), ga[k + 1, 3:].copy()
            nexttime = int(ts[k + 1])
            dt = dur_to_sec(nexttime - time)
            if end < nexttime:               # :674-681
                interval = dur_to_sec(nexttime - int(ts[k]))
                nexttime = end
                dt = dur_to_sec(nexttime - time)
                r = dt / interval
                om1 = (1.0 - r) * om0 + r * om1
                ac1 = (1.0 - r) * ac0 + r * ac1
            if dt <= 0.0:                    # :683-685
                self.it += 1
                continue
            if not has_started:              # :686-691
                has_started = True
                r = dt / dur_to_sec(nexttime - int(ts[k]))
                om0 = r * om0 + (1.0 - r) * om1
                ac0 = r * ac0 + (1.0 - r) * ac1
            omega_S_true = 0.5 * (om0 + om1) - sb[3:6]   # :696-715
            theta_half = np.linalg.norm(omega_S_true) * 0.5 * dt
            dq = np.concatenate([sinc(theta_half) * omega_S_true * 0.5 * dt, [np.cos(theta_half)]])
            Delta_q_1 = qmul(self.Delta_q_, dq)
            C, C_1 = qrot(self.Delta_q_), qrot(Delta_q_1)
            acc_S_true = 0.5 * (ac0 + ac1) - sb[6:9]
            C_integral_1 = self.C_integral_ + 0.5 * (C + C_1) * dt
            acc_integral_1 = self.acc_integral_ + 0.5 * (C + C_1) @ acc_S_true * dt
            cross_1 = qrot(qinv(dq)) @ self.cross_ + right_jacobian(omega_S_true * dt) * dt
            acc_S_x = cross_mx(acc_S_true)
            X = C @ acc_S_x @ self.cross_ + C_1 @ acc_S_x @ cross_1
            dv_db_g_1 = self.dv_db_g_ + 0.5 * dt * X
            if nexttime == end:              # :717-739: stop and keep the interpolated values apart
                self.C_doubleintegral_interp_ = self.C_doubleintegral_ + self.C_integral_ * dt + 0.25 * (C + C_1) * dt * dt
                self.acc_doubleintegral_interp_ = (self.acc_doubleintegral_ + self.acc_integral_ * dt
                                                   + 0.25 * (C + C_1) @ acc_S_true * dt * dt)
                self.dalpha_db_g_interp_ = self.dalpha_db_g_ + dt * C_1
                self.dp_db_g_interp_ = self.dp_db_g_ + dt * self.dv_db_g_ + 0.25 * dt * dt * X
                self.omega_S_interp_ = omega_S_true
                self.Delta_q_interp_ = Delta_q_1
                self.C_integral_interp_ = C_integral_1
                self.acc_integral_interp_ = acc_integral_1
                self.cross_interp_ = cross_1
                self.dv_db_g_interp_ = dv_db_g_1
                break
            self.C_doubleintegral_ = self.C_doubleintegral_ + self.C_integral_ * dt + 0.25 * (C + C_1) * dt * dt
            self.acc_doubleintegral_ = (self.acc_doubleintegral_ + self.acc_integral_ * dt
                                        + 0.25 * (C + C_1) @ acc_S_true * dt * dt)
            self.dalpha_db_g_ = self.dalpha_db_g_ + dt * C_1
            self.dp_db_g_ = self.dp_db_g_ + dt * self.dv_db_g_ + 0.25 * dt * dt * X
            self.omega_S_ = omega_S_true
            self.Delta_q_ = Delta_q_1
            self.C_integral_ = C_integral_1
            self.acc_integral_ = acc_integral_1
            self.cross_ = cross_1
            self.dv_db_g_ = dv_db_g_1
            time = nexttime
            self.t_end_ = nexttime
            self.it += 1
        self.Delta_t_ = dur_to_sec(end - self.t_start_)
        return True

    def get_state(self, T_WS_0, sb_0):
        """(T_WS_1 [7], sb_1 [9], omega_S) (:762-798). T_WS_0 is a Transformation: its q is normalised."""
        g_W = np.array([0.0, 0.0, G])
        q0 = normalized(T_WS_0[3:])
        C_WS_0 = qrot(q0)
        Delta_b = sb_0[3:] - self.sb_ref_[3:]
        Dt = self.Delta_t_
        r_est_W = T_WS_0[:3] + sb_0[:3] * Dt - 0.5 * g_W * Dt * Dt
        v_est_W = sb_0[:3] - g_W * Dt
        Dq = qmul(delta_q(-self.dalpha_db_g_interp_ @ Delta_b[:3]), self.Delta_q_interp_)
        r_W_1 = r_est_W + C_WS_0 @ (self.acc_doubleintegral_interp_ + self.dp_db_g_interp_ @ Delta_b[:3]
                                    - self.C_doubleintegral_interp_ @ Delta_b[3:])
        q_WS_1 = qmul(q0, Dq)
        v_W_1 = v_est_W + C_WS_0 @ (self.acc_integral_interp_ + self.dv_db_g_interp_ @ Delta_b[:3]
                                    - self.C_integral_interp_ @ Delta_b[3:])
        sb_1 = np.array(sb_0, dtype=np.float64)
        sb_1[:3] = v_W_1
        return np.concatenate([r_W_1, normalized(q_WS_1)]), sb_1, self.omega_S_interp_.copy()


def transform_point(pose_live, T_WS, T_SL, ray, order="matrix"):
    """T_SW_live.T3x4() * T_WS.T() * T_SL.T() * ray.homogeneous() (LidarMotionUndistortion.cpp:79-81).
    order "matrix": left to right, as Eigen evaluates the product; "vector": right to left."""
    def mat(T):
        M = np.eye(4)
        M[:3, :3] = qrot(normalized(T[3:]))
        M[:3, 3] = T[:3]
        return M
    L = mat(pose_live)
    inv = np.hstack([L[:3, :3].T, (-(L[:3, :3].T @ L[:3, 3]))[:, None]])  # Transformation::inverse
    h = np.concatenate([ray, [1.0]])
    if order == "matrix":
        return ((inv @ mat(T_WS)) @ mat(T_SL)) @ h
    return inv @ (mat(T_WS) @ (mat(T_SL) @ h))


def _zeros():
    return np.zeros(7), np.zeros(3), np.zeros(3)


def deskew_literal(pose0, sb0, t_start, ts, ga, qt, ray, pose_live, T_SL):
    """deskew() (LidarMotionUndistortion.cpp:27-85) for one scan: dict of valid, pose, speed, omega_S,
    point_f64 per point. A point whose appendTo returns false (the reference asserts that there is none,
    :35) is reported invalid."""
    n = len(qt)
    out = {"valid": np.zeros(n, np.uint8), "pose": np.zeros((n, 7)), "speed": np.zeros((n, 3)),
           "omega_S": np.zeros((n, 3)), "point_f64": np.zeros((n, 3))}
    prop = LiteralPropagator(t_start, ts, ga)
    i = 0
    if n and qt[0] == t_start:               # :52-57
        out["valid"][0], out["pose"][0], out["speed"][0] = 1, pose0, sb0[:3]
        out["point_f64"][0] = transform_point(pose_live, pose0, T_SL, ray[0])
        i = 1
    for i in range(i, n):
        if qt[i] < t_start:                  # :61
            continue
        if not prop.append_to(sb0, qt[i]):
            continue
        T1, sb1, w = prop.get_state(pose0, sb0)
        out["valid"][i], out["pose"][i], out["speed"][i], out["omega_S"][i] = 1, T1, sb1[:3], w
        out["point_f64"][i] = transform_point(pose_live, T1, T_SL, ray[i])
    return out


# ---------------------------------------------------------------------------------------- (ii)
def step(ts, ga, k, tau, T, sb, state):
    """step(k, tau, T) of include/okvisgpu.h for ts[k] < T <= ts[k+1], tau < T: the new (Delta_q,
    acc_integral, acc_doubleintegral) and omega_S_true."""
    Dq, a_int, a_dint = state
    om0, ac0 = ga[k, :3].copy(), ga[k, 3:].copy()
    om1, ac1 = ga[k + 1, :3].copy(), ga[k + 1, 3:].copy()
    if T < ts[k + 1]:
        dt = dur_to_sec(T - tau)
        r = dt / dur_to_sec(int(ts[k + 1]) - int(ts[k]))
        om1 = (1.0 - r) * om0 + r * om1
        ac1 = (1.0 - r) * ac0 + r * ac1
    else:
        dt = dur_to_sec(int(ts[k + 1]) - tau)
    r = dt / dur_to_sec(T - int(ts[k]))
    om0 = r * om0 + (1.0 - r) * om1
    ac0 = r * ac0 + (1.0 - r) * ac1
    w_true = 0.5 * (om0 + om1) - sb[3:6]
    theta_half = np.linalg.norm(w_true) * 0.5 * dt
    dq = np.concatenate([sinc(theta_half) * w_true * 0.5 * dt, [np.cos(theta_half)]])
    Dq1 = qmul(Dq, dq)
    C, C1 = qrot(Dq), qrot(Dq1)
    a_true = 0.5 * (ac0 + ac1) - sb[6:9]
    a_int1 = a_int + 0.5 * (C + C1) @ a_true * dt
    a_dint1 = a_dint + a_int * dt + 0.25 * (C + C1) @ a_true * dt * dt
    return (Dq1, a_int1, a_dint1), w_true


def committed_chain(ts, ga, t_start, sb):
    """Row k = the committed state before interval k, k = 0..N-1."""
    state = (np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(3))
    tau = int(t_start)
    rows = []
    for k in range(len(ts)):
        rows.append(state)
        if k + 1 < len(ts) and ts[k + 1] > tau:
            state, _ = step(ts, ga, k, tau, int(ts[k + 1]), sb, state)
            tau = int(ts[k + 1])
    return rows


def query_state(pose0, sb0, t_start, ts, ga, rows, T, g=G):
    """(valid, pose [7], speed [3], omega_S [3]) of one query."""
    T, t_start = int(T), int(t_start)
    if T < t_start or T > ts[-1]:
        return (0,) + _zeros()
    if T == t_start:
        return 1, np.array(pose0, dtype=np.float64), np.array(sb0[:3], dtype=np.float64), np.zeros(3)
    k = int(np.searchsorted(ts, T, side="left")) - 1  # the largest index with ts[k] < T
    (Dq, a_int, a_dint), w = step(ts, ga, k, max(t_start, int(ts[k])), T, sb0, rows[k])
    Dt = dur_to_sec(T - t_start)
    g_W = np.array([0.0, 0.0, g])
    q0 = normalized(pose0[3:])
    C0 = qrot(q0)
    r = (pose0[:3] + sb0[:3] * Dt - 0.5 * g_W * Dt * Dt) + C0 @ a_dint
    v = (sb0[:3] - g_W * Dt) + C0 @ a_int
    return 1, np.concatenate([r, normalized(qmul(q0, Dq))]), v, w


def deskew_scan(pose0, sb0, t_start, ts, ga, qt, ray=None, pose_live=None, T_SL=None, g=G, order="matrix"):
    """One scan in the per-query form: dict of valid, pose, speed, omega_S, n_before and, with rays,
    point_f64 and point."""
    ts = np.asarray(ts, dtype=np.int64)
    ga = np.asarray(ga, dtype=np.float64).reshape(-1, 6)
    n = len(qt)
    out = {"valid": np.zeros(n, np.uint8), "pose": np.zeros((n, 7)), "speed": np.zeros((n, 3)),
           "omega_S": np.zeros((n, 3)), "n_before": int(np.sum(np.asarray(qt) < t_start))}
    if ray is not None:
        out["point_f64"] = np.zeros((n, 3))
    rows = committed_chain(ts, ga, t_start, sb0) if n else []
    for i in range(n):
        out["valid"][i], out["pose"][i], out["speed"][i], out["omega_S"][i] = \
            query_state(pose0, sb0, t_start, ts, ga, rows, qt[i], g)
        if ray is not None and out["valid"][i]:
            out["point_f64"][i] = transform_point(pose_live, out["pose"][i], T_SL, ray[i], order)
    if ray is not None:
        out["point"] = out["point_f64"].astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------- batches
class Scans:
    """A batch of scans in the arrays of okvisgpu_lidar_deskew_batch."""
    FIELDS = ("pose0", "sb0", "t_start", "pose_live", "T_SL")

    def __init__(self, scans):
        """scans: dicts of pose0, sb0, t_start, ts, ga, qt, ray, pose_live, T_SL."""
        self.scans = scans
        self.pose0 = np.array([s["pose0"] for s in scans], dtype=np.float64).reshape(-1, 7)
        self.sb0 = np.array([s["sb0"] for s in scans], dtype=np.float64).reshape(-1, 9)
        self.t_start = np.array([s["t_start"] for s in scans], dtype=np.int64)
        self.pose_live = np.array([s["pose_live"] for s in scans], dtype=np.float64).reshape(-1, 7)
        self.T_SL = np.array([s["T_SL"] for s in scans], dtype=np.float64).reshape(-1, 7)
        self.sample_begin = np.concatenate([[0], np.cumsum([len(s["ts"]) for s in scans])]).astype(np.int32)
        self.query_begin = np.concatenate([[0], np.cumsum([len(s["qt"]) for s in scans])]).astype(np.int32)
        cat = lambda key, dt, cols: (np.concatenate([np.asarray(s[key], dtype=dt).reshape(-1, cols) for s in scans])
                                     if scans else np.zeros((0, cols), dt))
        self.ts = cat("ts", np.int64, 1).reshape(-1)
        self.ga = cat("ga", np.float64, 6)
        self.qt = cat("qt", np.int64, 1).reshape(-1)
        self.ray = cat("ray", np.float64, 3)

    def subset(self, idx):
        return Scans([self.scans[i] for i in idx])

    def batch(self, og, rays=True, **over):
        """The ctypes batch (and what it points into) for og.Context.lidar_deskew."""
        a = dict(pose0=self.pose0, speed_bias0=self.sb0, t_start=self.t_start, sample_begin=self.sample_begin,
                 sample_t=self.ts, sample_ga=self.ga, query_begin=self.query_begin, query_t=self.qt)
        if rays:
            a.update(ray=self.ray, pose_live=self.pose_live, T_SL=self.T_SL)
        a.update(over)
        return og.lidar_deskew_batch(**a)

    def reference(self, g=G):
        """deskew_scan over the batch, concatenated in the layout of okvisgpu_lidar_deskew_result."""
        per = [deskew_scan(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"], s["ray"], s["pose_live"],
                           s["T_SL"], g) for s in self.scans]
        shapes = {"valid": ((0,), np.uint8), "pose": ((0, 7), np.float64), "speed": ((0, 3), np.float64),
                  "omega_S": ((0, 3), np.float64), "point_f64": ((0, 3), np.float64), "point": ((0, 3), np.float32)}
        out = {k: (np.concatenate([p[k] for p in per]) if per else np.zeros(*shapes[k])) for k in shapes}
        out["n_before"] = np.array([p["n_before"] for p in per], dtype=np.int32)
        return out


def random_pose(rng, reach):
    return np.concatenate([rng.uniform(-reach, reach, 3), normalized(rng.normal(size=4))])


def make_scan(rng, N, t_start_offset_ns, qt_offsets_ns, rate_ns=5_000_000, reach=300.0, ray_reach=50.0,
              duplicate_stamp=None):
    """A scan of N samples on a 200 Hz grid with moderate motion. t_start = ts[0] + t_start_offset_ns and
    the queries at ts[0] + qt_offsets_ns (sorted here); duplicate_stamp = k repeats stamp k at k + 1."""
    base = int(rng.integers(1, 1000)) * 1_000_000_000 + int(rng.integers(0, rate_ns))
    ts = base + np.arange(N, dtype=np.int64) * rate_ns
    if duplicate_stamp is not None:
        ts[duplicate_stamp + 1] = ts[duplicate_stamp]
    w = rng.uniform(-1.0, 1.0, 3) + 0.2 * rng.normal(size=(N, 3))
    a = np.array([0.0, 0.0, 9.81]) + rng.uniform(-2, 2, 3) + 0.5 * rng.normal(size=(N, 3))
    qt = np.sort(base + np.asarray(qt_offsets_ns, dtype=np.int64).reshape(-1))
    return {"pose0": random_pose(rng, reach),
            "sb0": np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.1, 0.1, 3)]),
            "t_start": base + int(t_start_offset_ns), "ts": ts, "ga": np.hstack([w, a]), "qt": qt,
            "ray": rng.uniform(-ray_reach, ray_reach, (len(qt), 3)), "pose_live": random_pose(rng, reach),
            "T_SL": random_pose(rng, 0.5)}


# ---------------------------------------------------------------------------------------- voxels
def voxel_of(points, voxel_size):
    """(ok [n], voxel [n, 3] int32): per component the float32 quotient p / float32(voxel_size) truncated
    toward zero (VoxelGridFilter.hpp:54); ok = every quotient finite and inside int32."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = p / np.float32(voxel_size)
        ok = (np.isfinite(q) & (q >= np.float32(-2147483648.0)) & (q < np.float32(2147483648.0))).all(axis=1)
        vox = np.where(ok[:, None], np.trunc(np.where(ok[:, None], q, 0)), 0).astype(np.int32)
    assert q.dtype == np.float32
    return ok, vox


def voxel_downsample(points, voxel_size, use=None):
    """VoxelDownSample<float> (VoxelGridFilter.hpp:46-67) as a mask in input order: keep[i] = 1 for the
    first used point of every voxel. A dict over the input order, as the reference's unordered_map."""
    ok, vox = voxel_of(points, voxel_size)
    keep = np.zeros(len(ok), dtype=np.uint8)
    grid = {}
    for i in range(len(ok)):
        if not ok[i] or (use is not None and not use[i]):
            continue
        key = (int(vox[i, 0]), int(vox[i, 1]), int(vox[i, 2]))
        if key not in grid:
            grid[key] = i
            keep[i] = 1
    return keep


def voxel_downsample_clouds(cloud_begin, points, voxel_sizes, use=None):
    """The batch form of okvisgpu_voxel_downsample: (keep [n_points], n_kept [n_clouds])."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    keep = np.zeros(len(points), dtype=np.uint8)
    n_kept = np.zeros(len(voxel_sizes), dtype=np.int32)
    for c in range(len(voxel_sizes)):
        a, b = cloud_begin[c], cloud_begin[c + 1]
        keep[a:b] = voxel_downsample(points[a:b], voxel_sizes[c], None if use is None else use[a:b])
        n_kept[c] = keep[a:b].sum()
    return keep, n_kept
