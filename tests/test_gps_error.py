"""okvisgpu_gps_evaluate: GpsErrorAsynchronous (GpsErrorAsynchronous.cpp:98-507), the factor
ViGraph::addGpsMeasurement (ViGraph.cpp:973-1006) adds for every GPS fix, and GpsErrorSynchronous
(GpsErrorSynchronous.cpp:41-144), for a batch of factors on the device.

CPU: the numpy restatement (tests/_gps_error.py) against the reference's own finite-difference
property (TestGpsError.cpp:254-332), against the pre-integration of the solver's ImuError (the oracle),
against a closed form, and through the redo logic. GPU: okvisgpu_gps_evaluate against the restatement
at the functor-level contract: r, error, sqrt_info and every Jacobian within 1e-12
max(1, |ref|), P_delta within 1e-12 max|P_ref| per factor, counters, flags and steps equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _gps_error as ge
import _imu_propagate as ipr
from _gps import pose_plus
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
NS = 5_000_000  # 200 Hz
R_SA = np.array([0.05, -0.02, 0.1])
# the bound of the ImuError tie (test 2): 100 x the largest deviation measured on the CPU
# (test_tie_to_the_solvers_imu_error's docstring)
TIE_MEASURED = 4.5e-16
TIE_BOUND = 100 * TIE_MEASURED


def _params(og):
    ip = og.ImuParams()
    ip.a_max, ip.g_max = 176.0, 7.8
    ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c = 12.0e-4, 8.0e-3, 4.0e-6, 4.0e-5
    ip.g = 9.81007
    return ip


def _unit(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _gps_side(rng, poses, sbs, t_k, t_g, n_gw=2):
    """The GPS half of a batch for given states: T_GW blocks, gw_index, fixes near the prediction with
    sigmas in 0.05 .. 0.5 m (information = R diag(sigma^-2) R^T, condition <= 100)."""
    n = len(poses)
    T_GW = np.array([np.concatenate([rng.normal(0.0, 2.0, 3), _unit(rng)]) for _ in range(n_gw)])
    gw = rng.integers(0, n_gw, n).astype(np.int32)
    z, info = np.zeros((n, 3)), np.zeros((n, 3, 3))
    for i in range(n):
        Dt = ipr.dur_to_sec(int(t_g[i]) - int(t_k[i]))
        G = T_GW[gw[i]]
        z[i] = ipr.qrot(G[3:]) @ (poses[i, :3] + sbs[i, :3] * Dt + ipr.qrot(poses[i, 3:]) @ R_SA) + G[:3] + rng.normal(0.0, 0.3, 3)
        R = ipr.qrot(_unit(rng))
        A = R @ np.diag(rng.uniform(0.05, 0.5, 3) ** -2.0) @ R.T
        info[i] = 0.5 * (A + A.T)
    return T_GW, gw, z, info


def _batch(og, rng, items):
    """[(pose, sb, t_k, t_g, ts, ga)] -> (args, kw) for og.gps_batch and ge.evaluate_batch."""
    poses = np.ascontiguousarray([it[0] for it in items], dtype=np.float64)
    sbs = np.ascontiguousarray([it[1] for it in items], dtype=np.float64)
    t_k = np.array([it[2] for it in items], np.int64)
    t_g = np.array([it[3] for it in items], np.int64)
    begin = np.concatenate([[0], np.cumsum([len(it[4]) for it in items])]).astype(np.int32)
    ts = np.concatenate([np.asarray(it[4], np.int64) for it in items])
    ga = np.concatenate([np.asarray(it[5], np.float64).reshape(-1, 6) for it in items])
    T_GW, gw, z, info = _gps_side(rng, poses, sbs, t_k, t_g)
    return ((_params(og), R_SA, poses, T_GW, z, info),
            dict(speed_biases=sbs, t_k=t_k, t_g=t_g, sample_begin=begin, sample_t=ts, sample_ga=ga, gw_index=gw))


def _random_batch(og, seed, n, lo=2, hi=45):
    rng = np.random.default_rng(seed)
    poses, sbs, t0, t1, begin, ts, ga = ipr.random_items(rng, n, lo, hi)
    T_GW, gw, z, info = _gps_side(rng, poses, sbs, t0, t1)
    return ((_params(og), R_SA, poses, T_GW, z, info),
            dict(speed_biases=sbs, t_k=t0, t_g=t1, sample_begin=begin, sample_t=ts, sample_ga=ga, gw_index=gw))


def _sub(args, kw, n):
    """The first n factors of a batch."""
    ip, r_SA, poses, T_GW, z, info = args
    b = kw["sample_begin"]
    return ((ip, r_SA, poses[:n], T_GW, z[:n], info[:n]),
            dict(speed_biases=kw["speed_biases"][:n], t_k=kw["t_k"][:n], t_g=kw["t_g"][:n], sample_begin=b[:n + 1],
                 sample_t=kw["sample_t"][:b[n]], sample_ga=kw["sample_ga"][:b[n]], gw_index=kw["gw_index"][:n]))


def _moved(kw, d_bg, d_ba=0.0, rows=None):
    """kw with the biases of `rows` (default: all) moved."""
    sbs = kw["speed_biases"].copy()
    rows = slice(None) if rows is None else rows
    sbs[rows, 3:6] += d_bg
    sbs[rows, 6:9] += d_ba
    return dict(kw, speed_biases=sbs)


def _crafted(og):
    """The ragged batch of test 6 and the index of each item. f and g carry a state integrated at a bias
    1e-3 rad/s away (49 and 50 samples: a redo, and the first-order path with the flag kept); they share
    a wavefront with the 201-sample h and the 2-sample i."""
    ip = _params(og)
    rng = np.random.default_rng(611)

    def motion(N, t0=3_000_000_000):
        t = t0 + np.arange(N, dtype=np.int64) * NS
        w = rng.uniform(-1, 1, 3) + 0.2 * rng.normal(size=(N, 3))
        a = np.array([0.0, 0.0, 9.81]) + rng.uniform(-2, 2, 3) + 0.5 * rng.normal(size=(N, 3))
        pose = np.concatenate([rng.uniform(-5, 5, 3), _unit(rng)])
        sb = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.1, 0.1, 3)])
        return pose, sb, t, np.hstack([w, a])

    items = {}
    pose, sb, t, ga = motion(2)
    items["a"] = (pose, sb, int(t[0]), int(t[1]), t, ga)                       # both stamps on the samples
    pose, sb, t, ga = motion(7)
    items["b"] = (pose, sb, int(t[0] + 1_234_567), int(t[6] - 777_777), t, ga)  # interpolation at both ends
    pose, sb, t, ga = motion(4)
    items["c"] = (pose, sb, int(t[1] + 1_000_000), int(t[1] + 1_000_000), t, ga)  # t_g == t_k
    pose, sb, t, ga = motion(9)
    items["d"] = (pose, sb, int(t[0] + 2_000_000), int(t[8]), t, ga)            # the last sample exactly at t_g
    pose, sb, t, ga = motion(49)
    items["f"] = (pose, sb, int(t[0] + 1_000_000), int(t[48] - 1_000_000), t, ga)
    pose, sb, t, ga = motion(50)
    items["g"] = (pose, sb, int(t[0] + 1_000_000), int(t[49] - 1_000_000), t, ga)
    pose, sb, t, ga = motion(201)
    items["h"] = (pose, sb, int(t[0]), int(t[200]), t, ga)
    pose, sb, t, ga = motion(2)
    items["i"] = (pose, sb, int(t[0] + 1_000_000), int(t[1] - 1_000_000), t, ga)
    pose, sb, t, ga = motion(8)
    ga[3, 1] = 2.0 * ip.g_max
    ga[4, 5] = -1.5 * ip.a_max
    items["e"] = (pose, sb, int(t[0] + 1_000_000), int(t[7] - 1_000_000), t, ga)  # saturation
    index = {k: i for i, k in enumerate(items)}
    args, kw = _batch(og, rng, list(items.values()))
    state = np.zeros((len(items), ge.STATE))
    rows = [index["f"], index["g"]]
    for i in rows:  # integrated once at the original bias
        one_args, one_kw = _sub(args, kw, i + 1)
        s = state[:i + 1].copy()
        ge.evaluate_batch(*one_args, **one_kw, state=s)
        state[i] = s[i]
    return args, _moved(kw, 1e-3, rows=rows), state, index


@pytest.fixture(scope="module")
def crafted(og):
    args, kw, state, index = _crafted(og)
    ref_state = state.copy()
    return args, kw, state, index, ge.evaluate_batch(*args, **kw, state=ref_state), ref_state


@pytest.fixture(scope="module")
def random257(og):
    args, kw = _random_batch(og, 257, 257)
    ref_state = np.zeros((257, ge.STATE))
    return args, kw, ge.evaluate_batch(*args, **kw, state=ref_state), ref_state


# ------------------------------------------------------------------------------------------ CPU
def _reference_scenario(og, seed, duration=0.2):
    """The scenario of TestGpsError.cpp:40-232: a circle of radius 5 m at omega = (0.2, 0.2, 0.2) rad/s, a
    1 kHz IMU with the test's noise, frames at 80 Hz and fixes at 100 Hz (t_g - t_k <= 10 ms), r_SA =
    (0.2, 0.3, 0.1), gps_std = 0.02 m, every state disturbed as there. Every fix gives a factor on the latest
    frame with all samples so far, as the test's growing deque does. Returns (ip, r_SA, T_GW, factors)."""
    rng = np.random.default_rng(seed)
    rand3 = lambda: rng.uniform(-1.0, 1.0, 3)  # Eigen's Vector3d::Random()
    ip = og.ImuParams()
    ip.a_max = ip.g_max = 1000.0
    ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c, ip.g = 6.0e-4, 2.0e-3, 3.0e-6, 2.0e-5, 9.81
    r_SA, gps_std, dt = np.array([0.2, 0.3, 0.1]), 0.02, 1e-3

    def random_T(reach, angle):  # Transformation::setRandom
        axis = rand3()
        return np.concatenate([reach * rand3(), ipr.delta_q(angle * rng.uniform(-1.0, 1.0) * axis / np.linalg.norm(axis))])

    def compose(A, B):
        return np.concatenate([A[:3] + ipr.qrot(A[3:]) @ B[:3], ipr.qmul(A[3:], B[3:])])

    omega = np.array([0.2, 0.2, 0.2])
    T_GW_true = random_T(10.0, np.pi)
    T_GW = compose(T_GW_true, random_T(2.0, np.pi / 2))
    r, q = np.array([0.0, 5.0, 1.0]), np.array([0.0, 0.0, 0.0, 1.0])
    ts, ga, factors = [], [], []
    frames = fixes = 0
    frame = None
    for i in range(int(duration * 1000)):
        time = i / 1000.0
        v = np.cross(omega, r)
        a_W = np.cross(omega, v)
        r = r + v * dt
        q = ipr.qmul(q, ipr.delta_q(omega * dt))
        C = ipr.qrot(q)
        ts.append(i * 1_000_000)
        ga.append(np.concatenate([omega + ip.sigma_g_c / np.sqrt(dt) * rand3(),
                                  C.T @ (a_W + np.array([0.0, 0.0, ip.g])) + ip.sigma_a_c / np.sqrt(dt) * rand3()]))
        if time > frames / 80.0:
            sb = np.concatenate([v + 0.1 * rand3(), 2e-3 * rand3(), 1e-2 * rand3()])
            frame = (compose(np.concatenate([r, q]), random_T(1.0, np.pi)), sb, ts[-1])
            frames += 1
        if time > fixes / 100.0:
            z = ipr.qrot(T_GW_true[3:]) @ (r + C @ r_SA) + T_GW_true[:3] + gps_std * rand3()
            factors.append((frame[0], frame[1], frame[2], ts[-1], np.array(ts, np.int64), np.array(ga), z,
                            np.eye(3) / gps_std ** 2))
            fixes += 1
    return ip, r_SA, T_GW, factors


@pytest.mark.parametrize("use_cov", [0, 1])
def test_jacobians_against_central_differences(og, use_cov):
    """1. The reference's own property (TestGpsError.cpp:254-332) in its own scenario: the functor is
    evaluated, then central differences with dx = 1e-6 on each of the three blocks, taken through the
    manifold on the same functor (the biases move by less than the threshold, so the first-order path),
    lifted with minusJacobian where the block is a pose: ||J_num - J|| < 1e-3 (Frobenius, as Eigen's norm;
    measured 8.9e-4 over the 20 factors, with and without the IMU covariance).
    (The analytic bias-gyro columns hold to first order in the rotation over t_g - t_k, which is why the
    property belongs to short intervals: the 10 ms of the reference's test, not a 200 ms frame gap.)"""
    from _gps import lift
    ip, r_SA, G, factors = _reference_scenario(og, 254)
    dx, worst = 1e-6, 0.0
    assert len(factors) == 20 and max(f[3] - f[2] for f in factors) == 10_000_000
    for pose, sb, t_k, t_g, ts, ga, z, info in factors:
        state = np.zeros(ge.STATE)

        def r_at(T, sbx, Gx):
            return ge.evaluate_async(ts, ga, ip, r_SA, T, sbx, Gx, z, info, t_k, t_g, state.copy(), bool(use_cov))["r"]

        out = ge.evaluate_async(ts, ga, ip, r_SA, pose, sb, G, z, info, t_k, t_g, state, bool(use_cov))
        assert state[ge.S_COUNTER] == 1
        J0, J1, J2 = np.zeros((3, 6)), np.zeros((3, 9)), np.zeros((3, 6))
        for j in range(6):
            d = np.zeros(6)
            d[j] = dx
            J0[:, j] = (r_at(pose_plus(pose, d), sb, G) - r_at(pose_plus(pose, -d), sb, G)) / (2 * dx)
            J2[:, j] = (r_at(pose, sb, pose_plus(G, d)) - r_at(pose, sb, pose_plus(G, -d))) / (2 * dx)
        for j in range(9):
            d = np.zeros(9)
            d[j] = dx
            J1[:, j] = (r_at(pose, sb + d, G) - r_at(pose, sb - d, G)) / (2 * dx)
        errs = (np.linalg.norm(J0 @ lift(pose) - out["J_pose_ambient"]), np.linalg.norm(J1 - out["J_speed_bias"]),
                np.linalg.norm(J2 @ lift(G) - out["J_T_GW_ambient"]))
        worst = max(worst, *errs)
    print(f"central differences (use_imu_covariance {use_cov}): worst ||J_num - J|| = {worst:.3e}")
    assert worst < 1e-3, worst


def _tie_deviation(og, oracle):
    """Largest deviation between the restatement's pre-integration and what the oracle's ImuError leaves
    in imu_state, over the 9 factors of an S10 window: increments [2..56] relative to max(1, |ref|),
    P_delta relative to max|P_ref|."""
    w = og.SynthWindow(10, 500, 4000, seed=77)
    p = w.problem
    n = p.n_imu
    assert not w.imu_state().any()
    begin = np.ctypeslib.as_array(p.imu_sample_begin, shape=(n + 1,))
    ts = np.ctypeslib.as_array(p.imu_sample_t_ns, shape=(begin[-1],))
    ga = np.ctypeslib.as_array(p.imu_sample_gyr_acc, shape=(begin[-1], 6))
    t0 = np.ctypeslib.as_array(p.imu_t0_ns, shape=(n,))
    t1 = np.ctypeslib.as_array(p.imu_t1_ns, shape=(n,))
    blocks = np.ctypeslib.as_array(p.imu_blocks, shape=(n, 4))
    sbs = w.speed_biases().copy()
    oracle.eval_imu(w.problem_ptr(), n)
    imu_state = w.imu_state()
    worst_inc = worst_P = 0.0
    for f in range(n):
        state = np.zeros(ge.STATE)
        s = slice(begin[f], begin[f + 1])
        steps = ge.redo_preintegration(state, ts[s], ga[s], p.imu_params, sbs[blocks[f, 1]], int(t0[f]), int(t1[f]), True)
        assert steps > 0 and steps == int(imu_state[f, 291])
        a, b = state[2:57], imu_state[f, 2:57]
        worst_inc = max(worst_inc, (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
        Pa, Pb = state[ge.S_P:], imu_state[f, 301:526]
        worst_P = max(worst_P, np.abs(Pa - Pb).max() / np.abs(Pb).max())
    return worst_inc, worst_P


def test_tie_to_the_solvers_imu_error(og, oracle):
    """2. Same samples, t0 = t_k, t1 = t_g, same biases: the state entries [2..56] and P_delta agree with
    what the oracle's ImuError leaves in imu_state ([2..56], [301..525]); neither side is the code under
    test. Measured on the CPU (seed 77, the 9 factors of an S10 window): increments 4.44e-16 relative to
    max(1, |ref|), P_delta 5.3e-18 relative to max|P_ref|; asserted 100 x the larger, 4.5e-14."""
    worst_inc, worst_P = _tie_deviation(og, oracle)
    print(f"ImuError tie (CPU): increments {worst_inc:.3e}, P_delta {worst_P:.3e}")
    assert worst_inc <= TIE_BOUND and worst_P <= TIE_BOUND


def test_stationary_closed_form(og):
    """3. A stationary IMU (gyro = b_g, accelerometer = C_WS^T g_W + b_a): T_WS(t_g) = (r + v Dt, q), so the
    residual is kind 1's at that pose; and kind 0 with t_g = t_k equals kind 1 at the pose itself. Both
    without the IMU covariance, within 1e-12."""
    ip = _params(og)
    rng = np.random.default_rng(3)
    worst = 0.0
    for N in (2, 13, 40):
        pose = np.concatenate([rng.uniform(-5, 5, 3), _unit(rng)])
        sb = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.1, 0.1, 3)])
        G = np.concatenate([rng.normal(0.0, 2.0, 3), _unit(rng)])
        t = 5_000_000_000 + np.arange(N, dtype=np.int64) * NS
        ga = np.tile(np.concatenate([sb[3:6], ipr.qrot(pose[3:]).T @ np.array([0.0, 0.0, ip.g]) + sb[6:9]]), (N, 1))
        t_k, t_g = int(t[0] + 1_000_000), int(t[-1] - 1_500_000)
        Dt = ipr.dur_to_sec(t_g - t_k)
        z = rng.normal(0.0, 3.0, 3)
        info = np.diag(rng.uniform(0.05, 0.5, 3) ** -2.0)
        out = ge.evaluate_async(t, ga, ip, R_SA, pose, sb, G, z, info, t_k, t_g, None, False)
        later = np.concatenate([pose[:3] + sb[:3] * Dt, pose[3:]])
        ref = ge.evaluate_sync(R_SA, later, G, z, info)
        for k in ("r", "error", "sqrt_info"):
            worst = max(worst, np.abs(out[k] - ref[k]).max())
        same = ge.evaluate_async(t, ga, ip, R_SA, pose, sb, G, z, info, t_k, t_k, None, False)
        ref = ge.evaluate_sync(R_SA, pose, G, z, info)
        assert same["steps"] == 0
        for k in ge.OUTPUTS[:-1]:
            worst = max(worst, np.abs(same[k] - ref[k]).max())
    print(f"closed form: worst {worst:.3e}")
    assert worst <= 1e-12, worst


def test_redo_logic(og):
    """4. One functor through the sequence of :134-142."""
    args, kw = _random_batch(og, 4, 1, 49, 49)
    ip, r_SA, poses, T_GW, z, info = args
    ts, ga, sb = kw["sample_t"], kw["sample_ga"], kw["speed_biases"][0]
    state = np.zeros(ge.STATE)

    def run(sb_now, ts=ts, ga=ga, always=False):
        return ge.evaluate_async(ts, ga, ip, r_SA, poses[0], sb_now, T_GW[0], z[0], info[0], kw["t_k"][0], kw["t_g"][0], state,
                                 True, always)

    first = run(sb)                                     # fresh: redo
    assert state[ge.S_COUNTER] == 1 and state[ge.S_FLAG] == 0 and first["steps"] > 0
    assert np.array_equal(state[ge.S_REF:ge.S_REF + 9], sb)
    frozen = state.copy()
    small = sb.copy()
    small[3] += 1e-4
    out = run(small)                                    # below the threshold: the first-order path
    assert state[ge.S_COUNTER] == 1 and state[ge.S_FLAG] == 0 and np.array_equal(state, frozen)
    assert np.abs(out["r"] - first["r"]).max() > 0
    large = sb.copy()
    large[3] += 1e-3
    run(large)                                          # above it with 49 samples: redo
    assert state[ge.S_COUNTER] == 2 and state[ge.S_FLAG] == 0 and np.array_equal(state[ge.S_REF:ge.S_REF + 9], large)
    ts50, ga50 = np.concatenate([ts, [ts[-1] + NS]]), np.vstack([ga, ga[-1:]])
    frozen = state.copy()
    run(sb, ts50, ga50)                                 # the same with 50 samples: no redo, the flag stays
    assert state[ge.S_COUNTER] == 2 and state[ge.S_FLAG] == 1
    frozen[ge.S_FLAG] = 1
    assert np.array_equal(state, frozen)
    run(large, ts50, ga50)                              # the bias back on ref: the flag still stands
    assert state[ge.S_COUNTER] == 2 and state[ge.S_FLAG] == 1
    run(sb, ts50, ga50, always=True)                    # redo_propagation_always: redo
    assert state[ge.S_COUNTER] == 3 and state[ge.S_FLAG] == 0 and np.array_equal(state[ge.S_REF:ge.S_REF + 9], sb)


def test_symbol_and_null_context(og):
    """5. The entry point is declared, exported and refuses a NULL context."""
    assert "okvisgpu_gps_evaluate" in og.EXPORTED_SYMBOLS
    lib = og.lib()
    assert hasattr(lib, "okvisgpu_gps_evaluate")
    args, kw = _random_batch(og, 5, 3)
    b, keep = og.gps_batch(*args, **kw)
    r = og.GpsResult()
    assert lib.okvisgpu_gps_evaluate(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
    assert og.GPS_STATE_DOUBLES == ge.STATE


def test_struct_layout(og, tmp_path):
    """GpsBatch and GpsResult mirror the header."""
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    tb, tr = "okvisgpu_gps_batch", "okvisgpu_gps_result"
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {",
           f'  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof({tb}), offsetof({tb}, r_SA), offsetof({tb}, T_GW), '
           f'offsetof({tb}, state), sizeof({tr}), offsetof({tr}, steps), OKVISGPU_GPS_STATE_DOUBLES);',
           "  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(og.GpsBatch), og.GpsBatch.r_SA.offset, og.GpsBatch.T_GW.offset, og.GpsBatch.state.offset,
                   C.sizeof(og.GpsResult), og.GpsResult.steps.offset, og.GPS_STATE_DOUBLES]


# ------------------------------------------------------------------------------------------ GPU
def _compare(parity, name, got, ref, state=None, ref_state=None):
    """GPU outputs (and state) against the restatement's, at the contract."""
    assert np.array_equal(got["steps"], ref["steps"])
    for k in ge.OUTPUTS[:-1]:
        parity(f"gps_evaluate/{name}/{k}", (np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max(), 1e-12)
    if state is None:
        return
    for col in (ge.S_COUNTER, ge.S_FLAG, ge.S_STEPS):
        assert np.array_equal(state[:, col], ref_state[:, col]), col
    a, b = state[:, 2:66], ref_state[:, 2:66]
    parity(f"gps_evaluate/{name}/increments", (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max(), 1e-12)
    worst = 0.0
    for i in range(len(state)):
        Pa, Pb = state[i, ge.S_P:], ref_state[i, ge.S_P:]
        m = np.abs(Pb).max()
        if m == 0.0:
            assert not Pa.any(), i
        else:
            worst = max(worst, np.abs(Pa - Pb).max() / m)
    parity(f"gps_evaluate/{name}/P_delta", worst, 1e-12)


def _run(og, ctx, args, kw, state=None, **flags):
    b, keep = og.gps_batch(*args, **kw, state=state, **flags)
    return ctx.gps_evaluate(b, fill=np.nan)


def _same_bits(a, b, n=None):
    for k in ge.OUTPUTS:
        assert a[k].tobytes() == (b[k] if n is None else b[k][:n]).tobytes(), k


@pytest.mark.gpu
def test_gpu_crafted_batch(og, gpu_ctx, crafted, parity):
    """6. The ragged batch of crafted items, on the state that makes f re-integrate and g not."""
    args, kw, state0, index, ref, ref_state = crafted
    state = state0.copy()
    got = _run(og, gpu_ctx, args, kw, state)
    _compare(parity, "crafted", got, ref, state, ref_state)
    for v in got.values():
        assert not np.isnan(np.asarray(v, dtype=np.float64)).any()
    steps = {k: int(got["steps"][i]) for k, i in index.items()}
    assert (steps["a"], steps["c"], steps["d"], steps["h"], steps["i"]) == (1, 0, 8, 200, 1)
    f, g, c = index["f"], index["g"], index["c"]
    assert state[f, ge.S_COUNTER] == 2 and state[f, ge.S_FLAG] == 0
    assert state[g, ge.S_COUNTER] == 1 and state[g, ge.S_FLAG] == 1
    keep = np.ones(ge.STATE, bool)
    keep[ge.S_FLAG] = False
    assert state[g, keep].tobytes() == state0[g, keep].tobytes()
    assert state[c, ge.S_COUNTER] == 1 and np.array_equal(state[c, 2:6], [0, 0, 0, 1]) and not state[c, 6:57].any()
    assert not state[c, ge.S_P:].any()
    assert len(set(kw["gw_index"])) == 2


@pytest.mark.gpu
def test_gpu_four_matrix_recursion(og, gpu_ctx, crafted, parity, monkeypatch):
    """6b. The same batch with OKVISGPU_GPS_FOUR_P=1 (read on every call): k_gps_async<true, 4> carries the
    reference's four dPdsigma matrices through the recursion and the symmetrisation and sums them at the
    end. Same contract and step counts as test_gpu_crafted_batch."""
    monkeypatch.setenv("OKVISGPU_GPS_FOUR_P", "1")
    args, kw, state0, index, ref, ref_state = crafted
    state = state0.copy()
    got = _run(og, gpu_ctx, args, kw, state)
    _compare(parity, "crafted_four_p", got, ref, state, ref_state)
    steps = {k: int(got["steps"][i]) for k, i in index.items()}
    assert (steps["a"], steps["c"], steps["d"], steps["h"], steps["i"]) == (1, 0, 8, 200, 1)


@pytest.mark.gpu
def test_gpu_random_batch_bitwise(og, gpu_ctx, random257, parity):
    """7. 257 random factors of 2 to 45 samples: within the contract; the first 1 and the first 5 alone
    give the bits they have inside the 257; two runs give the same bits."""
    args, kw, ref, ref_state = random257
    state = np.zeros((257, ge.STATE))
    full = _run(og, gpu_ctx, args, kw, state)
    _compare(parity, "random257", full, ref, state, ref_state)
    assert (full["steps"] > 0).all() and (state[:, ge.S_COUNTER] == 1).all()
    for n in (1, 5):
        sa, skw = _sub(args, kw, n)
        part_state = np.zeros((n, ge.STATE))
        _same_bits(_run(og, gpu_ctx, sa, skw, part_state), full, n)
        assert part_state.tobytes() == state[:n].tobytes()
    again_state = np.zeros((257, ge.STATE))
    _same_bits(_run(og, gpu_ctx, args, kw, again_state), full)
    assert again_state.tobytes() == state.tobytes()


@pytest.mark.gpu
def test_gpu_continuation(og, gpu_ctx, random257, parity):
    """8. Evaluate, move the biases by less than the threshold, evaluate again on the returned state: the
    device's first-order path. Then the same two calls with state = NULL (both fresh)."""
    args, kw = _sub(*random257[:2], 65)
    moved = _moved(kw, np.array([1e-4, -5e-5, 8e-5]), np.array([1e-2, -2e-2, 5e-3]))
    state, ref_state = np.zeros((65, ge.STATE)), np.zeros((65, ge.STATE))
    _run(og, gpu_ctx, args, kw, state)
    ge.evaluate_batch(*args, **kw, state=ref_state)
    first = state.copy()
    got = _run(og, gpu_ctx, args, moved, state)
    ref = ge.evaluate_batch(*args, **moved, state=ref_state)
    _compare(parity, "continuation", got, ref, state, ref_state)
    assert state.tobytes() == first.tobytes() and (state[:, ge.S_COUNTER] == 1).all()
    got = _run(og, gpu_ctx, args, moved, None)
    _compare(parity, "continuation_no_state", got, ge.evaluate_batch(*args, **moved))


@pytest.mark.gpu
def test_gpu_flags_and_synchronous(og, gpu_ctx, random257, parity):
    """9. use_imu_covariance = 0, redo_propagation_always = 1 (on a state that would not re-integrate), and
    kind 1, each against the restatement."""
    args, kw = _sub(*random257[:2], 65)
    state, ref_state = np.zeros((65, ge.STATE)), np.zeros((65, ge.STATE))
    got = _run(og, gpu_ctx, args, kw, state, use_imu_covariance=False)
    ref = ge.evaluate_batch(*args, **kw, state=ref_state, use_imu_covariance=False)
    _compare(parity, "no_imu_covariance", got, ref, state, ref_state)
    assert not state[:, ge.S_P:].any()
    moved = _moved(kw, 1e-5)
    got = _run(og, gpu_ctx, args, moved, state, redo_propagation_always=True)
    ref = ge.evaluate_batch(*args, **moved, state=ref_state, redo_propagation_always=True)
    _compare(parity, "redo_always", got, ref, state, ref_state)
    assert (state[:, ge.S_COUNTER] == 2).all() and state[:, ge.S_P:].any()
    sync_kw = dict(gw_index=kw["gw_index"], kind=1)
    got = _run(og, gpu_ctx, args, sync_kw)
    _compare(parity, "synchronous", got, ge.evaluate_batch(*args, **sync_kw))
    assert not got["J_speed_bias"].any() and not got["steps"].any()


@pytest.mark.gpu
def test_gpu_argument_errors(og, crafted):
    """10. Every refused call returns OKVISGPU_ERR_INVALID_ARGUMENT, leaves the sentinel in the outputs and
    the state alone, and names the factor; n = 0 and a result of NULLs succeed."""
    args, kw, state0, index, _, _ = crafted
    ip, r_SA, poses, T_GW, z, info = args
    lib = og.lib()
    ctx = og.Context(0)
    try:
        def refused(match, a=args, k=kw, **flags):
            state = state0.copy()
            b, keep = og.gps_batch(*a, **k, state=state, **flags)
            out = {name: np.full((b.n,) + og.GPS_OUTPUTS[name], -7, dtype=np.int32 if name == "steps" else np.float64)
                   for name in og.GPS_OUTPUTS}
            r = og.GpsResult()
            og._set_arrays(r, out)
            assert lib.okvisgpu_gps_evaluate(ctx.h, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
            msg = lib.okvisgpu_last_error(ctx.h).decode()
            assert match in msg, msg
            assert all((v == -7).all() for v in out.values()) and state.tobytes() == state0.tobytes()

        begin, ts = kw["sample_begin"], kw["sample_t"]
        shifted = begin.copy()
        shifted[0] = 1
        refused("start at 0", k=dict(kw, sample_begin=shifted))
        bad = begin.copy()
        bad[3] = bad[4] + 1
        refused("monotone", k=dict(kw, sample_begin=bad))
        short = kw["t_g"].copy()
        short[2] = ts[begin[3] - 1] + 1        # the samples of factor 2 do not reach t_g
        refused("factor 2", k=dict(kw, t_g=short))
        late = kw["t_k"].copy()
        late[3] = ts[begin[3]] - 1             # factor 3's first sample is newer than t_k
        refused("factor 3", k=dict(kw, t_k=late))
        back = kw["t_g"].copy()
        back[1] = kw["t_k"][1] - 1             # t_g < t_k
        refused("factor 1", k=dict(kw, t_g=back))
        for what, edit in (("finite", lambda m: m.__setitem__((0, 0), np.nan)),
                           ("symmetric", lambda m: m.__setitem__((0, 1), m[0, 1] + 1e-3)),
                           ("positive definite", lambda m: m.__setitem__((2, 2), -m[2, 2]))):
            broken = info.copy()
            edit(broken[4])
            refused("factor 4", a=(ip, r_SA, poses, T_GW, z, broken))
            assert what in lib.okvisgpu_last_error(ctx.h).decode()
        for v in (-1, 2):
            gw = kw["gw_index"].copy()
            gw[5] = v
            refused("factor 5", k=dict(kw, gw_index=gw))
        refused("kind", kind=2)

        w = og.SynthWindow(10, 500, 4000, seed=78)
        ctx.set_problems([w.problem])
        ctx.solve_begin(og.default_options(max_num_iterations=2))
        try:
            refused("solve_end")
        finally:
            ctx.solve_end()

        b, keep = og.gps_batch(*args, **kw)
        r = og.GpsResult()
        assert lib.okvisgpu_gps_evaluate(ctx.h, C.byref(b), C.byref(r)) == 0  # every output NULL
        assert lib.okvisgpu_gps_evaluate(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_gps_evaluate(ctx.h, None, C.byref(r)) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_gps_evaluate(ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
        b.n = 0
        assert lib.okvisgpu_gps_evaluate(ctx.h, C.byref(b), C.byref(r)) == 0
        b.n = -1
        assert lib.okvisgpu_gps_evaluate(ctx.h, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        b.n = len(poses)
        b.measurement = None
        assert lib.okvisgpu_gps_evaluate(ctx.h, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        assert "missing" in lib.okvisgpu_last_error(ctx.h).decode()
    finally:
        ctx.close()
