"""okvisgpu_imu_propagate: the static ImuError::propagation (ImuError.cpp:537-759) for a batch of
items on the device: the pose and speed of ViGraph::addStatesPropagate (ViGraph.cpp:400-417) and
ThreadedSlam::processFrame (ThreadedSlam.cpp:613-627), and with the 15x15 covariance and Jacobian
what Frontend::propagation (Frontend.cpp:1146-1162) asks for.

CPU: the numpy restatement (tests/_imu_propagate.py) against the pose-and-speed helper the
sliding-window tests use, against finite differences, against a closed form, on the degenerate
cases, and against the solver's own ImuError (the oracle). GPU: okvisgpu_imu_propagate against the
restatement at the functor-level contract: pose, speed/bias and Jacobian within
1e-12 max(1, |ref|), the covariance within 1e-12 max|P_ref| per item, steps equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _imu_propagate as ipr
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
NS = 5_000_000  # 200 Hz
# the bound of the ImuError tie (tests 7 and 13): 100 x the largest |weighted residual| measured on
# the CPU (test_tie_to_the_solvers_imu_error's docstring)
TIE_MEASURED = 5.1e-13
TIE_BOUND = 100 * TIE_MEASURED


def _params(og):
    ip = og.ImuParams()
    ip.a_max, ip.g_max = 176.0, 7.8
    ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c = 12.0e-4, 8.0e-3, 4.0e-6, 4.0e-5
    ip.g = 9.81007
    return ip


def _pack(items):
    """[(pose, sb, t_start, t_end, ts, ga)] -> the batch arrays."""
    poses = np.ascontiguousarray([it[0] for it in items], dtype=np.float64)
    sbs = np.ascontiguousarray([it[1] for it in items], dtype=np.float64)
    t0 = np.array([it[2] for it in items], np.int64)
    t1 = np.array([it[3] for it in items], np.int64)
    begin = np.concatenate([[0], np.cumsum([len(it[4]) for it in items])]).astype(np.int32)
    ts = np.concatenate([np.asarray(it[4], np.int64) for it in items])
    ga = np.concatenate([np.asarray(it[5], np.float64).reshape(-1, 6) for it in items])
    return poses, sbs, t0, t1, begin, ts, ga


def _full_step_item(ip):
    """Two samples, t_start and t_end on them, identity rotation, one gyro and one accelerometer
    component above the limits (test 4 / 8a)."""
    t = 7_000_000_000 + np.arange(2, dtype=np.int64) * NS
    ga = np.array([[0.1, 1.5 * ip.g_max, -0.2, 0.3, 0.1, 9.8], [0.1, 0.2, -0.2, 0.3, -1.2 * ip.a_max, 9.8]])
    pose = np.array([1.0, -2.0, 0.5, 0.0, 0.0, 0.0, 1.0])
    sb = np.array([0.4, -0.3, 0.1, 0.01, -0.02, 0.005, 0.05, -0.02, 0.1])
    return pose, sb, int(t[0]), int(t[1]), t, ga


def _full_step_covariance(ip, dt):
    s_v = dt * 100 * ip.sigma_a_c ** 2
    return np.diag(np.repeat([0.5 * dt * dt * s_v, dt * (100 * ip.sigma_g_c) ** 2, s_v, dt * ip.sigma_gw_c ** 2,
                              dt * ip.sigma_aw_c ** 2], 3))


def _crafted(ip):
    """The ragged batch of test 8, items a..i, and the index of each."""
    rng = np.random.default_rng(811)

    def motion(N, t0=3_000_000_000):
        t = t0 + np.arange(N, dtype=np.int64) * NS
        w = rng.uniform(-1, 1, 3) + 0.2 * rng.normal(size=(N, 3))
        a = np.array([0.0, 0.0, 9.81]) + rng.uniform(-2, 2, 3) + 0.5 * rng.normal(size=(N, 3))
        q = rng.normal(size=4)
        pose = np.concatenate([rng.uniform(-5, 5, 3), q / np.linalg.norm(q)])
        sb = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.1, 0.1, 3)])
        return pose, sb, t, np.hstack([w, a])

    items = {}
    items["a"] = _full_step_item(ip)
    pose, sb, t, ga = motion(2)
    items["b"] = (pose, sb, int(t[0] + 1_234_567), int(t[1] - 777_777), t, ga)
    pose, sb, t, ga = motion(6)
    items["c"] = (pose, sb, int(t[0] + 2_000_000), int(t[3]), t, ga)
    pose, sb, t, ga = motion(9)
    items["d"] = (pose, sb, int(t[2]), int(t[8] - 1_000_000), t, ga)
    pose, sb, t, ga = motion(4)
    items["e"] = (pose, sb, int(t[1] + 1_000_000), int(t[1] + 1_000_000), t, ga)
    pose, sb, t, ga = motion(5)
    items["f"] = (pose, sb, int(t[0]), int(t[4] + 1), t, ga)  # the last sample 1 ns before t_end
    pose, sb, t, ga = motion(8)
    ga[3, 1] = 2.0 * ip.g_max
    ga[4, 5] = -1.5 * ip.a_max
    items["g"] = (pose, sb, int(t[0] + 1_000_000), int(t[7] - 1_000_000), t, ga)
    pose, sb, t, ga = motion(1)
    items["h"] = (pose, sb, int(t[0] + 3), int(t[0] - 2), t, ga)
    pose, sb, t, ga = motion(201)
    items["i"] = (pose, sb, int(t[0]), int(t[200]), t, ga)
    return list(items.values()), {k: i for i, k in enumerate(items)}


@pytest.fixture(scope="module")
def crafted(og):
    ip = _params(og)
    items, index = _crafted(ip)
    batch = _pack(items)
    return ip, batch, index, ipr.propagate_batch(ip, *batch)


@pytest.fixture(scope="module")
def random257(og):
    ip = _params(og)
    batch = ipr.random_items(np.random.default_rng(257), 257)
    return ip, batch, ipr.propagate_batch(ip, *batch)


def _sub(batch, n):
    """The first n items of a batch."""
    poses, sbs, t0, t1, begin, ts, ga = batch
    return poses[:n].copy(), sbs[:n].copy(), t0[:n], t1[:n], begin[:n + 1], ts[:begin[n]], ga[:begin[n]]


# ------------------------------------------------------------------------------------------ CPU
def test_symbol_and_struct_layout(og, tmp_path):
    """1. The entry point is declared, exported and refuses NULL; ImuPropagateBatch mirrors the header."""
    assert "okvisgpu_imu_propagate" in og.EXPORTED_SYMBOLS
    lib = og.lib()
    assert hasattr(lib, "okvisgpu_imu_propagate")
    assert lib.okvisgpu_imu_propagate(None, None, None) != 0
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    t = "okvisgpu_imu_propagate_batch"
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {",
           f'  printf("%zu %zu %zu\\n", sizeof({t}), offsetof({t}, covariance), offsetof({t}, jacobian));',
           "  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    size, o_cov, o_jac = (int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(og.ImuPropagateBatch)
    assert o_cov == og.ImuPropagateBatch.covariance.offset and o_jac == og.ImuPropagateBatch.jacobian.offset


def test_restatement_equals_the_sliding_window_helper(og):
    """2. Pose and speed against _ref_scenarios.imu_propagate on ViGraph2World's samples, over one, two
    and three frame intervals: the same formulas, within 1e-13 max(1, |value|) (evaluation order and
    the final normalisation)."""
    import _ref_scenarios as rs
    world = rs.ViGraph2World(0, 5)
    T = np.array([0.3, -0.2, 0.1, *rs.angle_axis(np.array([0.1, -0.2, 0.3]))])
    sb = np.array([1.0, 0.1, -0.05, 1e-3, -2e-3, 5e-4, 0.02, -0.01, 0.03])
    worst = 0.0
    for k0, k1 in ((0, 1), (1, 2), (3, 5), (2, 5), (7, 8)):
        t0, t1 = int(world.frame_t[k0]), int(world.frame_t[k1])
        sel = (world.ts >= t0 - 20_000_000) & (world.ts <= t1 + 20_000_000)
        ts, ga = world.ts[sel], world.ga[sel]
        steps, T1, sb1, _, _ = ipr.propagate(ts, ga, world.imu_params, T, sb, t0, t1, covariance=False)
        Tr, sbr = rs.imu_propagate(ts, ga, world.imu_params, T, sb, t0, t1)
        assert steps > 0
        for got, ref in ((T1, Tr), (sb1, sbr)):
            worst = max(worst, (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    assert worst <= 1e-13, worst


def test_jacobian_against_finite_differences(og):
    """3. Central differences (h = 1e-6; delta r additive, q <- deltaQ(d alpha) (x) q, minus =
    2 vec(q1 (x) q0^-1)) over 24 random items of <= 45 samples: within 1e-3 max(1, |J|)."""
    ip = _params(og)
    poses, sbs, t0, t1, begin, ts, ga = ipr.random_items(np.random.default_rng(3), 24)
    h, worst = 1e-6, 0.0
    for i in range(len(t0)):
        s = slice(begin[i], begin[i + 1])
        steps, _, _, _, J = ipr.propagate(ts[s], ga[s], ip, poses[i], sbs[i], t0[i], t1[i], covariance=False)
        assert steps > 0
        fd = np.zeros((15, 15))
        for j in range(15):
            d = np.zeros(15)
            d[j] = h
            Tp, sbp = ipr.box_plus(poses[i], sbs[i], d)
            Tm, sbm = ipr.box_plus(poses[i], sbs[i], -d)
            _, T1p, sb1p, _, _ = ipr.propagate(ts[s], ga[s], ip, Tp, sbp, t0[i], t1[i], covariance=False)
            _, T1m, sb1m, _, _ = ipr.propagate(ts[s], ga[s], ip, Tm, sbm, t0[i], t1[i], covariance=False)
            fd[:, j] = ipr.box_minus(T1p, sb1p, T1m, sb1m) / (2 * h)
        worst = max(worst, np.abs(fd - J).max() / max(1.0, np.abs(J).max()))
    print(f"finite differences: worst {worst:.3e}")
    assert worst <= 1e-3, worst


def test_one_full_step_in_closed_form(og):
    """4. One saturated step from zero covariance at the identity rotation: P is the step's noise."""
    ip = _params(og)
    pose, sb, t0, t1, ts, ga = _full_step_item(ip)
    steps, _, _, P, _ = ipr.propagate(ts, ga, ip, pose, sb, t0, t1)
    assert steps == 1
    ref = _full_step_covariance(ip, NS * 1e-9)
    assert np.array_equal(P != 0, ref != 0)
    assert (np.abs(P - ref) <= 1e-15 * np.abs(ref)).all()


def test_degenerate_and_uncovered(og, crafted):
    """5, 6. t_end == t_start, t_end < t_start and a one-sample item: 0 steps, inputs unchanged, J = I,
    P = 0. The last sample 1 ns before t_end: -1."""
    ip, batch, index, (steps, poses, sbs, P, J) = crafted
    c = index["c"]
    rows = slice(batch[4][c], batch[4][c + 1])
    pose, sb, t, ga = batch[0][c], batch[1][c], batch[5][rows], batch[6][rows]
    s, T1, sb1, Pi, Ji = ipr.propagate(t, ga, ip, pose, sb, int(t[2]), int(t[1]))  # t_end < t_start
    assert s == 0 and T1.tobytes() == pose.tobytes() and sb1.tobytes() == sb.tobytes()
    assert np.array_equal(Ji, np.eye(15)) and not Pi.any()
    for k in ("e", "h"):
        i = index[k]
        assert steps[i] == 0
        assert poses[i].tobytes() == batch[0][i].tobytes() and sbs[i].tobytes() == batch[1][i].tobytes()
        assert np.array_equal(J[i], np.eye(15)) and not P[i].any()
    assert steps[index["f"]] == -1
    assert (steps[[index[k] for k in "abcdgi"]] == [1, 1, 3, 6, 7, 200]).all()


def _tie_window(og):
    return og.SynthWindow(10, 500, 4000, seed=77)


def _tie_factors(w):
    p = w.problem
    n = p.n_imu
    begin = np.ctypeslib.as_array(p.imu_sample_begin, shape=(n + 1,))
    ts = np.ctypeslib.as_array(p.imu_sample_t_ns, shape=(begin[-1],))
    ga = np.ctypeslib.as_array(p.imu_sample_gyr_acc, shape=(begin[-1], 6))
    t0 = np.ctypeslib.as_array(p.imu_t0_ns, shape=(n,))
    t1 = np.ctypeslib.as_array(p.imu_t1_ns, shape=(n,))
    blocks = np.ctypeslib.as_array(p.imu_blocks, shape=(n, 4))
    return [(blocks[f], int(t0[f]), int(t1[f]), ts[begin[f]:begin[f + 1]], ga[begin[f]:begin[f + 1]]) for f in range(n)]


def _tie(w, propagate_one):
    """Chain the window's states along its IMU factors with propagate_one(pose0, sb0, t0, t1, ts, ga)
    -> (pose1, sb1): pose1 and the speed of sb1 from the propagation, the bias of sb1 = that of sb0."""
    poses, sbs = w.poses(), w.speed_biases()
    assert not w.imu_state().any()  # fresh: the first evaluation integrates at the current bias
    for blk, t0, t1, ts, ga in _tie_factors(w):
        pose1, sb1 = propagate_one(poses[blk[0]].copy(), sbs[blk[1]].copy(), t0, t1, ts, ga)
        poses[blk[2]] = pose1
        sbs[blk[3]] = sb1


def test_tie_to_the_solvers_imu_error(og, oracle):
    """7. Propagating (pose0, sb0) over each IMU factor's samples and writing the result into the
    factor's second state makes the solver's own ImuError vanish: the bias rows are zero by
    construction, so every entry of the weighted residual is rounding noise times the square-root
    information.
    Measured on the CPU (seed 77, the 9 factors of an S10 window): max |r| = 5.08e-13; asserted 100 x
    that, 5.1e-11."""
    w = _tie_window(og)
    ip = w.problem.imu_params

    def one(pose0, sb0, t0, t1, ts, ga):
        steps, pose1, sb1, _, _ = ipr.propagate(ts, ga, ip, pose0, sb0, t0, t1, covariance=False)
        assert steps > 0
        return pose1, sb1

    _tie(w, one)
    r, _ = oracle.eval_imu(w.problem_ptr(), w.problem.n_imu)
    print(f"ImuError tie (CPU): max |r| = {np.abs(r).max():.3e}")
    assert np.abs(r).max() <= TIE_BOUND


# ------------------------------------------------------------------------------------------ GPU
def _compare(parity, name, got, ref, check_matrices=True):
    """GPU (steps, poses, sbs, P, J) against the restatement's, per item, at the contract."""
    steps, poses, sbs, P, J = got
    rsteps, rposes, rsbs, rP, rJ = ref
    assert np.array_equal(steps, rsteps)
    rel = lambda a, b: (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()
    parity(f"imu_propagate/{name}/pose", rel(poses, rposes), 1e-12)
    parity(f"imu_propagate/{name}/speed_bias", rel(sbs, rsbs), 1e-12)
    ok = steps >= 0
    if J is not None:
        parity(f"imu_propagate/{name}/jacobian", rel(J[ok], rJ[ok]), 1e-12)
    if P is not None:
        worst = 0.0
        for i in np.flatnonzero(ok):
            m = np.abs(rP[i]).max()
            if m == 0.0:
                assert not P[i].any()
            else:
                worst = max(worst, np.abs(P[i] - rP[i]).max() / m)
        parity(f"imu_propagate/{name}/covariance", worst, 1e-12)


def _run(ctx, ip, batch, covariance=True, jacobian=True):
    poses, sbs, t0, t1, begin, ts, ga = batch
    poses, sbs = poses.copy(), sbs.copy()
    n = len(t0)
    P = np.full((n, 15, 15), np.nan) if covariance else False
    J = np.full((n, 15, 15), np.nan) if jacobian else False
    out = ctx.imu_propagate(ip, poses, sbs, t0, t1, begin, ts, ga, covariance=P, jacobian=J)
    steps = out if isinstance(out, np.ndarray) else out[0]
    return steps, poses, sbs, (P if covariance else None), (J if jacobian else None)


@pytest.mark.gpu
def test_gpu_crafted_batch(og, gpu_ctx, crafted, parity):
    """8. The ragged batch of crafted items a..i, with and without the matrices."""
    ip, batch, index, ref = crafted
    got = _run(gpu_ctx, ip, batch)
    _compare(parity, "crafted", got, ref)
    steps, poses, sbs, P, J = got
    a, f = index["a"], index["f"]
    exp = _full_step_covariance(ip, NS * 1e-9)
    assert np.array_equal(P[a] != 0, exp != 0) and (np.abs(P[a] - exp) <= 1e-15 * np.abs(exp)).all()
    assert steps[f] == -1
    assert poses[f].tobytes() == batch[0][f].tobytes() and sbs[f].tobytes() == batch[1][f].tobytes()
    assert np.isnan(P[f]).all() and np.isnan(J[f]).all()
    assert not np.isnan(np.delete(P, f, axis=0)).any() and not np.isnan(np.delete(J, f, axis=0)).any()
    for k in ("e", "h"):
        i = index[k]
        assert poses[i].tobytes() == batch[0][i].tobytes() and sbs[i].tobytes() == batch[1][i].tobytes()
        assert np.array_equal(J[i], np.eye(15)) and not P[i].any()
    lane = _run(gpu_ctx, ip, batch, covariance=False, jacobian=False)
    _compare(parity, "crafted_lane", lane, ref)
    assert lane[1][f].tobytes() == batch[0][f].tobytes() and lane[2][f].tobytes() == batch[1][f].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("matrices", [True, False])
def test_gpu_batch_sizes_bitwise(og, gpu_ctx, random257, parity, matrices):
    """9. Batches of 1, 3, 65 and 257 items (a partial group, a partial wavefront, several workgroups
    in either mapping): within the contract, and each item's bits the same in every batch."""
    ip, batch, ref = random257
    full = _run(gpu_ctx, ip, batch, covariance=matrices, jacobian=matrices)
    _compare(parity, "random257" + ("" if matrices else "_lane"), full, ref)
    assert (full[0] > 0).all()
    for n in (1, 3, 65):
        part = _run(gpu_ctx, ip, _sub(batch, n), covariance=matrices, jacobian=matrices)
        for a, b in zip(part, full):
            assert (a is None and b is None) or a.tobytes() == b[:n].tobytes(), n


@pytest.mark.gpu
def test_gpu_output_combinations(og, gpu_ctx, random257, parity):
    """10. covariance / jacobian NULL or not, each within the contract; the same call twice gives the
    same bits."""
    ip, batch, ref = random257
    sub = _sub(batch, 65)
    ref65 = tuple(r[:65] for r in ref)
    for cov in (False, True):
        for jac in (False, True):
            got = _run(gpu_ctx, ip, sub, covariance=cov, jacobian=jac)
            _compare(parity, f"combo_cov{int(cov)}_jac{int(jac)}", got, ref65)
            again = _run(gpu_ctx, ip, sub, covariance=cov, jacobian=jac)
            for a, b in zip(got, again):
                assert (a is None and b is None) or a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_gpu_argument_errors(og, crafted):
    """11. Refused calls leave the caller's arrays alone; n = 0 and steps = NULL succeed."""
    ip, batch, index, _ = crafted
    lib = og.lib()
    ctx = og.Context(0)
    try:
        def refused(b, match):
            poses, sbs, t0, t1, begin, ts, ga = b
            poses, sbs = poses.copy(), sbs.copy()
            P, J = np.full((len(t0), 15, 15), np.nan), np.full((len(t0), 15, 15), np.nan)
            with pytest.raises(og.OkvisGpuError, match=match):
                ctx.imu_propagate(ip, poses, sbs, t0, t1, begin, ts, ga, covariance=P, jacobian=J)
            assert poses.tobytes() == b[0].tobytes() and sbs.tobytes() == b[1].tobytes()
            assert np.isnan(P).all() and np.isnan(J).all()

        poses, sbs, t0, t1, begin, ts, ga = batch
        late = t0.copy()
        late[2] = ts[begin[2]] - 1  # item 2's first sample is newer than t_start
        refused((poses, sbs, late, t1, begin, ts, ga), "item 2")
        empty = begin.copy()
        empty[4] = empty[5]  # item 4 without samples
        refused((poses, sbs, t0, t1, empty, ts, ga), "item 4")
        bad = begin.copy()
        bad[3] = bad[4] + 1
        refused((poses, sbs, t0, t1, bad, ts, ga), "monotone")
        shifted = begin.copy()
        shifted[0] = 1
        refused((poses, sbs, t0, t1, shifted, ts, ga), "start at 0")

        w = og.SynthWindow(10, 500, 4000, seed=78)
        ctx.set_problems([w.problem])
        ctx.solve_begin(og.default_options(max_num_iterations=2))
        try:
            refused(batch, "solve_end")
        finally:
            ctx.solve_end()

        b, keep = og.imu_propagate_batch(ip, poses.copy(), sbs.copy(), t0, t1, begin, ts, ga)
        assert lib.okvisgpu_imu_propagate(ctx.h, C.byref(b), None) == 0  # steps = NULL
        assert lib.okvisgpu_imu_propagate(None, C.byref(b), None) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_imu_propagate(ctx.h, None, None) == ERR_INVALID_ARGUMENT
        b.n = 0
        assert lib.okvisgpu_imu_propagate(ctx.h, C.byref(b), None) == 0
        b.n = -1
        assert lib.okvisgpu_imu_propagate(ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
        b.n = len(t0)
        b.poses = None
        assert lib.okvisgpu_imu_propagate(ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
    finally:
        ctx.close()


@pytest.mark.gpu
def test_gpu_context_undisturbed(og, gpu_ctx, crafted):
    """12. A solve, a propagation, then the same solve again: bitwise the same poses and costs."""
    ip, batch, _, _ = crafted
    w = og.SynthWindow(10, 500, 4000, seed=79)
    opts = og.default_options(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0,
                              parameter_tolerance=0.0)
    gpu_ctx.set_problems([w.problem])
    s1 = gpu_ctx.solve(opts)[0]
    assert s1["num_iterations"] == 3
    poses1 = w.poses().copy()
    _run(gpu_ctx, ip, batch)
    _run(gpu_ctx, ip, batch, covariance=False, jacobian=False)
    w.reset()
    gpu_ctx.update_params()
    s2 = gpu_ctx.solve(opts)[0]
    assert w.poses().tobytes() == poses1.tobytes()
    assert s2["initial_cost"] == s1["initial_cost"] and s2["final_cost"] == s1["final_cost"]


@pytest.mark.gpu
def test_gpu_tie_to_the_solvers_imu_error(og, gpu_ctx, parity):
    """13. Test 7 with the device propagation and the device ImuError, at test 7's bound."""
    w = _tie_window(og)
    ip = w.problem.imu_params

    def one(pose0, sb0, t0, t1, ts, ga):
        poses, sbs = pose0[None].copy(), sb0[None].copy()
        steps = gpu_ctx.imu_propagate(ip, poses, sbs, [t0], [t1], [0, len(ts)], ts, ga)
        assert steps[0] > 0
        return poses[0], sbs[0]

    _tie(w, one)
    gpu_ctx.set_problems([w.problem])
    r, _ = gpu_ctx.eval_imu(w.problem.n_imu)
    parity("imu_propagate/tie_to_imu_error", np.abs(r).max(), TIE_BOUND)
