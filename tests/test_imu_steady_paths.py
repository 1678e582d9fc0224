"""The two kernels an ImuError evaluation of a large batch runs through (kernels_eval.hip): k_eval_imu_steady
evaluates the wavefronts (four factors each) none of whose live factors redoes its preintegration and leaves
one byte per wavefront; k_eval_imu<false> behind it runs the others as before. Both call the same residual
and Jacobian section, so which kernel evaluated a factor must not show in a single bit of r, J or imu_state.

All cases run in the regime that reaches k_eval_imu<false> (66 windows: REGIMES["66 windows"] of
tests/test_imu_error_paths.py), on the crafted layouts of tests/_imu_error.py:
  1. a second evaluation at unchanged parameters (steady path) against the first (fresh state: heavy path);
  2. a wavefront in which one factor re-integrates and three do not (heavy path for all four) against the same
     three factors evaluated without it (steady path), the re-integrating factor at each of the four positions;
  3. the redo flag raised without a redo (a factor of 50 samples), and the same with redo_always (heavy path);
  4. factor counts of 4k + 1, 4k + 2 and 4k + 3 (a last wavefront of one, two and three factors), with and
     without the prior workgroups behind the factor wavefronts.
"Bit-equal" compares the bit patterns. The one exception is the layout `uncovered`, whose evaluation fails
quietly: its zeros are compared as values (a failed evaluation writes +0, the kept all-zero U gives 0 * x)."""
import numpy as np
import pytest

import _imu_error as ie
import test_imu_error_paths as paths
from _problem import OwnedProblem, pose_error_sqrt_info

U53 = ie.U53
N_FILL = paths.REGIMES["66 windows"]
CHOSEN = (4, 5, 6, 7)  # N16, N17, N22, N33: wavefront 1 of the batch, positions 0..3; all under 50 samples
INV_NAMES = ("J^T J (Frobenius rel)", "J^T r (rel)", "|r|^2 (rel)")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _heavy_kernel(og, n_windows):
    assert not og.launch_regime(n_windows, paths._cu_count(og))["few"]


def _unshared(factors, ip, rng):
    """_imu_error.problem with blocks of its own for every factor: factor f on (2f, 2f, 2f + 1, 2f + 1), so that
    moving one factor's bias reaches no other factor (in the chained problem block f + 1 is factor f's second)."""
    factors = list(factors)
    n = len(factors)
    p = ie.problem(factors, ip, rng)
    q = rng.standard_normal((2 * n, 4))
    p.poses = np.concatenate([rng.standard_normal((2 * n, 3)), q / np.linalg.norm(q, axis=1)[:, None]], axis=1)
    p.pose_constant = np.zeros(2 * n, np.uint8)
    sbs = np.array([ie.speed_bias(rng) for _ in range(2 * n)])
    sbs[0::2] = [f[4] for f in factors]
    p.speed_biases = sbs
    p.speed_bias_constant = np.zeros(2 * n, np.uint8)
    p.imu_blocks = np.array([[2 * f, 2 * f, 2 * f + 1, 2 * f + 1] for f in range(n)], np.int32)
    return p.bind()


def _chain_checks(tag, parity, st, r, J, ost, r0, J0, fac, ip, sb_now):
    """One re-integrated factor at the bounds of test_gpu_crafted_layouts: the state against the chain at the
    bias it was integrated with, bound from the oracle's own error; r and J against the oracle."""
    ts, ga, t0, t1, _ = fac
    ref = ie.chain(ts, ga, ip, sb_now, t0, t1)
    bound = paths._bounds(paths._errors(ost, ref, ip), ref["steps"])
    e = paths._errors(st, ref, ip)
    for k in e:
        parity(f"{tag} {k} (error / bound)", e[k] / bound[k], 1.0)
    U, Uo = (s[ie.S_U:ie.S_U + 225].reshape(15, 15) for s in (st, ost))
    assert not np.triu(U, 1).any()  # the Cholesky path
    cb = 16.0 * 15.0 * U53 * np.linalg.cond(Uo)
    eg, eo = np.linalg.solve(U, r), np.linalg.solve(Uo, r0)
    Fg, Fo = np.linalg.solve(U, J), np.linalg.solve(Uo, J0)
    parity(f"{tag} U^-1 r (error / bound)", np.linalg.norm(eg - eo) / np.linalg.norm(eo) / cb, 1.0)
    parity(f"{tag} U^-1 J (error / bound)", np.linalg.norm(Fg - Fo) / np.linalg.norm(Fo) / cb, 1.0)
    for k, v in zip(INV_NAMES, paths._invariants(r, J, r0, J0)):
        parity(f"{tag} {k}", v, 1e-12)


# ---- 1 ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("window", (0, 1), ids=("first crafted window", "zero-walk window"))
def test_second_evaluation_gives_the_first_bits(og, gpu_ctx, window):
    """eval_imu on fresh states (redo counter 0: every wavefront takes the heavy kernel), then again at unchanged
    parameters (every wavefront but the ones holding an `uncovered` factor takes k_eval_imu_steady): r and J of
    every factor of the window bit-equal, imu_state bit-equal from entry 1 on, the counters as the redo rule has them."""
    (L, _, p1), (Z, _, p2) = paths._windows()
    wins = [p1, p2] + paths._fillers(N_FILL)
    _heavy_kernel(og, len(wins))
    gpu_ctx.set_problems([w.struct for w in wins])
    lay, p = ((L, p1), (Z, p2))[window]
    r1, J1 = gpu_ctx.eval_imu(len(lay), window)
    s1 = [w.imu_state.copy() for w in wins]
    r2, J2 = gpu_ctx.eval_imu(len(lay), window)
    s2 = [w.imu_state.copy() for w in wins]
    for f, name in enumerate(lay):
        if name == "uncovered":
            assert not r1[f].any() and not J1[f].any() and np.array_equal(r1[f], r2[f]) and np.array_equal(J1[f], J2[f])
            continue
        assert r1[f].any() and J1[f].any(), name
        assert _same_bits(r1[f], r2[f]), name
        assert _same_bits(J1[f], J2[f]), name
    # every window of the batch. `uncovered` never integrates, so its reference bias stays zero and it redoes at
    # every evaluation (ImuError.cpp:845-853): its counter is 2, and its wavefront takes the heavy kernel again.
    again = np.array([name == "uncovered" for name in L], dtype=np.float64)
    for i, (a, b) in enumerate(zip(s1, s2)):
        assert (a[:, ie.S_COUNTER] == 1).all()
        assert np.array_equal(b[:, ie.S_COUNTER], 1 + (0 * b[:, 0] if i == 1 else again))
        assert _same_bits(a[:, 1:], b[:, 1:])


# ---- 2 ------------------------------------------------------------------------------------------------
def _mixed_windows():
    rng = np.random.default_rng(paths.SEED + 3000)
    ip = ie.imu_params()
    L = ie.layouts(rng, ip)
    p1 = _unshared(L.values(), ip, rng)
    (_, _, _), (_, _, p2) = paths._windows()
    return L, ip, p1, [p1, p2] + paths._fillers(N_FILL)


def _move(wins, chosen):
    """b_g of every factor's first speed/bias block + 1e-4 (below the redo threshold 3e-4, ImuError.cpp:845), of
    the chosen factor of window 0 + 1e-3."""
    for w in wins:
        w.speed_biases[:, 3] += 1e-4
    if chosen is not None:
        wins[0].speed_biases[2 * chosen, 3] += 1e-3 - 1e-4


def _mixed_run(ctx, chosen):
    L, ip, p1, wins = _mixed_windows()
    ctx.set_problems([w.struct for w in wins])
    ctx.eval_imu(len(L), 0)
    first = p1.imu_state.copy()
    _move(wins, chosen)
    ctx.update_params()
    r, J = ctx.eval_imu(len(L), 0)
    return dict(L=L, ip=ip, p=p1, first=first, r=r, J=J, state=p1.imu_state.copy())


@pytest.fixture(scope="module")
def mixed_steady(gpu_ctx):
    """Configuration B: every factor moved by 1e-4, no redo anywhere (computed once, left unchanged)."""
    return _mixed_run(gpu_ctx, None)


@pytest.mark.gpu
@pytest.mark.parametrize("chosen", CHOSEN, ids=[f"position {c % 4}" for c in CHOSEN])
def test_mixed_wavefront(og, oracle, gpu_ctx, mixed_steady, parity, chosen):
    """Configuration A (the chosen factor moved by 1e-3 re-integrates: its wavefront takes the heavy kernel with
    three factors that do not) against B (all steady): every other factor of the window bit-equal in r, J and
    imu_state; the chosen one against the chain and the oracle at the bounds of test_gpu_crafted_layouts."""
    assert chosen % 4 == CHOSEN.index(chosen) and chosen // 4 == CHOSEN[0] // 4
    A, B = _mixed_run(gpu_ctx, chosen), mixed_steady
    _heavy_kernel(og, 2 + N_FILL)
    names = list(A["L"])
    assert len(A["L"][names[chosen]][0]) < 50
    for f, name in enumerate(names):
        a, b = A["state"][f], B["state"][f]
        if f == chosen:
            assert (a[ie.S_COUNTER], a[ie.S_FLAG]) == (2, 0) and (b[ie.S_COUNTER], b[ie.S_FLAG]) == (1, 0)
            assert np.array_equal(a[ie.S_REF:ie.S_REF + 9], A["p"].speed_biases[2 * f])
            assert _same_bits(b[2:], A["first"][f][2:]) and not np.array_equal(a[2:6], b[2:6])
            continue
        assert _same_bits(a, b), name
        if name == "uncovered":
            assert np.array_equal(A["r"][f], B["r"][f]) and np.array_equal(A["J"][f], B["J"][f])
        else:
            assert A["r"][f].any() and _same_bits(A["r"][f], B["r"][f]), name
            assert _same_bits(A["J"][f], B["J"][f]), name
    # the oracle on the same window and sequence
    L, ip, po, wo = _mixed_windows()
    oracle.eval_imu(po.ptr(), len(L))
    _move(wo, chosen)
    r0, J0 = oracle.eval_imu(po.ptr(), len(L))
    ost = po.imu_state[chosen]
    assert (ost[ie.S_COUNTER], ost[ie.S_FLAG]) == (2, 0) and A["state"][chosen][ie.S_STEPS] == ost[ie.S_STEPS]
    _chain_checks(f"imu steady paths [mixed wavefront, position {chosen % 4}]", parity, A["state"][chosen], A["r"][chosen],
                  A["J"][chosen], ost, r0[chosen], J0[chosen], L[names[chosen]], ip, po.speed_biases[2 * chosen])


# ---- 3 ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("redo_always", (False, True), ids=("flag without redo", "redo_always"))
def test_flag_without_redo(og, oracle, gpu_ctx, parity, redo_always):
    """Factors of 49, 50, 49, 50 samples whose b_g moves by 1e-4, 1e-4, 1e-3, 1e-3 (test_redo_logic_on_the_oracle).
    redo_always off: factor 3 (50 samples, 1e-3) keeps its preintegration, state[1] becomes 1 and state[0] stays:
    its wavefront holds factor 2, which redoes (heavy kernel); factor 3 of the window behind it, moved the same way
    with factor 2 left alone, takes the steady kernel. redo_always on: factor 3 re-integrates (heavy kernel).
    Counters, flags and steps as the oracle's, r and J against the oracle's second evaluation."""
    def build():
        facs, ip, a = paths._redo_window()
        _, _, b = paths._redo_window()
        return facs, ip, [a, b] + paths._fillers(N_FILL)

    def move(wins):
        paths._move_biases(wins[0])
        wins[1].speed_biases[3, 3] += paths.MOVES[3]  # only the factor of 50 samples: no redo in its wavefront

    facs, ip, wins = build()
    _heavy_kernel(og, len(wins))
    gpu_ctx.set_problems([w.struct for w in wins])
    gpu_ctx.eval_imu(4, 0, redo_always)
    first = [w.imu_state.copy() for w in wins[:2]]
    move(wins)
    gpu_ctx.update_params()
    rg = [gpu_ctx.eval_imu(4, w, redo_always) for w in (0, 1)]
    second = [w.imu_state.copy() for w in wins[:2]]  # (the call for window 1 evaluates again: nothing moves)
    _, _, wo = build()
    ro = []
    for w in (0, 1):
        oracle.eval_imu(wo[w].ptr(), 4, redo_always)
    move(wo)
    for w in (0, 1):
        ro.append(oracle.eval_imu(wo[w].ptr(), 4, redo_always))
    for w in (0, 1):
        ost = wo[w].imu_state
        assert np.array_equal(second[w][:, :2], ost[:, :2]) and np.array_equal(second[w][:, ie.S_STEPS], ost[:, ie.S_STEPS])
        if redo_always:
            assert (second[w][3, ie.S_COUNTER], second[w][3, ie.S_FLAG]) == (2, 0)
            assert not np.array_equal(second[w][3, 2:6], first[w][3, 2:6])
        else:
            assert (second[w][3, ie.S_COUNTER], second[w][3, ie.S_FLAG]) == (1, 1) and first[w][3, ie.S_FLAG] == 0
            assert _same_bits(second[w][3, 2:], first[w][3, 2:])
        inv = np.max([paths._invariants(rg[w][0][f], rg[w][1][f], ro[w][0][f], ro[w][1][f]) for f in range(4)], axis=0)
        for k, v in zip(INV_NAMES, inv):
            parity(f"imu steady paths [{'redo_always' if redo_always else 'flag without redo'}, window {w}] {k}", v, 1e-12)
    if not redo_always:  # the same factor through either kernel: only state[0..1] of its neighbours differ
        assert _same_bits(rg[0][0][3], rg[1][0][3]) and _same_bits(rg[0][1][3], rg[1][1][3])


# ---- 4 ------------------------------------------------------------------------------------------------
def _prior_window(rng):
    """One pose with one PoseError and nothing else: the window's cost is 1/2 |r|^2 of the batch's first prior."""
    p = OwnedProblem()
    q = rng.standard_normal(4)
    p.poses = np.concatenate([rng.standard_normal(3), q / np.linalg.norm(q)])[None, :]
    p.pose_constant = np.zeros(1, np.uint8)
    q = p.poses[0, 3:] + 0.05 * rng.standard_normal(4)
    p.pose_prior_block = np.zeros(1, np.int32)
    p.pose_prior_meas = np.concatenate([p.poses[0, :3] + 0.1 * rng.standard_normal(3), q / np.linalg.norm(q)])[None, :]
    L = pose_error_sqrt_info(1e-2, 1e-3).reshape(6, 6) + 0.5 * np.tril(rng.standard_normal((6, 6)), -1)
    p.pose_prior_sqrt_info = L.reshape(1, 36)
    return p.bind()


def _tail_windows(tail, priors):
    (_, _, p1), (_, _, p2) = paths._windows()
    wins = [p1, p2] + paths._fillers(N_FILL - 1)
    n_imu = sum(len(w.imu_blocks) for w in wins)
    n_last = next(n for n in range(19, 23) if (n_imu + n) % 4 == tail)
    rng = np.random.default_rng(paths.SEED + 4000 + tail)
    ip = ie.imu_params()
    lay = dict(list(ie.layouts(rng, ip).items())[:n_last])
    assert list(lay)[-1] != "uncovered"
    wins.append(ie.problem(lay.values(), ip, rng))
    if priors:
        wins.append(_prior_window(rng))
    return wins, n_last


@pytest.mark.gpu
@pytest.mark.parametrize("priors", (False, True), ids=("no priors", "priors behind"))
@pytest.mark.parametrize("tail", (1, 2, 3))
def test_tail_wavefront(og, oracle, gpu_ctx, parity, tail, priors):
    """A last factor wavefront of `tail` factors (its idle groups load with clamped indices and store nothing),
    without and with the prior workgroups behind the factor wavefronts: the batch's last factor against the oracle
    through the heavy kernel (first evaluation) and the steady one (second, bit-equal to the first), the factors
    in front of it unharmed (bit-equal between the two), and the first prior's residual as the cost of its window."""
    wins, n_last = _tail_windows(tail, priors)
    last = N_FILL + 1
    _heavy_kernel(og, len(wins))
    gpu_ctx.set_problems([w.struct for w in wins])
    assert gpu_ctx.stats()["n_imu"] % 4 == tail
    r1, J1 = gpu_ctx.eval_imu(n_last, last)
    r2, J2 = gpu_ctx.eval_imu(n_last, last)
    assert _same_bits(r1, r2) and _same_bits(J1, J2) and r1[-1].any()
    wo, _ = _tail_windows(tail, priors)
    r0, J0 = oracle.eval_imu(wo[last].ptr(), n_last)
    assert np.array_equal(wins[last].imu_state[:, :2], wo[last].imu_state[:, :2])
    for path, (r, J) in (("heavy", (r1, J1)), ("steady", (r2, J2))):
        for k, v in zip(INV_NAMES, paths._invariants(r[-1], J[-1], r0[-1], J0[-1])):
            parity(f"imu steady paths [tail {tail}, {'priors' if priors else 'no priors'}, {path}] last factor {k}", v, 1e-12)
    if priors:
        cg, co = gpu_ctx.evaluate(last + 1), oracle.evaluate(wo[last + 1].ptr())
        assert co > 0.0
        parity(f"imu steady paths [tail {tail}] first prior 1/2 |r|^2 (rel)", abs(cg - co) / co, 1e-12)
