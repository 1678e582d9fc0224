"""The ImuError kernel (evalImuBlock, kernels_eval.hip) at functor level, on crafted sample layouts,
against a longdouble restatement of ImuError::redoPreintegration (tests/_imu_error.chain).

The kernel is compiled four ways (k_eval_few<16> for one or two windows, k_eval_few<4> up to the
few-window limit, k_eval_imu<false> beyond it, k_eval_imu<true> for okvisgpu_imu_append) and every
instantiation holds the same data-dependent paths: the chunked step records, the dt <= 0 skip, the
first- and last-step interpolation, saturation, the two small-angle branches, the uniform trip count
over the four factors of a wavefront, the Cholesky shortcut against the clamped Jacobi eigen-solver and
the redo decision. The generator's IMU data (a regular 200 Hz grid, equal sample counts, ascending
stamps, nothing saturated) reaches few of them, so the layouts here are made by hand
(_imu_error.layouts): two crafted windows, the second with zero bias random-walk densities, evaluated
alone, with one filler window and with 64, i.e. once by each of the three evaluation kernels.

What is compared, per factor:
  * the preintegration state the kernel writes to imu_state ([2..56] increments, [292..300] cross_,
    [301..525] P_delta_) against the longdouble chain; bound 16 max(e_ref, steps u), e_ref the oracle's
    own error on that factor and quantity, u = 2^-53. The factor 16 is the one _linsolve.bound allows
    another summation order: here the phase-split running sums, the block-sparse F_delta and the
    half-angle right Jacobian;
  * the square-root information U [66..290]: |U P U^T - I|_max with the chain's P for the Cholesky
    path (any orthogonal basis passes), the three blocks of U^T U against the mpmath
    (pseudo-)inverse for the clamped path; bound 16 max(e_ref, 15 u);
  * r and J against the oracle: the suite's basis-invariant J^T J, J^T r, |r|^2 at its 1e-12, and for
    the Cholesky path U^-1 r and U^-1 J (each side with its own U), bound 16 * 15 u * cond_2(U);
  * steps, the redo counter, the redo flag and speedAndBiases_ref_: exactly.
The CPU tests establish e_ref (oracle and float64 restatement against the chain), the reference's
redo logic and that four wrong restatements miss the GPU bound by a factor 100."""
import numpy as np
import pytest

import _imu_error as ie

SEED = 20261021
U53 = ie.U53
WITHIN = 4.0    # a reference error may exceed the value measured for it by at most this factor
CAUGHT = 100.0  # a mutation must miss the bound by at least this factor
# Worst reference errors measured over the covered layouts of the first crafted window (u = 2^-53):
MEASURED_U = {"oracle": {"inc": 18.2, "cross": 9.95, "P": 4.27}, "restatement": {"inc": 18.2, "cross": 9.95, "P": 4.69}}
MEASURED_SQRT = 5.26e-15     # oracle, |U P_ld U^T - I|_max
MEASURED_ZW_LEAD = 1.92e-15  # oracle, zero_walk: leading 9x9 of U^T U against the mpmath inverse (Frobenius rel)
REGIMES = {"alone": 0, "3 windows": 1, "66 windows": 64}  # tag -> filler windows behind the two crafted
KERNELS = {"alone": "k_eval_few<16>", "3 windows": "k_eval_few<4>", "66 windows": "k_eval_imu<false>"}
MOVES = (1e-4, 1e-4, 1e-3, 1e-3)  # of b_g, on factors of 49, 50, 49, 50 samples (redo threshold 3e-4, :845)


def _windows():
    """The two crafted windows, fresh: (layouts, params, OwnedProblem) each."""
    rng = np.random.default_rng(SEED)
    ip, ipz = ie.imu_params(), ie.imu_params(True)
    L = ie.layouts(rng, ip)
    p1 = ie.problem(L.values(), ip, rng)
    Z = ie.zero_walk_layouts(rng)
    return (L, ip, p1), (Z, ipz, ie.problem(Z.values(), ipz, rng))


def _fillers(n):
    """Copies of the first crafted window with other seeds."""
    ip = ie.imu_params()
    out = []
    for i in range(n):
        rng = np.random.default_rng(SEED + 1 + i)
        out.append(ie.problem(ie.layouts(rng, ip).values(), ip, rng))
    return out


def _errors(state, ref, ip):
    e = {"inc": ie.err_increments(state, ref), "cross": ie.err_cross(state, ref)}
    if ie.zero_walk(ip):
        e["P"] = ie.err_P(state, ref, 9)
        e["lead"], e["bias"], e["crs"] = ie.err_info_blocks(state, ie.information(ref["P"], ip))
    else:
        e["P"] = ie.err_P(state, ref)
        e["sqrt"] = ie.err_U(state, ref)
    return e


def _bounds(e_ref, steps):
    """Per quantity: 16 max(e_ref, steps u) for the state, 16 max(e_ref, 15 u) for the square root."""
    return {k: ie.bound(v, steps if k in ("inc", "cross", "P") else 15) for k, v in e_ref.items()}


@pytest.fixture(scope="module")
def crafted(oracle):
    """Per factor of the two crafted windows, computed once and left unchanged: the layout, the chain, the
    oracle's state / r / J after its first evaluation, the oracle's errors e_ref and the GPU bounds."""
    rows = []
    for w, (lay, ip, p) in enumerate(_windows()):
        r0, J0 = oracle.eval_imu(p.ptr(), len(lay))
        for f, (name, fac) in enumerate(lay.items()):
            ts, ga, t0, t1, sb = fac
            row = dict(name=name, window=w, ip=ip, factor=fac, ref=ie.chain(ts, ga, ip, sb, t0, t1),
                       ost=p.imu_state[f].copy(), r0=r0[f], J0=J0[f])
            if row["ref"] is not None:
                row["e_ref"] = _errors(row["ost"], row["ref"], ip)
                row["bound"] = _bounds(row["e_ref"], row["ref"]["steps"])
            rows.append(row)
    return rows


# ---- CPU: the references ------------------------------------------------------------------------------
def test_references_against_the_chain(crafted):
    """The oracle's imu_state after oracle.eval_imu and the float64 restatement, against the longdouble
    chain, on every covered layout. Neither is the code under test: these are the reference's own errors
    e_ref that the GPU bounds start from. Measured (u = 2^-53; oracle / restatement), each asserted within 4x:
      increments [2..56], relative to max(1, |x|):   18.2 u / 18.2 u   (N64; 0.03 u on `still`)
      cross_ [292..300], relative to max(1, |x|):     9.95 u / 9.95 u  (N64)
      P_delta_ relative to sqrt(P_ii P_jj):           4.27 u / 4.69 u  (N64)
      |U P_ld U^T - I|_max in longdouble (oracle):    5.26e-15         (on_stamps)
    zero_walk (N = 5, 22): increments 3.4 u / 4.5 u, cross_ 3.3 u / 4.5 u, the leading 9x9 of P 1.2 u / 1.8 u,
    the bias rows and columns of P exactly 0; U^T U: bias block exactly I / tol (tol = 2^-52), cross blocks
    exactly 0, leading 9x9 against the mpmath inverse 9.7e-16 / 1.92e-15 relative (Frobenius).
    The step counts of oracle, restatement and chain agree."""
    worst = {who: {"inc": 0.0, "cross": 0.0, "P": 0.0} for who in MEASURED_U}
    worst_sqrt = worst_lead = 0.0
    for row in crafted:
        ref = row["ref"]
        if ref is None:
            continue
        ts, ga, t0, t1, sb = row["factor"]
        rst, steps = ie.restatement(ts, ga, row["ip"], sb, t0, t1)
        assert steps == ref["steps"] == row["ost"][ie.S_STEPS], row["name"]
        eo = row["e_ref"]
        er = {"inc": ie.err_increments(rst, ref), "cross": ie.err_cross(rst, ref),
              "P": ie.err_P(rst, ref, 9 if row["window"] else 15)}
        print(f"{row['name']:14s} steps {steps:2d} (u) oracle " + " ".join(f"{k} {eo[k] / U53:5.2f}" for k in er)
              + " restatement " + " ".join(f"{k} {er[k] / U53:5.2f}" for k in er)
              + "".join(f" {k} {eo[k]:.2e}" for k in ("sqrt", "lead", "bias", "crs") if k in eo))
        for who, e in (("oracle", eo), ("restatement", er)):
            for k in worst[who]:
                worst[who][k] = max(worst[who][k], e[k] / U53)
        if row["window"]:
            assert eo["bias"] == 0.0 and eo["crs"] == 0.0, row["name"]  # exactly I / tol and 0
            worst_lead = max(worst_lead, eo["lead"])
        else:
            worst_sqrt = max(worst_sqrt, eo["sqrt"])
    print(f"worst (u): {worst}, sqrt {worst_sqrt:.3e}, zero_walk leading block {worst_lead:.3e}")
    for who in MEASURED_U:
        for k, v in worst[who].items():
            assert v <= WITHIN * MEASURED_U[who][k], (who, k, v)
    assert worst_sqrt <= WITHIN * MEASURED_SQRT
    assert worst_lead <= WITHIN * MEASURED_ZW_LEAD


def test_uncovered_on_the_oracle(crafted):
    """Samples ending 1 ms before t1 on a fresh functor (ImuError.cpp:270-273, :849-853): the redo counter
    counts the attempt, nothing is integrated (steps -1), and the evaluation fails quietly: r = 0, J = 0, the
    square-root information stays zero."""
    (row,) = [r for r in crafted if r["name"] == "uncovered"]
    st = row["ost"]
    assert row["ref"] is None
    assert st[ie.S_COUNTER] == 1 and st[ie.S_FLAG] == 0 and st[ie.S_STEPS] == -1
    assert not row["r0"].any() and not row["J0"].any() and not st[ie.S_U:ie.S_U + 225].any()


def _redo_window():
    rng = np.random.default_rng(SEED + 1000)
    ip = ie.imu_params()
    facs = []
    for n in (49, 50, 49, 50):
        sb = ie.speed_bias(rng)
        facs.append(ie.samples(rng, n, sb) + (sb,))
    return facs, ip, ie.problem(facs, ip, rng)


def _move_biases(p):
    for f, d in enumerate(MOVES):
        p.speed_biases[f, 3] += d


# per factor after the second evaluation: (counter, flag, re-integrated)
REDO_EXPECTED = ((1, 0, False), (1, 0, False), (2, 0, True), (1, 1, False))


def _check_redo(first, second, p):
    for f, (counter, flag, redone) in enumerate(REDO_EXPECTED):
        a, b = first[f], second[f]
        assert (b[ie.S_COUNTER], b[ie.S_FLAG]) == (counter, flag), f
        if redone:
            assert np.array_equal(b[ie.S_REF:ie.S_REF + 9], p.speed_biases[f]), f
            assert not np.array_equal(a[2:6], b[2:6]) and not np.array_equal(a[ie.S_U:ie.S_U + 225], b[ie.S_U:ie.S_U + 225])
        else:
            assert np.array_equal(a[2:], b[2:]), f  # increments, reference bias, U, steps, cross_, P_delta_


@pytest.fixture(scope="module")
def redo_oracle(oracle):
    """The oracle's two evaluations of the redo window: states, r, J after each and the moved problem."""
    facs, ip, p = _redo_window()
    r1, J1 = oracle.eval_imu(p.ptr(), 4)
    first = p.imu_state.copy()
    _move_biases(p)
    r2, J2 = oracle.eval_imu(p.ptr(), 4)
    return dict(facs=facs, ip=ip, p=p, first=first, second=p.imu_state.copy(), r1=r1, J1=J1, r2=r2, J2=J2)


def test_redo_logic_on_the_oracle(redo_oracle):
    """ImuError.cpp:833-859 on factors of 49, 50, 49, 50 samples whose b_g moves by 1e-4, 1e-4, 1e-3, 1e-3
    between two evaluations: below the threshold nothing happens; above it the factor of fewer than 50 samples
    re-integrates at the new bias (counter 2), the one of 50 keeps its preintegration and raises redo_."""
    o = redo_oracle
    assert all(s[ie.S_COUNTER] == 1 and s[ie.S_FLAG] == 0 for s in o["first"])
    _check_redo(o["first"], o["second"], o["p"])
    assert not np.array_equal(o["r1"], o["r2"])


MUTATIONS = (("step_start_ts", "backwards"), ("dup_prev_dt", "dup_mid"), ("no_saturation", "saturated"),
             ("restart_chunk", "backwards_8"))


@pytest.mark.parametrize("mutation,name", MUTATIONS, ids=[m for m, _ in MUTATIONS])
def test_mutations_are_caught(crafted, mutation, name):
    """Four subtly wrong float64 restatements (_imu_error.restatement) on the layout each targets: every one
    misses the GPU bound of a state quantity by at least a factor 100, and the unmutated restatement passes it."""
    (row,) = [r for r in crafted if r["name"] == name]
    ts, ga, t0, t1, sb = row["factor"]
    ref, bound = row["ref"], row["bound"]
    good, _ = ie.restatement(ts, ga, row["ip"], sb, t0, t1)
    bad, _ = ie.restatement(ts, ga, row["ip"], sb, t0, t1, mutation)
    factors = {}
    for k, fn in (("inc", ie.err_increments), ("cross", ie.err_cross), ("P", ie.err_P)):
        assert fn(good, ref) <= bound[k]
        factors[k] = fn(bad, ref) / bound[k]
    print(f"{mutation} on {name}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in factors.items()))
    assert max(factors.values()) >= CAUGHT, factors


# ---- GPU ----------------------------------------------------------------------------------------------
def _cu_count(og):
    """Compute units of device 0: hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount = 63) of the HIP
    runtime the library is linked to (the value okvisgpu_ctx_create hands the launch regime)."""
    import ctypes
    v = ctypes.c_int(0)
    assert og.lib().hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0
    assert 8 <= v.value <= 1024, v.value
    return v.value


@pytest.fixture(scope="module")
def gpu_runs(og, gpu_ctx):
    """imu_state, r and J of the two crafted windows after okvisgpu_eval_imu on fresh states, per regime and
    once with redo_always; the kernel of each regime from okvisgpu_launch_regime at the device's CU count."""
    cu = _cu_count(og)
    runs = {}
    for tag, n_fill, redo_always in [(t, n, False) for t, n in REGIMES.items()] + [("alone, redo_always", 0, True)]:
        (L, _, p1), (Z, _, p2) = _windows()
        wins = [p1, p2] + _fillers(n_fill)
        few = og.launch_regime(len(wins), cu)["few"]
        gpu_ctx.set_problems([w.struct for w in wins])
        st = gpu_ctx.stats()
        assert st["n_windows"] == len(wins) and st["n_imu"] == sum(len(w.imu_blocks) for w in wins)
        r1, J1 = gpu_ctx.eval_imu(len(L), 0, redo_always)
        state = np.concatenate([p1.imu_state, p2.imu_state])  # (every window's state is written back)
        r2, J2 = gpu_ctx.eval_imu(len(Z), 1, redo_always)
        runs[tag] = dict(kernel=("k_eval_few<16>" if len(wins) <= 2 else "k_eval_few<4>") if few else "k_eval_imu<false>",
                         state=state, r=np.concatenate([r1, r2]), J=np.concatenate([J1, J2]))
    assert {t: runs[t]["kernel"] for t in REGIMES} == KERNELS
    return runs


def _invariants(r, J, r0, J0):
    H, H0 = J.T @ J, J0.T @ J0
    g, g0 = J.T @ r, J0.T @ r0
    return (np.linalg.norm(H - H0) / np.linalg.norm(H0), np.linalg.norm(g - g0) / (np.linalg.norm(g0) + 1e-300),
            abs(r @ r - r0 @ r0) / (r0 @ r0))


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(REGIMES) + ["alone, redo_always"])
def test_gpu_crafted_layouts(crafted, gpu_runs, parity, regime):
    """Every crafted factor in one regime against the chain (state, U) and the oracle (r, J). The parity rows
    hold the worst error / bound over the factors (bound 1), the invariants their worst value (bound 1e-12)."""
    run = gpu_runs[regime]
    tag = f"imu paths [{regime}, {run['kernel']}]"
    worst = {}
    inv = [0.0, 0.0, 0.0]
    print(f"{tag}: error / bound per factor")
    for i, row in enumerate(crafted):
        st, r, J = run["state"][i], run["r"][i], run["J"][i]
        ts, ga, t0, t1, sb = row["factor"]
        U = st[ie.S_U:ie.S_U + 225].reshape(15, 15)
        assert (st[ie.S_COUNTER], st[ie.S_FLAG]) == (row["ost"][ie.S_COUNTER], row["ost"][ie.S_FLAG]) == (1, 0), row["name"]
        assert st[ie.S_STEPS] == row["ost"][ie.S_STEPS], (row["name"], st[ie.S_STEPS])
        if row["ref"] is None:  # uncovered: as the oracle, nothing integrated and a quiet failure
            assert not r.any() and not J.any() and not st[2:ie.S_STEPS].any() and not st[ie.S_CROSS:].any()
            continue
        assert st[ie.S_STEPS] == row["ref"]["steps"]
        assert np.array_equal(st[ie.S_REF:ie.S_REF + 9], sb), row["name"]
        e = _errors(st, row["ref"], row["ip"])
        ratios = {k: e[k] / row["bound"][k] for k in e}
        # the path taken: the Cholesky shortcut leaves a lower-triangular U, the eigen-solver a full one
        cholesky = not np.triu(U, 1).any()
        assert cholesky == (row["window"] == 0), row["name"]
        if cholesky:
            Uo = row["ost"][ie.S_U:ie.S_U + 225].reshape(15, 15)
            cb = 16.0 * 15.0 * U53 * np.linalg.cond(Uo)
            eg, eo = np.linalg.solve(U, r), np.linalg.solve(Uo, row["r0"])
            Fg, Fo = np.linalg.solve(U, J), np.linalg.solve(Uo, row["J0"])
            ratios["U^-1 r"] = np.linalg.norm(eg - eo) / np.linalg.norm(eo) / cb
            ratios["U^-1 J"] = np.linalg.norm(Fg - Fo) / np.linalg.norm(Fo) / cb
        for k, v in zip(range(3), _invariants(r, J, row["r0"], row["J0"])):
            inv[k] = max(inv[k], v)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        print(f"{row['name']:14s} " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in worst.items():
        parity(f"{tag} {k} (error / bound)", v, 1.0)
    for k, v in zip(("J^T J (Frobenius rel)", "J^T r (rel)", "|r|^2 (rel)"), inv):
        parity(f"{tag} {k}", v, 1e-12)


@pytest.mark.gpu
def test_gpu_regimes_agree(crafted, gpu_runs, parity):
    """The same factor alone, in 3 windows and in 66 windows: states equal within the bound each is held to
    against the chain (the three kernels differ in chunk length, not in the sums' order: the count of
    entries that differ bitwise is printed)."""
    base = gpu_runs["alone"]["state"]
    for regime in ("3 windows", "66 windows", "alone, redo_always"):
        other = gpu_runs[regime]["state"]
        worst, differing = 0.0, 0
        for i, row in enumerate(crafted):
            a, b = base[i], other[i]
            differing += int((a[2:] != b[2:]).sum())
            if row["ref"] is None:
                continue
            d = np.abs(a - b)
            Pa = a[ie.S_P:ie.S_P + 225].reshape(15, 15)
            n = 9 if row["window"] else 15
            s = np.sqrt(np.diag(Pa)[:n])
            e = {"inc": (d[2:57] / np.maximum(1, np.abs(a[2:57]))).max(),
                 "cross": (d[ie.S_CROSS:ie.S_CROSS + 9] / np.maximum(1, np.abs(a[ie.S_CROSS:ie.S_CROSS + 9]))).max(),
                 "P": (d[ie.S_P:ie.S_P + 225].reshape(15, 15)[:n, :n] / np.outer(s, s)).max()}
            worst = max(worst, max(e[k] / row["bound"][k] for k in e))
        print(f"alone against {regime}: {differing} state entries differ bitwise")
        parity(f"imu paths [alone against {regime}] state (difference / bound)", worst, 1.0)


def _append_cases(crafted):
    """N22, dup_mid, saturated and backwards, each split at an interior stamp m: the link [t0, ts[m]] over
    ts[:m + 1], then the samples ts[m:] appended up to t1 with another bias."""
    rng = np.random.default_rng(SEED + 2000)
    cases = []
    for name, m in (("N22", 9), ("dup_mid", 5), ("saturated", 7), ("backwards", 3)):
        (row,) = [r for r in crafted if r["name"] == name]
        ts, ga, t0, t1, sb = row["factor"]
        sb2 = sb.copy()
        sb2[3:6] += 5e-4 * rng.standard_normal(3)
        sb2[6:9] += 5e-3 * rng.standard_normal(3)
        cases.append(dict(name=name, first=(ts[:m + 1].copy(), ga[:m + 1].copy(), t0, int(ts[m]), sb),
                          ts=ts[m:].copy(), ga=ga[m:].copy(), t1_old=int(ts[m]), t1=t1, sb2=sb2))
    return cases


def _append_args(cases, state):
    begin = np.concatenate([[0], np.cumsum([len(c["ts"]) for c in cases])])
    return (state, np.array([c["t1_old"] for c in cases]), np.array([c["t1"] for c in cases]),
            np.array([c["sb2"] for c in cases]), begin, np.concatenate([c["ts"] for c in cases]),
            np.concatenate([c["ga"] for c in cases]))


@pytest.mark.gpu
def test_gpu_append_on_crafted_layouts(crafted, oracle, gpu_ctx, parity):
    """okvisgpu_imu_append (k_eval_imu<true>) from the states the device integrated, against the chain
    continued in longdouble; e_ref is the error of oracle.imu_append from the oracle's own first link."""
    ip = ie.imu_params()
    cases = _append_cases(crafted)
    rng = np.random.default_rng(SEED + 2001)
    po = ie.problem([c["first"] for c in cases], ip, rng)
    oracle.eval_imu(po.ptr(), len(cases))
    ost = po.imu_state.copy()
    osteps = oracle.imu_append(ip, *_append_args(cases, ost))
    rng = np.random.default_rng(SEED + 2001)
    pg = ie.problem([c["first"] for c in cases], ip, rng)
    gpu_ctx.set_problems([pg.struct])
    gpu_ctx.eval_imu(len(cases))
    before = pg.imu_state.copy()
    gst = before.copy()
    gsteps = gpu_ctx.imu_append(ip, *_append_args(cases, gst))
    worst = {}
    for i, c in enumerate(cases):
        first = ie.chain(*c["first"][:2], ip, c["first"][4], c["first"][2], c["first"][3])
        ref = ie.chain(c["ts"], c["ga"], ip, c["sb2"], c["t1_old"], c["t1"], init=first)
        assert gsteps[i] == osteps[i] == ref["steps"] > 0, c["name"]
        assert gst[i, ie.S_STEPS] == ost[i, ie.S_STEPS]
        assert np.array_equal(gst[i, :2], before[i, :2]) and np.array_equal(gst[i, ie.S_REF:ie.S_REF + 9], c["first"][4])
        bound = _bounds(_errors(ost[i], ref, ip), first["steps"] + ref["steps"])
        e = _errors(gst[i], ref, ip)
        print(f"append {c['name']:10s} steps {first['steps']} + {ref['steps']}: error / bound "
              + " ".join(f"{k} {e[k] / bound[k]:.3f}" for k in e))
        for k in e:
            worst[k] = max(worst.get(k, 0.0), e[k] / bound[k])
    for k, v in worst.items():
        parity(f"imu paths [append, k_eval_imu<true>] {k} (error / bound)", v, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_fill", (0, 65), ids=("1 window", "66 windows"))
def test_gpu_redo_logic(og, gpu_ctx, redo_oracle, parity, n_fill):
    """The sequence of test_redo_logic_on_the_oracle through okvisgpu_update_params + okvisgpu_eval_imu, on
    the device's own states: counters, flags and kept states as the reference's, the re-integrated factor
    against the chain at the moved bias, r and J against the oracle's second evaluation."""
    o = redo_oracle
    facs, ip, p = _redo_window()
    wins = [p] + _fillers(n_fill)
    gpu_ctx.set_problems([w.struct for w in wins])
    gpu_ctx.eval_imu(4)
    first = p.imu_state.copy()
    assert np.array_equal(first[:, :2], o["first"][:, :2])
    _move_biases(p)
    gpu_ctx.update_params()
    r, J = gpu_ctx.eval_imu(4)
    second = p.imu_state.copy()
    _check_redo(first, second, p)
    assert np.array_equal(second[:, :2], o["second"][:, :2]) and np.array_equal(second[:, ie.S_STEPS], o["second"][:, ie.S_STEPS])
    tag = f"imu paths [redo logic, {1 + n_fill} windows]"
    ts, ga, t0, t1, _ = facs[2]
    ref = ie.chain(ts, ga, ip, p.speed_biases[2], t0, t1)
    bound = _bounds(_errors(o["second"][2], ref, ip), ref["steps"])
    e = _errors(second[2], ref, ip)
    for k in e:
        parity(f"{tag} re-integrated {k} (error / bound)", e[k] / bound[k], 1.0)
    inv = np.max([_invariants(r[f], J[f], o["r2"][f], o["J2"][f]) for f in range(4)], axis=0)
    for k, v in zip(("J^T J (Frobenius rel)", "J^T r (rel)", "|r|^2 (rel)"), inv):
        parity(f"{tag} {k}", v, 1e-12)
