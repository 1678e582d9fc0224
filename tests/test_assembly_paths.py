"""The assembly of the reduced system (kernels_schur.hip asmPairsHeavy / asmPairsLight / asmPairsSb,
shared by k_assemble_pp, k_assemble_pp_light, k_assemble_sb and k_assemble_few) and the packed work
item record it reads (device_problem.hpp AsmRec, plan.cpp assemblyRecords).

  * host records (CPU): every record of the `_batch70` plan of test_plan_digest.py at 32 and 256 CUs
    equals what the planner's separate arrays give for its item, pads included;
  * S and rhs of small shaped windows against the oracle's reduction at 1e-11 (the bound of
    test_gpu_parity.py and test_lm_visit_paths.py), mu = 0 and mu = 1e-2: alone (k_assemble_few) and
    inside a batch of 70 unequal windows (light list, XCD interleave, pads);
  * position independence: the same window first, in the middle and last in that batch gives the
    same bits of S and rhs (diagF enters S's diagonal at mu > 0; the ABI has no read-back of its own
    for it), also with the window count changed by one;
  * masks: a batch in which every other window ends at its first gradient test and one retries mu.

The shaped windows start from a synthetic window and keep chosen observations (`_assembly.py`); each
test first checks from the planner's records (okvisgpu_plan_assembly) that the window has the pair it
is there for. A speed/bias block carries at most one prior per block in these problems but nothing
in the problem format forbids several, so the pairs with 5 contributions (nc > kSbPre) are built
from repeated priors on one block."""
import numpy as np
import pytest

from _assembly import LIGHT_MAX, chain_window, expected_records, owned, pair_runs, retry_window, with_sb_priors

S10 = (10, 500, 4000)
S_TOL = 1e-11
MUS = (0.0, 1e-2)


def _batch70(og):
    # test_plan_digest._batch70: >= 64 windows (light lists) and >= 8 (XCD interleave), unequal windows
    shapes = [S10, (6, 150, 1000), (20, 800, 6000)]
    return [og.SynthWindow(*shapes[i % 3], seed=1 + i) for i in range(70)]


# ---------------------------------------------------------------------------------- host records
@pytest.mark.parametrize("cu", [32, 256])
def test_host_records_restate_the_arrays(og, cu):
    ws = _batch70(og)
    counts, rec, old = og.plan_assembly([w.problem for w in ws], cu)
    assert len(rec) == sum(counts) and all(c > 0 for c in counts), counts
    n_pad = int((old[:, 0] < 0).sum())
    assert n_pad > 0 and (old[counts[0] + counts[1]:, 0] >= 0).all()  # pads in the interleaved lists only
    want = expected_records(old)
    bad = np.flatnonzero((rec != want).any(axis=1))
    assert bad.size == 0, (bad[:8], rec[bad[:2]], want[bad[:2]])
    # the lists: light items are off-diagonal pose-pose pairs without visits and few contributions
    live = old[:, 0] >= 0
    light = np.zeros(len(old), bool)
    light[counts[0]:counts[0] + counts[1]] = True
    r = rec[live & light]
    assert (r[:, 10] == 0).all() and (r[:, 1] == r[:, 2]).all() and (r[:, 4] - r[:, 1] <= LIGHT_MAX).all()
    sb = rec[counts[0] + counts[1]:]
    assert ((sb[:, 10] & 6) != 0).all() and ((rec[:counts[0] + counts[1]][:, 10] & 6) == 0).all()
    # every pair of the batch is some item exactly once
    pairs = old[live, 0]
    assert len(np.unique(pairs)) == len(pairs) and pairs.min() == 0 and pairs.max() == len(pairs) - 1


def test_single_window_records(og):
    """One window: no light list, no pads, the records in pair order per list."""
    counts, rec, old = og.plan_assembly([og.SynthWindow(*S10, seed=20251015).problem], 256)
    assert counts[1] == 0 and (old[:, 0] >= 0).all()
    assert (rec == expected_records(old)).all()


# ------------------------------------------------------------------------ S and rhs against the oracle
CHAIN_BIG = (1, 7, 8, 9, 16, 17, 24, 25, 64, 65)  # in a large batch: the light / heavy threshold is 24 / 25
N_BATCH = 70
SHAPED_AT = (3, 17, 44)  # positions of the shaped windows among the fillers (three XCD queues, not the first item)


def _fill(og, n):
    shapes = [S10, (6, 150, 1000), (20, 800, 6000)]
    return [owned(og, *shapes[i % 3], seed=4300 + i) for i in range(n)]


def _chain_few(og):
    # 16-landmark groups alone; a pose prior (keyframe 0), two relative-pose edges
    return chain_window(og, 16, 4101, n_relpose=2, relpose_stride=3)


def _chain_big(og):
    return chain_window(og, 64, 4102, counts=CHAIN_BIG)


def _extrinsics(og):
    return owned(og, 6, 150, 1000, seed=4103, do_extrinsics=1)


def _sb_priors(og):
    # speed/bias diagonal pairs: 1 (last state), 2 (two IMU factors), 3 (+ one prior), 5 (+ three priors)
    return with_sb_priors(owned(og, 6, 150, 1000, seed=4104), np.array([2, 3, 3, 3]))


SHAPES = {"chain_few": _chain_few, "chain_big": _chain_big, "extrinsics": _extrinsics, "sb_priors": _sb_priors}


class _Ref:
    """A shaped window and the oracle's reduction of it per mu, computed once and left unchanged."""

    def __init__(self, oracle, P):
        self.P = P
        self.red = {mu: oracle.linearize_reduce(P.ptr(), True, mu) for mu in MUS}
        again = oracle.linearize_reduce(P.ptr(), True, MUS[1])
        for S, rhs, cost, rc in self.red.values():
            assert rc == 0 and np.isfinite(S).all() and np.isfinite(rhs).all()
        assert np.abs(again[0] - self.red[MUS[1]][0]).max() <= S_TOL * np.abs(again[0]).max()


@pytest.fixture(scope="module")
def refs(og, oracle):
    return {name: _Ref(oracle, build(og)) for name, build in SHAPES.items()}


@pytest.fixture(scope="module")
def fillers(og):
    return _fill(og, N_BATCH + 1)


def _runs(og, problems, cu=256):
    counts, rec, _ = og.plan_assembly(problems, cu)
    nv, npart, nfac, flags = pair_runs(rec)
    live = rec[rec[:, 0] >= 0]
    heavy = np.zeros(len(rec), bool)
    heavy[:counts[0]] = True
    light = np.zeros(len(rec), bool)
    light[counts[0]:counts[0] + counts[1]] = True
    keep = rec[:, 0] >= 0
    return dict(win=live[:, 0], nv=nv, npart=npart, nfac=nfac, diag=(flags & 1) != 0, sb=(flags & 6) != 0,
                heavy=heavy[keep], light=light[keep], n_pad=int((~keep).sum()), counts=counts)


def test_shapes_have_their_pairs(og, refs):
    """The planner's records show the pairs each shaped window is there for (CPU)."""
    r = _runs(og, [refs["chain_few"].P.struct])
    pp = ~r["sb"]
    assert r["counts"][1] == 0  # one window: no light list
    assert {1, 8, 9, 64, 65} <= set(r["nv"][pp & r["diag"]])            # 65: a second round of 64 descriptors
    assert {1, 7, 8, 9, 16, 17, 32, 33} <= set(r["npart"][pp & ~r["diag"]])
    assert (pp & ~r["diag"] & (r["npart"] == 0) & (r["nfac"] == 1)).sum() >= 1   # factor blocks only
    P = refs["chain_few"].P
    assert P.struct.n_pose_priors >= 1 and P.struct.n_relpose == 2 and np.all(np.diff(P.relpose_blocks, axis=1) == 3)
    # (the 11 IMU factors couple neighbours, the two relative-pose edges keyframes three apart)
    assert (pp & ~r["diag"] & (r["nfac"] == 1)).sum() == len(P.poses) - 1 + 2
    r = _runs(og, [refs["extrinsics"].P.struct])
    assert np.any(refs["extrinsics"].P.extrinsics_constant == 0)
    r = _runs(og, [refs["sb_priors"].P.struct])
    tot = (r["nv"] + r["npart"] + r["nfac"])[r["sb"] & r["diag"]]
    assert {1, 2, 3, 5} <= set(tot)  # 5 > kSbPre: the loop over the descriptors


def _batch_of(refs, fillers, n, at=None):
    """n windows: the fillers with the shaped windows at SHAPED_AT (or `at`: {position: name})."""
    at = at or dict(zip(SHAPED_AT, ("chain_big", "sb_priors", "extrinsics")))
    ws = list(fillers[:n])
    for k, name in at.items():
        ws[k] = refs[name].P
    return ws, at


def test_batch_has_its_pairs(og, refs, fillers):
    ws, at = _batch_of(refs, fillers, N_BATCH)
    r = _runs(og, [w.struct for w in ws])
    assert r["n_pad"] > 0 and r["counts"][1] > 0
    k = [p for p, n in at.items() if n == "chain_big"][0]
    mine = r["win"] == k
    tot = r["npart"] + r["nfac"]
    assert {1, 7, 8, 9, 16, 17, 24} <= set(tot[mine & r["light"]]) and tot[mine & r["light"]].max() == 24
    assert 25 in set(tot[mine & r["heavy"] & ~r["diag"]])
    assert 65 in set(r["nv"][mine & r["heavy"] & r["diag"]])
    k = [p for p, n in at.items() if n == "sb_priors"][0]
    assert {1, 2, 3, 5} <= set((r["nfac"])[(r["win"] == k) & r["sb"] & r["diag"]])


def _check_reduce(ctx, ref, parity, tag, window=0):
    for mu, (S0, rhs0, cost0, rc) in ref.red.items():
        S, rhs, cost = ctx.linearize_reduce(window, True, mu)
        assert S.shape == S0.shape
        parity(f"{tag} S, mu={mu} (max abs / max |S|)", np.abs(S - S0).max() / np.abs(S0).max(), S_TOL)
        parity(f"{tag} rhs, mu={mu} (max abs / max |rhs|)", np.abs(rhs - rhs0).max() / np.abs(rhs0).max(), S_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain_few", "extrinsics", "sb_priors"])
def test_reduce_alone(og, gpu_ctx, refs, parity, name):
    """One window: k_assemble_few (one pair per wavefront, no light list)."""
    gpu_ctx.set_problems([refs[name].P.struct])
    _check_reduce(gpu_ctx, refs[name], parity, f"assembly {name} alone")


@pytest.mark.gpu
def test_reduce_in_batch(og, gpu_ctx, refs, fillers, parity):
    """70 unequal windows: k_assemble_pp, k_assemble_pp_light (XCD interleave, pads) and k_assemble_sb."""
    ws, at = _batch_of(refs, fillers, N_BATCH)
    gpu_ctx.set_problems([w.struct for w in ws])
    for k, name in at.items():
        _check_reduce(gpu_ctx, refs[name], parity, f"assembly {name} in a batch of {N_BATCH}", window=k)


# ---------------------------------------------------------------------------- position independence
@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_BATCH, N_BATCH + 1])
def test_position_independence(og, gpu_ctx, refs, fillers, n):
    """The same window first, in the middle and last in the batch: the first items of the lists, the
    middle and the tail with its pads. Its S (with mu > 0 the diagonal carries diagF^2 mu) and rhs are
    the same bits at the three positions; n + 1 windows shift every list."""
    got = []
    for pos in (0, n // 2, n - 1):
        ws, _ = _batch_of(refs, fillers, n, at={pos: "chain_big"})
        gpu_ctx.set_problems([w.struct for w in ws])
        got.append([gpu_ctx.linearize_reduce(pos, True, mu)[:2] for mu in MUS])
    for other in got[1:]:
        for (S0, r0), (S1, r1) in zip(got[0], other):
            assert np.array_equal(S0, S1) and np.array_equal(r0, r1)


# ------------------------------------------------------------------------------------------- masks
N_MASK = 66
G_TOL = 1e-2  # a window at its optimum has a gradient far below it, a fresh window far above (checked below)
MU_FLOOR = 1e-8
_TIMES = ("total_time_s", "preprocessor_time_s", "minimizer_time_s", "postprocessor_time_s", "linear_solver_time_s",
          "residual_evaluation_time_s", "jacobian_evaluation_time_s", "step_time_s")


def _same_summary(a, b):
    return all(a[k] == b[k] for k in a if k not in _TIMES)


@pytest.mark.gpu
def test_masks(og, gpu_ctx, parity):
    """66 windows: the even ones start at their optimum and end at the first gradient test, the odd
    ones run three iterations and window 1 retries mu. The finished windows are skipped pair by pair
    inside the wavefronts that also hold live pairs: every live window gives the bits it gives when
    live fillers stand in the finished windows' places, and the retrying window its solve alone."""
    shapes = [(6, 150, 1000), S10]
    done_ws = [owned(og, *shapes[i % 2], seed=4500 + i) for i in range(N_MASK // 2)]
    subst = [owned(og, *shapes[i % 2], seed=4600 + i) for i in range(N_MASK // 2)]
    live_ws = [retry_window(og, 4700)] + [owned(og, *shapes[i % 2], seed=4700 + i) for i in range(1, N_MASK // 2)]
    # (to a gradient a hundred times below G_TOL; some of these windows take a few hundred iterations)
    tight = og.default_options(max_num_iterations=2000, function_tolerance=0.0, gradient_tolerance=1e-2 * G_TOL,
                               parameter_tolerance=0.0)
    gpu_ctx.set_problems([w.struct for w in done_ws])
    gpu_ctx.solve(tight, len(done_ws))  # (writes the optimum back into done_ws)
    opts = og.default_options(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=G_TOL,
                              parameter_tolerance=0.0, min_lm_diagonal=1e-318)
    snaps = [w.snapshot() for w in live_ws]

    def run(even):
        for w, s in zip(live_ws, snaps):
            w.restore(s)
        ws = [None] * N_MASK
        ws[0::2], ws[1::2] = even, live_ws
        gpu_ctx.set_problems([w.struct for w in ws])
        sums = gpu_ctx.solve(opts, N_MASK)
        return sums, [(w.poses.copy(), w.landmarks.copy()) for w in live_ws]

    sa, pa = run(done_ws)
    late = [(2 * k, s["num_iterations"], s["termination_type"]) for k, s in enumerate(sa[0::2])
            if s["num_iterations"] > 1 or s["termination_type"] != 0]
    assert not late, late
    assert all(s["num_iterations"] == 3 for s in sa[1::2])
    assert sa[1]["final_mu"] > 10 * MU_FLOOR and all(s["final_mu"] == MU_FLOOR for s in sa[3::2])  # one retry
    sb, pb = run(subst)
    assert all(s["num_iterations"] == 3 for s in sb)
    for k in range(N_MASK // 2):
        assert _same_summary(sa[2 * k + 1], sb[2 * k + 1]), (k, sa[2 * k + 1], sb[2 * k + 1])
        assert np.array_equal(pa[k][0], pb[k][0]) and np.array_equal(pa[k][1], pb[k][1]), k
    # the retrying window alone: the cross-regime bounds of test_gpu_parity.test_window_alone_vs_large_batch
    live_ws[0].restore(snaps[0])
    gpu_ctx.set_problems([live_ws[0].struct])
    s1 = gpu_ctx.solve(opts, 1)[0]
    for f in ("num_iterations", "termination_type", "num_successful_steps"):
        assert s1[f] == sa[1][f], f
    parity(f"retrying window alone vs in a batch of {N_MASK}: cost (rel)",
           abs(s1["final_cost"] - sa[1]["final_cost"]) / sa[1]["final_cost"], 1e-9)
    parity(f"retrying window alone vs in a batch of {N_MASK}: positions (m)",
           float(np.abs(live_ws[0].poses[:, :3] - pa[0][0][:, :3]).max()), 1e-8)
