"""okvisgpu_covisibilities: ViGraph::computeCovisibilities (ViGraph.cpp:727-785) on the device.

CPU: the two restatements (tests/_covis.py) against each other and a hand-written case, the entry
point's NULL check and the struct layout. GPU: the device counts against the restatement. The
operation is all integers, so every comparison is exact (np.array_equal / tobytes)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _covis
from _paths import REPO
from _problem import _ARRAYS, OwnedProblem

ERR_INVALID_ARGUMENT, ERR_NO_PROBLEM = 1, 5
KEYS = ("counts", "n_observed", "visible")
SCALARS = ("n_pairs", "n_visible", "any")

# The path-0 budget of the count kernel is 64 KiB of LDS for n_states rows of (words | 1) 64-bit words,
# words = ceil(n_landmarks / 64) (kCovisLdsBudget, covisRowStride in csrc/launch.hpp). 200 states and
# 2,500 landmarks are 40 words, stride 41: 200 * 41 * 8 = 65,600 bytes, 64 over the budget, the
# smallest 200-state window on the tiled path. The same window cut to 2,496 landmarks has 39 words:
# 200 * 39 * 8 = 62,400 bytes, path 0.
TILED = (200, 2500, 20000)
TILED_CUT = 2496

_CACHE = {}


def _window(og, key):
    """OwnedProblem copies of the synthetic windows (generated once, handed out as copies)."""
    if key not in _CACHE:
        make = {"s6": lambda: og.SynthWindow(6, 150, 1000, seed=3),
                "s10": lambda: og.SynthWindow(10, 500, 4000, seed=20251015),
                "dense": lambda: og.SynthWindow(100, 200, 30000, seed=7, kf_dt_s=0.02, max_obs_per_landmark=240),
                "tiled": lambda: og.SynthWindow(*TILED, seed=26),
                "s530": lambda: og.SynthWindow(530, 2000, 16000, seed=9)}[key]
        _CACHE[key] = OwnedProblem.copy_of(make().problem)
    return OwnedProblem.copy_of(_CACHE[key].struct)


def _keep_observations(q, keep):
    for k, (_, _, cnt) in _ARRAYS.items():
        if cnt == "n_observations":
            setattr(q, k, getattr(q, k)[keep])
    return q.bind()


def _crafted(og):
    """The S6 window with pose 2 unobserved and the observations of landmarks >= 40 dropped (one
    word of 40 bits; landmarks 40.. stay in the problem without observations), and landmarks 0..4
    left with their first pose only."""
    q = _window(og, "s6")
    keep = (q.obs_pose != 2) & (q.obs_landmark < 40)
    for l in range(5):
        of_l = np.flatnonzero(keep & (q.obs_landmark == l))
        assert len(of_l)
        keep[of_l[q.obs_pose[of_l] != q.obs_pose[of_l].min()]] = False
    return _keep_observations(q, keep)


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    for k in SCALARS:
        assert a[k] == b[k], k


def _consistent(res):
    c = res["counts"]
    assert c.dtype == np.int32 and res["n_observed"].dtype == np.int32
    assert np.array_equal(c, c.T) and not np.diag(c).any() and (c >= 0).all()
    assert res["n_pairs"] == int((np.triu(c, 1) > 0).sum())
    assert np.array_equal(res["visible"], res["n_observed"] > 0)
    assert res["n_visible"] == int(res["visible"].sum())
    assert res["any"] == (res["n_pairs"] > 0)
    # a pair is counted on landmarks both states observe
    assert (c <= np.minimum.outer(res["n_observed"], res["n_observed"])).all()


# ---------------------------------------------------------------- CPU: the restatements
@pytest.mark.parametrize("key", ["s6", "s10", "dense"])
def test_restatements_agree(og, key):
    q = _window(og, key)
    rng = np.random.default_rng(5)
    for ex in (None, rng.random(len(q.landmarks)) < 0.3):
        a, b = _covis.of_problem(q, ex, _covis.literal), _covis.of_problem(q, ex, _covis.matrix)
        _same(a, b)
        _consistent(a)
        assert a["any"]


def test_hand_checked_case():
    """Three poses, four landmarks: l0 from poses 0, 1 (pose 0 with both cameras), l1 from 0, 1, 2,
    l2 from pose 2 alone, l3 unobserved."""
    obs_pose = [0, 0, 1, 0, 1, 2, 2]
    obs_lm = [0, 0, 0, 1, 1, 1, 2]
    want = np.array([[0, 2, 1], [2, 0, 1], [1, 1, 0]])
    for f in (_covis.literal, _covis.matrix):
        r = f(obs_pose, obs_lm, 3, 4)
        assert np.array_equal(r["counts"], want)
        assert list(r["n_observed"]) == [2, 2, 2] and r["visible"].all()
        assert (r["n_pairs"], r["n_visible"], r["any"]) == (3, 3, True)
        # without l1 only the pair (0, 1) remains; pose 2 stays visible through l2, which adds no pair
        r = f(obs_pose, obs_lm, 3, 4, excluded=[0, 1, 0, 0])
        assert np.array_equal(r["counts"], [[0, 1, 0], [1, 0, 0], [0, 0, 0]])
        assert list(r["n_observed"]) == [1, 1, 1] and (r["n_pairs"], r["n_visible"], r["any"]) == (1, 3, True)
        r = f(obs_pose, obs_lm, 3, 4, excluded=[1, 1, 0, 0])
        assert not r["counts"].any() and list(r["visible"]) == [False, False, True] and not r["any"]


def test_stereo_input_exercises_the_deduplication(og):
    q = _window(og, "s10")
    pairs = set()
    stereo = 0
    for p, l in zip(q.obs_pose, q.obs_landmark):
        stereo += (int(p), int(l)) in pairs
        pairs.add((int(p), int(l)))
    assert stereo > 0 and len(set(q.obs_camera)) == 2
    raw = _covis.raw_pair_count(q.obs_pose, q.obs_landmark, len(q.poses), len(q.landmarks))
    assert not np.array_equal(raw, _covis.of_problem(q)["counts"])


def test_null_arguments_are_rejected(og):
    assert og.lib().okvisgpu_covisibilities(None, None) != 0
    assert "okvisgpu_covisibilities" in og.EXPORTED_SYMBOLS


def test_covisibility_layout_matches_the_header(og, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    fields = [f for f, _ in og.Covisibility._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {",
           '  printf("size %zu\\n", sizeof(okvisgpu_covisibility));']
    src += [f'  printf("{f} %zu\\n", offsetof(okvisgpu_covisibility, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(og.Covisibility)
    for f in fields:
        assert int(got[f]) == getattr(og.Covisibility, f).offset, f


# ---------------------------------------------------------------- GPU
def _solo(ctx, q, excluded=None):
    ctx.set_problems([q.struct])
    return ctx.covisibilities(excluded)[0]


def _bytes(res):
    return tuple(res[k].tobytes() for k in KEYS) + tuple(res[k] for k in SCALARS + ("path",))


def _third(n):
    return (np.arange(n) % 3 == 0).astype(np.uint8)


@pytest.mark.gpu
def test_s10_solo(og, gpu_ctx):
    q = _window(og, "s10")
    assert len(q.landmarks) % 64 == 52  # the last word is partly filled
    res = _solo(gpu_ctx, q)
    _same(res, _covis.of_problem(q))
    _consistent(res)
    assert res["path"] == 0 and res["any"] and res["n_visible"] == 10
    again = gpu_ctx.covisibilities()[0]
    assert _bytes(res) == _bytes(again)


@pytest.mark.gpu
def test_crafted_window_below_one_word(og, gpu_ctx):
    q = _crafted(og)
    assert len(q.landmarks) == 150 and q.obs_landmark.max() == 39 and not (q.obs_pose == 2).any()
    ref = _covis.of_problem(q)
    # landmarks 0..4 are seen from a single pose: they count as observed and add no pair
    single = np.zeros(len(q.landmarks), dtype=np.uint8)
    single[5:] = 1
    only = _covis.of_problem(q, single)
    assert only["n_observed"].sum() == 5 and only["n_visible"] >= 1 and not only["any"]
    res = _solo(gpu_ctx, q)
    _same(res, ref)
    _consistent(res)
    assert res["path"] == 0 and res["any"]
    assert not res["visible"][2] and not res["counts"][2].any() and not res["counts"][:, 2].any()
    assert res["n_observed"].sum() == len(set(zip(q.obs_pose.tolist(), q.obs_landmark.tolist())))
    _same(gpu_ctx.covisibilities(single)[0], only)


@pytest.mark.gpu
def test_exclusion_masks(og, gpu_ctx):
    q = _window(og, "s10")
    n = len(q.landmarks)
    plain = _solo(gpu_ctx, q)
    third = gpu_ctx.covisibilities(_third(n))[0]
    _same(third, _covis.of_problem(q, _third(n)))
    _consistent(third)
    assert third["n_pairs"] > 0 and not np.array_equal(third["counts"], plain["counts"])
    none = gpu_ctx.covisibilities(np.ones(n, dtype=np.uint8))[0]
    assert not none["counts"].any() and not none["n_observed"].any() and not none["visible"].any()
    assert (none["n_pairs"], none["n_visible"], none["any"]) == (0, 0, False)
    assert _bytes(gpu_ctx.covisibilities(np.zeros(n, dtype=np.uint8))[0]) == _bytes(plain)
    assert _bytes(gpu_ctx.covisibilities(None)[0]) == _bytes(plain)


@pytest.mark.gpu
def test_dense_window(og, gpu_ctx):
    q = _window(og, "dense")
    res = _solo(gpu_ctx, q)
    _same(res, _covis.of_problem(q))
    _consistent(res)
    S = len(q.poses)
    print(f"dense: max count {res['counts'].max()}, pairs {res['n_pairs']} of {S * (S - 1) // 2}")
    assert res["path"] == 0 and res["counts"].max() >= 100 and res["n_pairs"] >= 0.9 * S * (S - 1) // 2


@pytest.mark.gpu
def test_tiled_path(og, gpu_ctx):
    q = _window(og, "tiled")
    assert (len(q.poses), len(q.landmarks)) == TILED[:2]
    res = _solo(gpu_ctx, q)
    assert res["path"] == 1
    _same(res, _covis.of_problem(q))
    _consistent(res)
    ex = _third(len(q.landmarks))
    _same(gpu_ctx.covisibilities(ex)[0], _covis.of_problem(q, ex))
    # the same window without its last four landmarks fits the LDS budget: path 0, and the same
    # integers as the tiled path with those four excluded
    cut = (np.arange(len(q.landmarks)) >= TILED_CUT).astype(np.uint8)
    tiled = gpu_ctx.covisibilities(cut)[0]
    small = _window(og, "tiled")
    small.landmarks, small.landmark_constant = small.landmarks[:TILED_CUT], small.landmark_constant[:TILED_CUT]
    _keep_observations(small, small.obs_landmark < TILED_CUT)
    lds = _solo(gpu_ctx, small)
    assert (tiled["path"], lds["path"]) == (1, 0)
    _same(tiled, lds)
    _same(lds, _covis.of_problem(small))


@pytest.mark.gpu
def test_more_states_than_one_pass_of_the_bit_kernel(og, gpu_ctx):
    """k_covis_bits keeps one LDS word per state for 512 states at a time (kBitsStates): 530 states
    take two passes, and a landmark seen from both sides of state 512 resumes its walk in the second."""
    q = _window(og, "s530")
    assert len(q.poses) == 530
    lo, hi = np.zeros(len(q.landmarks), bool), np.zeros(len(q.landmarks), bool)
    lo[q.obs_landmark[q.obs_pose < 512]] = True
    hi[q.obs_landmark[q.obs_pose >= 512]] = True
    assert (lo & hi).sum() >= 10 and (hi & ~lo).any()
    res = _solo(gpu_ctx, q)
    ref = _covis.of_problem(q)
    _same(res, ref)
    _consistent(res)
    assert res["counts"][:512, 512:].any() and res["counts"][512:, 512:].any() and res["n_observed"][512:].any()
    assert not res["visible"].all()  # (three states of this window observe nothing)
    ex = _third(len(q.landmarks))
    _same(gpu_ctx.covisibilities(ex)[0], _covis.of_problem(q, ex))


@pytest.mark.gpu
def test_batch_of_three_windows_equals_the_solo_results(og, gpu_ctx):
    qs = [_window(og, "s10"), _crafted(og), _window(og, "dense")]
    masks = [_third(len(qs[0].landmarks)), None, (np.arange(len(qs[2].landmarks)) % 5 == 1).astype(np.uint8)]
    solo = [_solo(gpu_ctx, q, m) for q, m in zip(qs, masks)]
    gpu_ctx.set_problems([q.struct for q in qs])
    batch = gpu_ctx.covisibilities(masks, n_windows=3)
    for q, m, s, b in zip(qs, masks, solo, batch):
        assert _bytes(s) == _bytes(b)
        _same(b, _covis.of_problem(q, m))


@pytest.mark.gpu
def test_unchanged_by_a_solve_and_changes_nothing(og, gpu_ctx):
    q = _window(og, "s10")
    gpu_ctx.set_problems([q.struct])
    before = gpu_ctx.covisibilities()[0]
    opts = og.default_options(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0,
                              parameter_tolerance=0.0)
    assert gpu_ctx.solve(opts)[0]["num_iterations"] == 3
    cost = gpu_ctx.evaluate()
    arrays = {k: getattr(q, k).tobytes() for k in _ARRAYS}
    after = gpu_ctx.covisibilities()[0]
    assert _bytes(before) == _bytes(after)
    _same(after, _covis.of_problem(q))
    for k in _ARRAYS:
        assert getattr(q, k).tobytes() == arrays[k], k
    assert gpu_ctx.evaluate() == cost


@pytest.mark.gpu
def test_argument_checks(og):
    lib = og.lib()
    ctx = og.Context(0)
    try:
        vs = (og.Covisibility * 1)()
        assert lib.okvisgpu_covisibilities(ctx.h, vs) == ERR_NO_PROBLEM
        q = _window(og, "s10")
        ctx.set_problems([q.struct])
        assert lib.okvisgpu_covisibilities(ctx.h, None) == ERR_INVALID_ARGUMENT
        ctx.solve_begin(og.default_options(max_num_iterations=2))
        try:
            assert lib.okvisgpu_covisibilities(ctx.h, vs) == ERR_INVALID_ARGUMENT
        finally:
            ctx.solve_end()
        # every array pointer may be NULL: the scalars alone
        assert lib.okvisgpu_covisibilities(ctx.h, vs) == 0
        ref = _covis.of_problem(q)
        assert (vs[0].n_pairs, vs[0].n_visible, vs[0].any, vs[0].path) == (ref["n_pairs"], ref["n_visible"], 1, 0)
        # a window without observations: all zeros, nothing launched
        empty = _keep_observations(_window(og, "s6"), np.zeros(0, dtype=np.int64))
        ctx.set_problems([empty.struct])
        res = ctx.covisibilities()[0]
        assert not res["counts"].any() and not res["visible"].any() and not res["any"] and res["n_pairs"] == 0
    finally:
        ctx.close()
