"""okvisgpu_update_landmarks: ViGraph::updateLandmarks (ViGraph.cpp:1762-1841) and
ViGraph::areLandmarksInFrontOfCameras (:1621-1642) on the device, after a solve.

CPU: the numpy restatement (tests/_landmarks.py) on hand-built cases, the entry point's NULL check
and the struct layout. GPU: the device pass against the restatement. Every estimate of the GPU tests
comes from a 10-iteration oracle solve on the CPU, written into the host arrays and uploaded with
set_problems, so a difference is the landmark pass's and not the solver's. The restatement takes the
oracle's residual norms; a landmark with a decision closer than 1e-9 to its threshold is left out of
the flag and position comparisons (none is, on these inputs: the smallest margin is 2e-6), and at
most 1 % of a window's landmarks may be left out."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _landmarks as lmk
from _paths import REPO
from _problem import _ARRAYS, OwnedProblem

ERR_INVALID_ARGUMENT, ERR_NO_PROBLEM = 1, 5
IDENT = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


# ---------------------------------------------------------------- CPU: the restatement itself
def _tiny(landmark, cams_x=(0.0, 1.0), err=0.5):
    poses = np.array([[x, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] for x in cams_x])
    n = len(cams_x)
    return lmk.update_landmarks(poses, np.array([IDENT]), np.array([landmark]), np.arange(n), np.zeros(n, dtype=int),
                                np.zeros(n, dtype=int), np.full(n, err))


def test_restatement_two_rays_give_the_analytic_quality():
    """Two unit rays at angle theta: the deviations from the mean are +-(d1 - d2) / 2, so
    quality = |d1 - d2| / sqrt(2) = sqrt(2) sin(theta / 2)."""
    ref = _tiny([0.5, 0.0, 2.0, 1.0])
    half = np.arctan2(0.5, 2.0)  # theta / 2
    assert abs(ref["quality"][0] - np.sqrt(2.0) * np.sin(half)) < 1e-15
    assert ref["initialised"][0] and not ref["reset"][0] and ref["in_front"]
    assert np.array_equal(ref["landmarks"][0], [0.5, 0.0, 2.0, 1.0])
    # the same landmark in other homogeneous scalings
    for s in (3.0, -2.0):
        assert abs(_tiny([0.5 * s, 0.0, 2.0 * s, s])["quality"][0] - ref["quality"][0]) < 1e-15
    # an observation over the error gate is left out: one ray remains
    two = lmk.update_landmarks(np.array([IDENT, [1.0, 0, 0, 0, 0, 0, 1.0]]), np.array([IDENT]),
                               np.array([[0.5, 0.0, 2.0, 1.0]]), np.arange(2), np.zeros(2, dtype=int),
                               np.zeros(2, dtype=int), np.array([0.5, 2.6]))
    assert two["quality"][0] == 0.0 and not two["initialised"][0] and list(two["skip"]) == [False, True]


def test_restatement_single_observation_has_quality_zero():
    ref = _tiny([0.3, -0.2, 4.0, 1.0], cams_x=(0.0,))
    assert ref["quality"][0] == 0.0 and not ref["initialised"][0] and not ref["reset"][0]
    # no observation at all: untouched, quality 0
    none = lmk.update_landmarks(np.array([IDENT]), np.array([IDENT]), np.array([[1.0, 2.0, 3.0, 1.0]]),
                                np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0, dtype=int), np.zeros(0))
    assert none["quality"][0] == 0.0 and not none["initialised"][0] and not none["reset"][0] and none["in_front"]


def test_restatement_reset_distance_is_the_four_vector_norm():
    """A point 0.05 m along a ray is behind the 0.1 m plane; it is re-placed on that ray at
    max(0.1, |[x y z 1]|) = sqrt(1 + 0.05^2): the reference's norm includes w."""
    ray = np.array([0.3, -0.2, 1.0])
    ray /= np.linalg.norm(ray)
    ref = _tiny([*(0.05 * ray), 1.0], cams_x=(0.0,))
    assert ref["reset"][0] and not ref["initialised"][0] and not ref["in_front"]
    assert abs(ref["reset_distance"][0] - np.sqrt(1.0 + 0.05 ** 2)) < 1e-15
    assert np.allclose(ref["landmarks"][0], [*(np.sqrt(1.0 + 0.05 ** 2) * ray), 1.0], rtol=0, atol=1e-15)
    # behind the camera: the ray is reversed, the landmark lands in front
    back = _tiny([*(-0.5 * ray), 1.0], cams_x=(0.0,))
    assert back["reset"][0] and np.allclose(back["landmarks"][0][:3], np.sqrt(1.25) * ray, rtol=0, atol=1e-15)


def test_null_arguments_are_rejected(og):
    assert og.lib().okvisgpu_update_landmarks(None, None) != 0
    assert "okvisgpu_update_landmarks" in og.EXPORTED_SYMBOLS


def test_landmark_update_layout_matches_the_header(og, tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    fields = [f for f, _ in og.LandmarkUpdate._fields_]
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {",
           '  printf("size %zu\\n", sizeof(okvisgpu_landmark_update));']
    src += [f'  printf("{f} %zu\\n", offsetof(okvisgpu_landmark_update, {f}));' for f in fields]
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(og.LandmarkUpdate)
    for f in fields:
        assert int(got[f]) == getattr(og.LandmarkUpdate, f).offset, f


# ---------------------------------------------------------------- GPU: inputs, computed once
_CACHE = {}


def _solved(og, oracle, key, make):
    """An OwnedProblem holding the estimates of a 10-iteration oracle solve (computed once, never
    modified: the tests work on copies)."""
    if key not in _CACHE:
        q = make()
        oracle.solve(q.ptr(), og.default_options(max_num_iterations=10))
        _CACHE[key] = q
    return OwnedProblem.copy_of(_CACHE[key].struct)


def _s10(og, oracle):
    return _solved(og, oracle, "s10", lambda: OwnedProblem.copy_of(og.SynthWindow(10, 500, 4000, seed=20251015).problem))


def _small_with_constants(og, oracle):
    def make():
        q = OwnedProblem.copy_of(og.SynthWindow(6, 150, 1000, seed=3).problem)
        q.landmark_constant = np.zeros(len(q.landmarks), dtype=np.uint8)
        q.landmark_constant[::5] = 1
        return q.bind()
    return _solved(og, oracle, "small", make)


def _crafted(og, oracle):
    """S10 after the oracle solve with landmark l edited by l % 7, relative to the camera centre c of
    its first observation and the ray v from c to it: 0 very close in front, 1 behind the camera,
    2 far, 3 negative w, 4 a direction (w = 0), 5 and 6 untouched."""
    q = _s10(og, oracle)
    _, r_WC = lmk.camera_frames(q.poses, q.extrinsics)
    for l, run in enumerate(lmk.observation_order(q.obs_pose, q.obs_landmark, q.obs_camera, len(q.landmarks))):
        if not run:
            continue
        c = r_WC[q.obs_pose[run[0]], q.obs_camera[run[0]]]
        hp = q.landmarks[l].copy()
        v = hp[:3] / hp[3] - c
        n = np.linalg.norm(v)
        kind = l % 7
        if kind == 0:
            q.landmarks[l] = [*(c + v * 0.05 / n), 1.0]
        elif kind == 1:
            q.landmarks[l] = [*(c - v * 0.5 / n), 1.0]
        elif kind == 2:
            q.landmarks[l] = [*(c + 200.0 * v), 1.0]
        elif kind == 3:
            q.landmarks[l] = hp * -2.0
        elif kind == 4:
            q.landmarks[l] = [*(v / n), 0.0]
    return q


def _reference(oracle, q):
    """The restatement on q's current host values, with the oracle's residual norms."""
    r, _, _ = oracle.eval_reprojection(q.ptr(), len(q.obs_pose))
    err = np.linalg.norm(r, axis=1)
    ref = lmk.update_landmarks(q.poses, q.extrinsics, q.landmarks, q.obs_pose, q.obs_landmark, q.obs_camera, err)
    ref["err"] = err
    return ref


def _arrays(q):
    return {k: getattr(q, k).copy() for k in _ARRAYS}


def _compare(q, before, res, ref, errors=True):
    """One window's outputs and its host arrays after the call against the restatement."""
    ok = lmk.decided(ref)
    left_out = 1.0 - ok.mean()
    print(f"left out {left_out:.4f} of {len(ok)} landmarks, smallest margin {ref['margin'].min():.3e}; "
          f"initialised {res['n_initialised']} / {ref['n_initialised']}, reset {res['n_reset']} / {ref['n_reset']}, "
          f"over 2.5: {int((res['obs_error'] > 2.5).sum())} / {int(ref['skip'].sum())}")
    assert left_out <= 0.01
    assert np.array_equal(res["initialised"][ok], ref["initialised"][ok])
    assert np.array_equal(res["reset"][ok], ref["reset"][ok])
    dq = np.abs(res["quality"] - ref["quality"])[ok]
    print(f"quality: max abs deviation {dq.max():.3e}")
    assert np.all(np.isfinite(res["quality"])) and dq.max() <= 1e-12
    assert res["n_initialised"] == int(res["initialised"].sum()) and res["n_reset"] == int(res["reset"].sum())
    if ok.all():
        assert res["n_initialised"] == ref["n_initialised"] and res["n_reset"] == ref["n_reset"]
        assert res["in_front"] == ref["in_front"]
    # the skip decision per observation, and the residual norms where they are compared
    obs_ok = ok[q.obs_landmark]
    assert np.array_equal((res["obs_error"] > 2.5)[obs_ok], ref["skip"][obs_ok])
    if errors:
        de = np.abs(res["obs_error"] - ref["err"]) / np.maximum(1.0, ref["err"])
        print(f"obs_error: max scaled deviation {de.max():.3e}")
        assert de.max() <= 1e-11
    # the caller's arrays: only re-placed landmarks change, to [x y z 1] on the best ray
    for k, a in before.items():
        b = getattr(q, k)
        if k != "landmarks":
            assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), k
    keep = ~res["reset"]
    assert before["landmarks"][keep].tobytes() == q.landmarks[keep].tobytes()
    both = res["reset"] & ok
    if both.any():
        new, want = q.landmarks[both], ref["landmarks"][both]
        dp = np.abs(new - want).max(axis=1) / np.maximum(1.0, np.linalg.norm(want[:, :3], axis=1))
        print(f"reset positions: max scaled deviation {dp.max():.3e}")
        assert np.all(new[:, 3] == 1.0) and dp.max() <= 1e-12


def _solo(ctx, q):
    before = _arrays(q)
    ctx.set_problems([q.struct])
    return before, ctx.update_landmarks()[0]


@pytest.mark.gpu
def test_s10_after_the_oracle_solve(og, oracle, gpu_ctx):
    q = _s10(og, oracle)
    ref = _reference(oracle, q)
    assert (ref["n_initialised"], ref["n_reset"], int(ref["skip"].sum())) == (107, 1, 207)
    assert lmk.decided(ref).all()
    before, res = _solo(gpu_ctx, q)
    _compare(q, before, res, ref)
    assert (res["n_initialised"], res["n_reset"], int((res["obs_error"] > 2.5).sum())) == (107, 1, 207)
    # deterministic: a second upload of the same values gives the same bits
    q2 = _s10(og, oracle)
    _, res2 = _solo(gpu_ctx, q2)
    for k in ("quality", "initialised", "reset", "obs_error"):
        assert res[k].tobytes() == res2[k].tobytes(), k
    assert q.landmarks.tobytes() == q2.landmarks.tobytes()
    # the device holds the re-placed landmarks: reading the parameters back changes nothing
    after = q2.landmarks.copy()
    gpu_ctx.get_params()
    assert after.tobytes() == q2.landmarks.tobytes()


@pytest.mark.gpu
def test_crafted_branches(og, oracle, gpu_ctx):
    q = _crafted(og, oracle)
    ref = _reference(oracle, q)
    kind = np.arange(len(q.landmarks)) % 7
    assert [int(ref["reset"][kind == k].sum()) for k in range(7)] == [71, 69, 0, 0, 0, 0, 1]
    assert np.all(np.isfinite(ref["quality"])) and np.all(np.isfinite(ref["landmarks"]))
    before, res = _solo(gpu_ctx, q)
    # (residual norms are ill-conditioned next to z = 0: the skip decisions are compared, not the values)
    _compare(q, before, res, ref, errors=False)
    assert np.all(np.isfinite(res["quality"])) and np.all(np.isfinite(res["obs_error"])) and np.all(np.isfinite(q.landmarks))
    assert [int(res["reset"][kind == k].sum()) for k in range(7)] == [71, 69, 0, 0, 0, 0, 1]
    # kind 0 sat 0.05 m from its camera: it is re-placed at |[x y z 1]| = sqrt(1 + 0.05^2) = 1.00125 m
    _, r_WC = lmk.camera_frames(q.poses, q.extrinsics)
    runs = lmk.observation_order(q.obs_pose, q.obs_landmark, q.obs_camera, len(q.landmarks))
    for l in np.flatnonzero(res["reset"] & (kind == 0)):
        centres = np.array([r_WC[q.obs_pose[o], q.obs_camera[o]] for o in runs[l]])
        d = np.linalg.norm(centres - q.landmarks[l, :3], axis=1)
        assert np.abs(d - np.sqrt(1.0 + 0.05 ** 2)).min() <= 1e-9, l
        assert abs(ref["reset_distance"][l] - 1.00125) < 1e-5
    # the device holds what the host arrays hold now: the cost of the device values is, bit for bit,
    # the cost after uploading the host arrays again
    on_device = gpu_ctx.evaluate()
    gpu_ctx.update_params()
    assert on_device == gpu_ctx.evaluate() and np.isfinite(on_device)


@pytest.mark.gpu
def test_batch_of_three_windows_equals_the_solo_results(og, oracle, gpu_ctx):
    makers = (_s10, _small_with_constants, _crafted)
    solo = []
    for make in makers:
        q = make(og, oracle)
        _, res = _solo(gpu_ctx, q)
        solo.append((q, res))
    batch = [make(og, oracle) for make in makers]
    before = [_arrays(q) for q in batch]
    gpu_ctx.set_problems([q.struct for q in batch])
    out = gpu_ctx.update_landmarks(n_windows=3)
    for (qs, rs), qb, rb in zip(solo, batch, out):
        for k in ("quality", "initialised", "reset", "obs_error"):
            assert rs[k].tobytes() == rb[k].tobytes(), k
        assert (rs["n_initialised"], rs["n_reset"], rs["in_front"]) == (rb["n_initialised"], rb["n_reset"], rb["in_front"])
        assert qs.landmarks.tobytes() == qb.landmarks.tobytes()
    # the window with constant landmarks against the restatement (constant landmarks like any other)
    q = _small_with_constants(og, oracle)
    _compare(batch[1], before[1], out[1], _reference(oracle, q))


@pytest.mark.gpu
def test_variable_extrinsics_are_read_from_their_blocks(og, oracle, gpu_ctx):
    q = _solved(og, oracle, "extr", lambda: OwnedProblem.copy_of(
        og.SynthWindow(10, 500, 4000, seed=51, do_extrinsics=1).problem))
    assert not q.extrinsics_constant.any()
    # perturb the host T_SC before the upload: the pass must see these values, not the build's copy
    rng = np.random.default_rng(7)
    q.extrinsics[:, :3] += rng.normal(0.0, 2e-3, (len(q.extrinsics), 3))
    q.extrinsics[:, 3:] += rng.normal(0.0, 2e-3, (len(q.extrinsics), 4))
    q.extrinsics[:, 3:] /= np.linalg.norm(q.extrinsics[:, 3:], axis=1, keepdims=True)
    ref = _reference(oracle, q)
    before = _arrays(q)
    gpu_ctx.set_problems([q.struct])
    res = gpu_ctx.update_landmarks()[0]
    _compare(q, before, res, ref)


@pytest.mark.gpu
def test_after_a_gpu_solve_without_a_new_upload(og, oracle, gpu_ctx):
    w = og.SynthWindow(10, 500, 4000, seed=20251015)
    q = OwnedProblem.copy_of(w.problem)
    opts = og.default_options(max_num_iterations=6, function_tolerance=0.0, gradient_tolerance=0.0,
                              parameter_tolerance=0.0)
    gpu_ctx.set_problems([q.struct])
    assert gpu_ctx.solve(opts)[0]["num_iterations"] == 6
    ref = _reference(oracle, q)  # on the values the solve wrote back
    before = _arrays(q)
    res = gpu_ctx.update_landmarks()[0]
    _compare(q, before, res, ref)
    # the device's current values carry the re-placed landmarks ...
    after = q.landmarks.copy()
    gpu_ctx.get_params()
    assert after.tobytes() == q.landmarks.tobytes()
    # ... and the next solve starts from them
    gpu_ctx.update_params()
    cost = gpu_ctx.evaluate()
    s = gpu_ctx.solve(og.default_options(max_num_iterations=1))[0]
    print(f"initial cost {s['initial_cost']!r} evaluate {cost!r}")
    assert abs(s["initial_cost"] - cost) <= 1e-12 * abs(cost)


@pytest.mark.gpu
def test_argument_checks(og, oracle):
    lib = og.lib()
    ctx = og.Context(0)
    try:
        ups = (og.LandmarkUpdate * 1)()
        assert lib.okvisgpu_update_landmarks(ctx.h, ups) == ERR_NO_PROBLEM
        q = _s10(og, oracle)
        ctx.set_problems([q.struct])
        assert lib.okvisgpu_update_landmarks(ctx.h, None) == ERR_INVALID_ARGUMENT
        ctx.solve_begin(og.default_options(max_num_iterations=2))
        try:
            assert lib.okvisgpu_update_landmarks(ctx.h, ups) == ERR_INVALID_ARGUMENT
        finally:
            ctx.solve_end()
        # every output array may be NULL: the counts alone
        assert lib.okvisgpu_update_landmarks(ctx.h, ups) == 0
        assert ups[0].n_initialised > 0 and ups[0].reserved == 0
    finally:
        ctx.close()
