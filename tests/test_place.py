"""okvisgpu_place_match / okvisgpu_place_refine: the descriptor matching (Frontend.cpp:316-345) and the pose
refinement with the evaluation after it (:434-598) of Frontend::verifyRecognisedPlace on the device.

CPU: the struct layouts against the header; the NULL checks through the C ABI; the two formulations of the
matching (tests/_place.py: the serial loops, the first minimum in order) agree exactly on every scene the GPU
tests use; a hand-written match case with its table written out; the Levenberg-Marquardt restatement with the
damped problem solved by QR (`refine_literal`, as Ceres' DENSE_QR) and by the 6x6 normal equations
(`refine_normal`, as the device) give equal integers on every refine scene and doubles within REFINE_BOUND,
and every decision of the loop keeps a relative margin of 1e-6 from its threshold, which is what makes the
exact comparison of the device's integers legitimate; the scenes hold what they are for; a noise-free scene is
refined to its ground truth.
GPU: the device against `match_literal` (all integers, exact) and against `refine_literal` (integers exact,
doubles within REFINE_BOUND); batch independence and run-to-run equality bit for bit; the validation failures.

REFINE_BOUND: the largest deviation of the device's pose, H, initial and final cost from `refine_literal` over
the refine scenes below, pose and costs scaled by max(1, |value|), H by its largest entry per job, measured on
an MI355X: REFINE_MEASURED. The bound is ten times that (the factor covers the Cholesky-against-QR rounding on
other scenes) and may not exceed 1e-6."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _place as pl
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
MARGIN = 1e-6
REFINE_MEASURED = 2.7e-14
REFINE_BOUND = 10 * REFINE_MEASURED
FAR = ((1.35, -1.08, 0.81), (0.405, -0.27, 0.54))


def _descs(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 48), dtype=np.uint8)


def _flip(desc, n, seed):
    return pl.flip_bits(np.random.default_rng(seed), np.asarray(desc, np.uint8), n)


# ------------------------------------------------------------------------------------------ match scenes
def _shapes_scene():
    """Images of 1, 63, 64, 65, 130 and 0 keypoints over two cameras. Jobs: 1 landmark on images (0, 1); 65
    landmarks on (2, 3); 7 on (4, none); 5 on (the empty image, 4); 9 more on (2, 3), shared with job 1.
    Job 0's landmark is 10 bits from the one keypoint of image 0; the other landmarks have 1, 2, 3, 5 or no
    descriptors, a descriptor being a keypoint's with 0-75 bits flipped, or unrelated."""
    sizes = [1, 63, 64, 65, 130, 0]
    images = [_descs(100 + i, n) for i, n in enumerate(sizes)]
    rng = np.random.default_rng(7)

    def landmarks(n, imgs, seed):
        out = []
        for l in range(n):
            nd = (1, 2, 3, 5, 0)[l % 5]
            lm = []
            for d in range(nd):
                src = images[imgs[rng.integers(len(imgs))]]
                if len(src) and rng.random() < 0.8:
                    lm.append(_flip(src[rng.integers(len(src))], int(rng.integers(0, 76)), seed * 1000 + l * 8 + d))
                else:
                    lm.append(_descs(seed * 1000 + l * 8 + d, 1)[0])
            out.append(np.array(lm, np.uint8).reshape(-1, 48))
        return out

    jobs = [((0, 1), [np.array([_flip(images[0][0], 10, 99)])]), ((2, 3), landmarks(65, (2, 3), 2)), ((4, -1), landmarks(7, (4,), 3)),
            ((5, 4), landmarks(5, (4,), 4)), ((2, 3), landmarks(9, (2, 3), 5))]
    return pl.match_scene(2, images, jobs)


def _ties_scene(threshold=60.0):
    """One image of 130 keypoints, one camera, one job. Keypoints 5 and 9 are equal (a tie within a round),
    10 and 100 are equal (across rounds). Landmarks: 0 is 3 bits from 5 / 9; 1 is 4 bits from 10 / 100; 2 has
    two descriptors, the first 7 bits from keypoint 120, the second 7 bits from keypoint 2 (the earlier
    descriptor wins at the larger k); 3 is 59 bits from keypoint 30; 4 is 60 bits from keypoint 31; 5 has two
    descriptors, 20 bits from keypoint 70 and 12 bits from keypoint 3."""
    img = _descs(200, 130)
    img[9], img[100] = img[5], img[10]
    lms = [[_flip(img[5], 3, 1)], [_flip(img[10], 4, 2)], [_flip(img[120], 7, 3), _flip(img[2], 7, 4)],
           [_flip(img[30], 59, 5)], [_flip(img[31], 60, 6)], [_flip(img[70], 20, 7), _flip(img[3], 12, 8)]]
    return pl.match_scene(1, [img], [((0,), [np.array(lm, np.uint8) for lm in lms])], matching_threshold=threshold)


# At 60.5 and 59.5 distMin starts at 60 / 59, which :338 finds below the threshold: the landmarks whose walk
# replaces nothing come out as the reference's untouched (kMin, distMin) = (0, start).
TIES_EXPECTED = {60.0: ([5, 10, 120, 30, -1, 3], [3, 4, 7, 59, -1, 12], 5),
                 60.5: ([5, 10, 120, 30, 0, 3], [3, 4, 7, 59, 60, 12], 6),
                 59.5: ([5, 10, 120, 0, 0, 3], [3, 4, 7, 59, 59, 12], 6)}


def _hand_scene():
    """Two cameras, image 0 with three keypoints A, B, C, image 1 with two, D, E; one job of three landmarks.
    Landmark 0: one descriptor, 2 bits from A; nothing near in camera 1. Landmark 1: descriptors (4 bits from
    C), (4 bits from B): the earlier descriptor's C wins in camera 0, nothing near in camera 1. Landmark 2: no
    descriptor."""
    A, B, Cc, D, E = _descs(300, 5)
    l0 = _flip(A, 2, 1)
    lm1 = np.array([_flip(Cc, 4, 3), _flip(B, 4, 4)], np.uint8)
    return pl.match_scene(2, [np.array([A, B, Cc]), np.array([D, E])],
                          [((0, 1), [np.array([l0]), lm1, np.zeros((0, 48), np.uint8)])])


HAND_EXPECTED = {"match_keypoint": [[0, -1], [2, -1], [-1, -1]], "match_distance": [[2, -1], [4, -1], [-1, -1]],
                 "job_matches": [2]}

MATCH_SCENES = {"shapes": _shapes_scene, "ties": _ties_scene, "ties605": lambda: _ties_scene(60.5),
                "ties595": lambda: _ties_scene(59.5), "hand": _hand_scene}


@functools.lru_cache(maxsize=None)
def match_scene(name):
    s = MATCH_SCENES[name]()
    return s, pl.match_literal(s)


def _match_batch(og, s):
    return og.place_match_batch(**s)


# ------------------------------------------------------------------------------------------ refine scenes
def _main_scene():
    """Jobs of 0, 6, 64, 65 and 257 observations over two of the rig's three cameras (radtan, equidistant, no
    distortion), started close to the optimum; a job started far off (it takes unsuccessful steps); a job
    with 8 gross outliers among 90 observations."""
    return pl.refine_scene([pl.refine_job(1, 0), pl.refine_job(2, 6), pl.refine_job(3, 64, cams=(1, 2)),
                            pl.refine_job(4, 65, cams=(0, 2)), pl.refine_job(5, 257), pl.refine_job(20, 80, start=FAR),
                            pl.refine_job(7, 90, cams=(0, 2), outliers=8)], max_num_iterations=20)


def _capped_scene():
    return pl.refine_scene([pl.refine_job(8, 40, start=((0.5, -0.4, 0.3), (0.15, -0.1, 0.2))), pl.refine_job(9, 30)],
                           max_num_iterations=2)


def _noise_free_scene():
    return pl.refine_scene([pl.refine_job(10, 50, noise=0.0),
                            pl.refine_job(11, 33, cams=(1, 2), noise=0.0, start=((0.5, -0.4, 0.3), (0.15, -0.1, 0.2)))],
                           max_num_iterations=20)


def _plain_scene():
    """No loss (the Corrector's identity) on two small jobs."""
    return pl.refine_scene([pl.refine_job(12, 21, cams=(2, 1)), pl.refine_job(13, 9)], max_num_iterations=10,
                           loss=("none", 1.0))


REFINE_SCENES = {"main": _main_scene, "capped": _capped_scene, "noise_free": _noise_free_scene, "plain": _plain_scene}


@functools.lru_cache(maxsize=None)
def refine_scene(name):
    s = REFINE_SCENES[name]()
    return s, pl.refine_literal(s)


def _refine_batch(og, s):
    pose = np.ascontiguousarray(s["pose"], np.float64).copy()
    b, keep = og.place_refine_batch(cameras=pl.cameras_of(s), extrinsics=s["extrinsics"], pose=pose,
                                    loss=s["loss"], max_num_iterations=s["max_num_iterations"],
                                    **{k: s[k] for k in ("obs_begin", "obs_camera", "obs_keypoint", "obs_sqrt_info",
                                                         "obs_point")})
    return b, keep, pose


# ------------------------------------------------------------------------------------------ CPU
def test_symbols_and_struct_layouts(og, tmp_path):
    """The entry points are declared and exported; the four structs mirror the header."""
    for f in ("okvisgpu_place_match", "okvisgpu_place_refine"):
        assert f in og.EXPORTED_SYMBOLS and hasattr(og.lib(), f)
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    types = {"okvisgpu_place_match_batch": og.PlaceMatchBatch, "okvisgpu_place_match_result": og.PlaceMatchResult,
             "okvisgpu_place_refine_batch": og.PlaceRefineBatch, "okvisgpu_place_refine_result": og.PlaceRefineResult}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {"]
    for t, cls in types.items():
        src.append(f'  printf("{t} %zu\\n", sizeof({t}));')
        for f, _ in cls._fields_:
            src.append(f'  printf("{t}.{f} %zu\\n", offsetof({t}, {f}));')
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for t, cls in types.items():
        assert int(got[t]) == C.sizeof(cls), t
        for f, _ in cls._fields_:
            assert int(got[f"{t}.{f}"]) == getattr(cls, f).offset, (t, f)


def test_null_arguments_are_rejected(og):
    """NULL ctx, batch or result; and with a NULL context no count or index is even looked at."""
    lib = og.lib()
    b, keep = _match_batch(og, match_scene("hand")[0])
    r = og.PlaceMatchResult()
    assert lib.okvisgpu_place_match(None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.okvisgpu_place_match(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
    b.n_jobs = -1
    assert lib.okvisgpu_place_match(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
    b2, keep2, pose = _refine_batch(og, refine_scene("capped")[0])
    r2 = og.PlaceRefineResult()
    assert lib.okvisgpu_place_refine(None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.okvisgpu_place_refine(None, C.byref(b2), C.byref(r2)) == ERR_INVALID_ARGUMENT
    b2.loss.kind = 9
    assert lib.okvisgpu_place_refine(None, C.byref(b2), C.byref(r2)) == ERR_INVALID_ARGUMENT
    assert (pose == refine_scene("capped")[0]["pose"]).all()


@pytest.mark.parametrize("name", sorted(MATCH_SCENES))
def test_match_literal_and_ordered_agree(og, name):
    s, lit = match_scene(name)
    ordered = pl.match_ordered(s)
    for k in pl.MATCH_KEYS:
        assert np.array_equal(lit[k], ordered[k]), k


def _assert_hand(got):
    for k, v in HAND_EXPECTED.items():
        assert np.array_equal(got[k], np.array(v, np.int32)), k


def _assert_ties(got, threshold):
    kp, dist, ctr = TIES_EXPECTED[threshold]
    assert list(got["match_keypoint"][:, 0]) == kp and list(got["match_distance"][:, 0]) == dist
    assert list(got["job_matches"]) == [ctr]


def test_match_hand_written_case(og):
    s, lit = match_scene("hand")
    assert len(s["descriptor"]) == 5 and len(s["old_descriptor"]) == 3
    _assert_hand(lit)
    _assert_hand(pl.match_ordered(s))


def test_match_scenes_hold_what_they_are_for(og):
    s, lit = match_scene("shapes")
    assert list(np.diff(s["kp_begin"])) == [1, 63, 64, 65, 130, 0]
    assert list(np.diff(s["lm_begin"])) == [1, 65, 7, 5, 9] and sorted(set(np.diff(s["desc_begin"]))) == [0, 1, 2, 3, 5]
    assert list(s["job_image"][2]) == [4, -1] and list(s["job_image"][3]) == [5, 4]
    assert list(s["job_image"][1]) == list(s["job_image"][4])
    m = lit["match_keypoint"]
    assert (m[66:73, 1] == -1).all() and (m[73:78, 0] == -1).all()  # no image; an image without keypoints
    assert (m[66:73, 0] >= 64).sum() >= 1 and (m >= 0).sum() >= 40 and (m == -1).sum() >= 40
    assert (lit["job_matches"] > 0).all()
    empty = np.flatnonzero(np.diff(s["desc_begin"]) == 0)
    assert len(empty) >= 10 and (m[empty] == -1).all()
    for thr in TIES_EXPECTED:
        _assert_ties(match_scene({60.0: "ties", 60.5: "ties605", 59.5: "ties595"}[thr])[1], thr)
    s, _ = match_scene("ties")
    table = pl.hamming(s["old_descriptor"], s["descriptor"])
    assert table[0, 5] == table[0, 9] == 3 and table[1, 10] == table[1, 100] == 4
    assert table[2, 120] == table[3, 2] == 7 and table[4, 30] == 59 and table[5, 31] == 60


@pytest.mark.parametrize("name", sorted(REFINE_SCENES))
def test_refine_literal_and_normal_agree(og, oracle, name):
    """QR on the augmented Jacobian and Cholesky on the normal equations: the same decisions, the doubles
    within the bound the device is held to."""
    s, lit = refine_scene(name)
    nrm = pl.refine_normal(s)
    for k in pl.REFINE_INT_KEYS:
        assert np.array_equal(lit[k], nrm[k]), k
    gap = pl.refine_deviation(nrm, lit)
    print(f"{name}: literal against normal {gap:.3e}")
    assert gap < REFINE_BOUND <= 1e-6


@pytest.mark.parametrize("name", sorted(REFINE_SCENES))
def test_refine_scene_margins(og, oracle, name):
    """The three tolerance tests, rel > 1e-3, model_cost_change > 0 and |r| > 3 are each decided by a
    relative margin of at least 1e-6, in both formulations."""
    s, lit = refine_scene(name)
    nrm = pl.refine_normal(s)
    print(f"{name}: margin {lit['margin']:.3e} / {nrm['margin']:.3e}")
    assert lit["margin"] >= MARGIN and nrm["margin"] >= MARGIN
    assert np.isfinite(lit["pose"]).all() and np.isfinite(lit["H"]).all()


def test_refine_scenes_hold_what_they_are_for(og, oracle):
    s, lit = refine_scene("main")
    assert list(np.diff(s["obs_begin"])) == [0, 6, 64, 65, 257, 80, 90]
    assert {int(c) for j in (1, 4) for c in s["obs_camera"][s["obs_begin"][j]:s["obs_begin"][j + 1]]} == {0, 1}
    assert {int(c) for c in s["obs_camera"][s["obs_begin"][2]:s["obs_begin"][3]]} == {1, 2}
    assert [c["distortion"] for c in s["cameras"]] == [1, 2, 0]
    assert (lit["termination_type"] == pl.CONVERGENCE).all()
    assert lit["num_iterations"][0] == 0 and (lit["pose"][0] == s["pose"][0]).all() and not lit["H"][0].any()
    assert lit["initial_cost"][0] == lit["final_cost"][0] == 0.0 and lit["num_successful_steps"][0] == 1
    assert (2 <= lit["num_iterations"][1:5]).all() and (lit["num_iterations"][1:5] <= 5).all()
    assert (lit["num_unsuccessful_steps"][1:5] == 0).all() and lit["num_unsuccessful_steps"][5] >= 1
    assert lit["n_outliers"][6] == 8 and (lit["n_outliers"][:6] == 0).all()
    assert np.abs(lit["pose"][1:] - s["truth"][1:]).max() < 0.02  # the Cauchy loss keeps the solve on the inliers
    s, lit = refine_scene("capped")
    assert (lit["num_iterations"] == 2).all() and (lit["termination_type"] == pl.NO_CONVERGENCE).all()
    assert (lit["final_cost"] < lit["initial_cost"]).all()


def test_refine_noise_free_scene_reaches_the_ground_truth(og, oracle):
    """Ceres stops on the parameter tolerance without taking the last step, of at most 1e-8 (|x| + 1e-8)."""
    s, lit = refine_scene("noise_free")
    assert (lit["termination_type"] == pl.CONVERGENCE).all() and (lit["n_outliers"] == 0).all()
    assert np.abs(lit["pose"] - s["truth"]).max() < 1e-7
    assert np.abs(s["pose"] - s["truth"]).max() > 0.01


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MATCH_SCENES))
def test_gpu_match_scene(og, gpu_ctx, name):
    """Every scene against `match_literal`, the outputs pre-filled so that an element left unwritten shows."""
    s, lit = match_scene(name)
    b, keep = _match_batch(og, s)
    got = gpu_ctx.place_match(b, fill={k: 77 for k in pl.MATCH_KEYS})
    for k in pl.MATCH_KEYS:
        assert np.array_equal(got[k], lit[k]), (name, k)
    if name == "hand":
        _assert_hand(got)
    if name.startswith("ties"):
        _assert_ties(got, float(s["matching_threshold"]))


@pytest.mark.gpu
def test_gpu_match_batch_independence_and_determinism(og, gpu_ctx):
    """A job alone, among others and in the full batch: identical bytes. Two runs: identical bytes. n_jobs = 0
    gives empty arrays; NULL outputs are accepted."""
    s, _ = match_scene("shapes")
    run = lambda t: gpu_ctx.place_match(_match_batch(og, t)[0])
    full, again = run(s), run(s)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for j in (1, 4):
        alone, three = pl.match_sub_scene(s, [j]), pl.match_sub_scene(s, [0, j, 3])
        a, b, c = run(alone), run(three), pl.match_job_rows(s, full, j)
        for k, v in pl.match_job_rows(alone, a, 0).items():
            assert v.tobytes() == pl.match_job_rows(three, b, 1)[k].tobytes() == c[k].tobytes(), (j, k)
    got = run(pl.match_sub_scene(s, []))
    assert all(got[k].size == 0 for k in pl.MATCH_KEYS)
    b, keep = _match_batch(og, s)
    r = og.PlaceMatchResult()
    assert og.lib().okvisgpu_place_match(gpu_ctx.h, C.byref(b), C.byref(r)) == 0
    ctr = np.full(5, 77, np.int32)
    r.job_matches = ctr.ctypes.data_as(C.POINTER(C.c_int32))
    assert og.lib().okvisgpu_place_match(gpu_ctx.h, C.byref(b), C.byref(r)) == 0
    assert np.array_equal(ctr, full["job_matches"])


def _refused(og, ctx, call, b, r, outs, match):
    rc = call(ctx.h, C.byref(b), C.byref(r))
    assert rc == ERR_INVALID_ARGUMENT
    assert match in og.lib().okvisgpu_last_error(ctx.h).decode(), og.lib().okvisgpu_last_error(ctx.h).decode()
    for k, (a, sentinel) in outs.items():
        assert (a == sentinel).all(), k


@pytest.mark.gpu
def test_gpu_match_argument_errors(og, gpu_ctx):
    """Each listed cause is refused with OKVISGPU_ERR_INVALID_ARGUMENT and leaves the sentinel-filled outputs
    alone; so is a call between solve_begin and solve_end."""
    s, lit = match_scene("hand")

    def refused(change, match, field=None):
        t = dict(s)
        for k, (i, v) in change.items():
            t[k] = np.array(s[k]).copy()
            t[k].reshape(-1)[i] = v
        b, keep = _match_batch(og, t)
        if field:
            setattr(b, *field)
        r = og.PlaceMatchResult()
        outs = {k: (np.full(lit[k].shape, 77, np.int32), 77) for k in pl.MATCH_KEYS}
        for k, (a, _) in outs.items():
            setattr(r, k, a.ctypes.data_as(C.POINTER(C.c_int32)))
        _refused(og, gpu_ctx, og.lib().okvisgpu_place_match, b, r, outs, match)

    b, keep = _match_batch(og, s)
    assert og.lib().okvisgpu_place_match(gpu_ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
    assert og.lib().okvisgpu_place_match(gpu_ctx.h, None, C.byref(og.PlaceMatchResult())) == ERR_INVALID_ARGUMENT
    refused({"job_image": (1, 2)}, "job_image")
    refused({"job_image": (0, -2)}, "job_image")
    refused({"kp_begin": (0, 1)}, "kp_begin")
    refused({"kp_begin": (1, 9)}, "kp_begin")
    refused({"lm_begin": (0, 1)}, "lm_begin")
    refused({"desc_begin": (2, 0)}, "desc_begin")
    refused({}, "negative", field=("n_cameras", -1))
    refused({}, "negative", field=("n_images", -1))
    refused({}, "missing", field=("old_descriptor", None))
    refused({}, "missing", field=("lm_begin", None))
    w = og.SynthWindow(10, 500, 4000, seed=78)
    gpu_ctx.set_problems([w.problem])
    gpu_ctx.solve_begin(og.default_options(max_num_iterations=2))
    try:
        refused({}, "solve_end")
    finally:
        gpu_ctx.solve_end()
    _assert_hand(gpu_ctx.place_match(_match_batch(og, s)[0]))


def _run_refine(og, ctx, s, fill=None):
    b, keep, pose = _refine_batch(og, s)
    got = ctx.place_refine(b, fill=fill)
    got["pose"] = pose
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REFINE_SCENES))
def test_gpu_refine_scene(og, oracle, gpu_ctx, parity, name):
    """The device against `refine_literal`: the iterations, both step counts, the termination type and the
    outlier count exact; pose, H and both costs within REFINE_BOUND."""
    s, lit = refine_scene(name)
    got = _run_refine(og, gpu_ctx, s, fill={k: 77 for k in pl.REFINE_INT_KEYS + pl.REFINE_REAL_KEYS})
    for k in pl.REFINE_INT_KEYS:
        print(k, got[k], lit[k])
    dev = pl.refine_deviation(got, lit)
    print(f"place_refine/{name}: deviation {dev:.3e}")
    for k in pl.REFINE_INT_KEYS:
        assert np.array_equal(got[k], lit[k]), (name, k)
    parity(f"place_refine/{name}", dev, REFINE_BOUND)


@pytest.mark.gpu
def test_gpu_refine_batch_independence_and_determinism(og, oracle, gpu_ctx):
    """A job alone against the same job in the batch, and two runs: identical bytes. n_jobs = 0 is valid and
    NULL outputs are accepted."""
    s, _ = refine_scene("main")
    full, again = _run_refine(og, gpu_ctx, s), _run_refine(og, gpu_ctx, s)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for j in (3, 5):
        alone = _run_refine(og, gpu_ctx, pl.refine_sub_scene(s, [j]))
        three = _run_refine(og, gpu_ctx, pl.refine_sub_scene(s, [6, j, 0]))
        for k in full:
            assert alone[k][0].tobytes() == three[k][1].tobytes() == full[k][j].tobytes(), (j, k)
    got = _run_refine(og, gpu_ctx, pl.refine_sub_scene(s, []))
    assert all(v.size == 0 for v in got.values())
    b, keep, pose = _refine_batch(og, s)
    r = og.PlaceRefineResult()
    assert og.lib().okvisgpu_place_refine(gpu_ctx.h, C.byref(b), C.byref(r)) == 0
    assert pose.tobytes() == full["pose"].tobytes()


@pytest.mark.gpu
def test_gpu_refine_failure_on_a_non_finite_start(og, oracle, gpu_ctx):
    """A NaN landmark: OKVISGPU_FAILURE, 0 iterations, the pose untouched; the other job is not affected."""
    s0, lit0 = refine_scene("capped")
    s = dict(s0)
    s["obs_point"] = s0["obs_point"].copy()
    s["obs_point"][3, 1] = np.nan
    lit = pl.refine_literal(s)
    got = _run_refine(og, gpu_ctx, s)
    for g in (lit, got):
        assert g["termination_type"][0] == pl.FAILURE and g["num_iterations"][0] == 0
        assert g["pose"][0].tobytes() == s["pose"][0].tobytes() and np.isnan(g["initial_cost"][0])
    for k in pl.REFINE_INT_KEYS:
        assert np.array_equal(got[k], lit[k]), k
    clean = _run_refine(og, gpu_ctx, s0)
    for k in clean:
        assert clean[k][1].tobytes() == got[k][1].tobytes(), k


@pytest.mark.gpu
def test_gpu_refine_argument_errors(og, oracle, gpu_ctx):
    """Each listed cause is refused with OKVISGPU_ERR_INVALID_ARGUMENT and leaves the poses and the
    sentinel-filled outputs alone; so is a call between solve_begin and solve_end."""
    s, lit = refine_scene("capped")
    n = len(s["pose"])

    def refused(change, match, field=None, loss=None):
        t = dict(s)
        for k, (i, v) in change.items():
            t[k] = np.array(s[k]).copy()
            t[k].reshape(-1)[i] = v
        b, keep, pose = _refine_batch(og, t)
        if field:
            setattr(b, *field)
        if loss:
            b.loss = og.Loss(*loss)
        r = og.PlaceRefineResult()
        outs = {"pose": (pose, pose.copy())}
        for k in pl.REFINE_INT_KEYS + ("H", "initial_cost", "final_cost"):
            dt = np.int32 if k in pl.REFINE_INT_KEYS else np.float64
            a = np.full((n, 36) if k == "H" else (n,), 77, dt)
            outs[k] = (a, 77)
            setattr(r, k, a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dt))))
        _refused(og, gpu_ctx, og.lib().okvisgpu_place_refine, b, r, outs, match)

    b, keep, pose = _refine_batch(og, s)
    assert og.lib().okvisgpu_place_refine(gpu_ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
    assert og.lib().okvisgpu_place_refine(gpu_ctx.h, None, C.byref(og.PlaceRefineResult())) == ERR_INVALID_ARGUMENT
    refused({"obs_camera": (4, 3)}, "obs_camera")
    refused({"obs_camera": (0, -1)}, "obs_camera")
    refused({"obs_begin": (0, 2)}, "obs_begin")
    refused({"obs_begin": (1, 99)}, "obs_begin")
    refused({}, "negative", field=("n_cameras", -1))
    refused({}, "negative", field=("max_num_iterations", -1))
    refused({}, "missing", field=("obs_point", None))
    refused({}, "missing", field=("pose", None))
    refused({}, "missing", field=("cameras", None))
    refused({}, "loss kind", loss=(7, 0, 3.0, 0.0))
    refused({}, "loss scale", loss=(1, 0, 0.0, 0.0))
    refused({}, "loss scale", loss=(1, 0, -3.0, 0.0))
    w = og.SynthWindow(10, 500, 4000, seed=78)
    gpu_ctx.set_problems([w.problem])
    gpu_ctx.solve_begin(og.default_options(max_num_iterations=2))
    try:
        refused({}, "solve_end")
    finally:
        gpu_ctx.solve_end()
    got = _run_refine(og, gpu_ctx, s)
    for k in pl.REFINE_INT_KEYS:
        assert np.array_equal(got[k], lit[k]), k
