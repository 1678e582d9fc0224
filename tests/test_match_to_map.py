"""okvisgpu_match_to_map: the matching of Frontend::matchToMap (Frontend.cpp:1299-1956) on the device.

CPU: the numpy restatement (tests/_match.py) in its two formulations, the reference's serial loops
(`literal`) and first-minimum / strict-prefix-minima (`ordered`), agree exactly on every scene the GPU
tests use; every scene decides each floating-point comparison with a margin >= 1e-9, which makes the
exact comparison of the device's decisions legitimate; the window scenes reach every branch; a
hand-written case with its tables written out; the struct layouts and the NULL checks.
GPU: the device against `literal`: integers equal, doubles within 1e-9 max(1, |value|)."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _match as mt
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
MARGIN = 1e-9
BOUND = 1e-9
IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


def _bits(*byte_values):
    """A 48-byte descriptor from {byte index: value}."""
    d = np.zeros(48, np.uint8)
    for i, v in byte_values:
        d[i] = v
    return d


def _flip(desc, n, seed):
    return mt.flip_bits(np.random.default_rng(seed), np.asarray(desc, np.uint8), n)


def _window_scene(loop_closure):
    import okvisgpu as og
    w = og.SynthWindow(6, 150, 1000, seed=3)
    p = w.problem
    cams = [{"distortion": q.distortion, "width": q.width, "height": q.height, "fu": q.fu, "fv": q.fv, "cu": q.cu,
             "cv": q.cv, "dist": list(q.dist)} for q in (p.cameras[c] for c in range(p.n_cameras))]
    gt_poses, gt_landmarks, _ = w.ground_truth()
    arr = lambda ptr: np.ctypeslib.as_array(ptr, shape=(p.n_observations,)).copy()
    return mt.build_scene(gt_poses, gt_landmarks, w.true_extrinsics(), cams, arr(p.obs_pose), arr(p.obs_landmark),
                          arr(p.obs_camera), seed=3, loop_closure=loop_closure)


def _hand_scene():
    """Five map landmarks around an identity camera (f = 400, 640 x 480, centre (320, 240), T_SC
    = identity, reprThreshold = 3 + 400 * 0.06 = 27), map poses at x = -0.5 and x = +0.5, the current
    pose at the origin. A (0, 0, 5) is 3D and projects to (320, 240); B (1, 0, 5) is not 3D and
    projects to (400, 240); C (0, 0, -5) is behind inside the image; D has no observation; E projects
    800 px right of the centre. Job 0 is pass 0 and job 1 pass 1 over the same five keypoints."""
    cam = {"distortion": 0, "width": 640, "height": 480, "fu": 400.0, "fv": 400.0, "cu": 320.0, "cv": 240.0,
           "dist": [0.0] * 8}
    poses = np.array([[-0.5, 0, 0, 0, 0, 0, 1], [0.5, 0, 0, 0, 0, 0, 1]], np.float64)
    A0, A1 = _bits((0, 0xFF)), _bits()
    B0 = _bits(*[(i, 0xFF) for i in range(12, 24)])
    B1 = _bits(*[(i, 0xFF) for i in range(12, 24)], (24, 0x1F))
    landmarks = np.array([[0, 0, 5, 1], [1, 0, 5, 1], [0, 0, -5, 1], [0, 0, 5, 1], [2, 0, 1, 1]], np.float64)
    ray = lambda l, p: landmarks[l, :3] - poses[p, :3]
    kp_desc = [_bits((10, 0x07)),                     # 3 from A1, 11 from A0
               _bits((0, 0xFF), (10, 0x03)),          # 10 from A1, 2 from A0
               _bits(*[(i, 0xFF) for i in range(12, 24)], (24, 0x1F), (30, 0x03)),  # 2 from B1, 7 from B0
               _bits(),                               # A1 itself, 40 px below A's projection
               _bits()]                               # A1 itself, carrying A
    return {"poses": poses, "cameras": [cam], "extrinsics": IDENT[None].copy(), "landmarks": landmarks,
            "landmark_quality": np.array([0.5, 1e-5, 0.5, 0.5, 0.5]), "landmark_use": None,
            "obs_begin": np.array([0, 2, 4, 5, 5, 5], np.int32), "obs_pose": np.array([0, 1, 0, 1, 0], np.int32),
            "obs_camera": np.zeros(5, np.int32), "obs_descriptor": np.array([A0, A1, B0, B1, _bits((40, 1))]),
            "obs_ray": np.array([ray(0, 0), ray(0, 1), ray(1, 0), ray(1, 1), -ray(2, 0)]) * [[1.0], [2.0], [0.5], [0.2], [1.0]],
            "imu_use": True, "loop_closure": False, "matching_threshold": 60.0,
            "job_camera": np.array([0, 0], np.int32), "job_pass": np.array([0, 1], np.int32),
            "job_pose_prepare": np.tile(IDENT, (2, 1)), "job_pose_match": np.tile(IDENT, (2, 1)),
            "kp_begin": np.array([0, 5, 10], np.int32),
            "keypoint": np.tile(np.array([[322, 241], [322, 241], [400, 240], [320, 280], [320, 240]], np.float64), (2, 1)),
            "descriptor": np.array(kp_desc * 2), "ray": np.tile(np.array([[0.005, 0.0025, 1], [0.005, 0.0025, 1],
                                                                           [0.2, 0, 1], [0, 0.1, 1], [0, 0, 1]]), (2, 1)),
            "ray_valid": np.ones(10, np.uint8), "landmark": np.array([-1, -1, -1, -1, 0] * 2, np.int32)}


def _ties_scene(job_pass):
    """Landmarks 0 and 1: one descriptor, 2 cm apart, and a keypoint with that descriptor: the first
    wins. Landmark 2 / 3: a keypoint 60 / 59 bits from its only descriptor: unmatched / matched."""
    s = _hand_scene()
    q = 0.5 if job_pass == 0 else 1e-5
    rng = np.random.default_rng(60)
    Z, X, Y = (rng.integers(0, 256, 48, dtype=np.uint8) for _ in range(3))
    s["landmarks"] = np.array([[0, 0, 5, 1], [0.02, 0, 5, 1], [-1, 0, 5, 1], [-1, 1, 5, 1]], np.float64)
    s["landmark_quality"] = np.full(4, q)
    s["obs_begin"] = np.array([0, 1, 2, 3, 4], np.int32)
    s["obs_pose"] = np.array([1, 1, 0, 0], np.int32)
    s["obs_camera"] = np.zeros(4, np.int32)
    s["obs_descriptor"] = np.array([Z, Z, X, Y])
    s["obs_ray"] = np.array([s["landmarks"][l, :3] - s["poses"][p, :3] for l, p in ((0, 1), (1, 1), (2, 0), (3, 0))])
    s["job_camera"], s["job_pass"] = np.array([0], np.int32), np.array([job_pass], np.int32)
    s["job_pose_prepare"] = s["job_pose_match"] = IDENT[None].copy()
    s["kp_begin"] = np.array([0, 3], np.int32)
    s["keypoint"] = np.array([[321, 240.5], [240.5, 239], [241, 319]], np.float64)
    s["descriptor"] = np.array([Z, _flip(X, 60, 1), _flip(Y, 59, 2)])
    s["ray"] = np.array([[0.002, 0.001, 1], [-0.2, 0.001, 1], [-0.2, 0.2, 1]], np.float64)
    s["ray_valid"] = np.ones(3, np.uint8)
    s["landmark"] = np.full(3, -1, np.int32)
    return s


def _lanes_scene():
    """Jobs of 1, 63, 64, 65 and 130 keypoints in each pass over a map of 70 landmarks (two rounds of
    64 lanes), landmark 0 with 20 observations, and a job in each pass no landmark is visible from."""
    cams = [mt.pinhole()]
    world = mt.toy_world(21, 70, cams, seed=11, full_landmarks=1)
    s = mt.build_scene(*world[:3], cams, *world[3:], seed=12, passes=(0,))
    n0 = int(s["kp_begin"][1])
    prepared, matched = s["job_pose_prepare"][0], s["job_pose_match"][0]
    away = prepared + np.array([1000.0, 0, 0, 0, 0, 0, 0])
    jobs = [(0, p, (np.arange(n) * 7 + n) % n0, prepared, matched) for p in (0, 1) for n in (1, 63, 64, 65, 130)]
    jobs += [(0, p, np.arange(10), away, away) for p in (0, 1)]
    return mt.with_jobs(s, jobs)


def _distortion_scene():
    """One camera per distortion model, both passes. For the radtan8 camera two more landmarks: one
    at rho = 100 in front (Invalid) and one behind the camera that projects just left of the image
    (not Behind: a candidate)."""
    cams = [mt.pinhole(0), mt.pinhole(1, (-0.28, 0.07, 2e-4, 1.8e-5)), mt.pinhole(2, (-0.01, 0.02, -0.01, 0.005)),
            mt.pinhole(3, (0.1, -0.05, 1e-3, -5e-4, 0.01, 0.12, -0.04, 8e-3))]
    world = mt.toy_world(8, 40, cams, seed=21)
    s = mt.build_scene(*world[:3], cams, *world[3:], seed=22)
    C1, r1 = mt.compose(s["job_pose_prepare"][3], s["extrinsics"][3])
    desc = np.random.default_rng(23).integers(0, 256, 48, dtype=np.uint8)
    s = mt.append_landmark(s, [*(r1 + C1 @ np.array([30.0, 0.0, 3.0])), 1.0], 0.5, [(0, 3, desc, [0.1, 0.0, 1.0])])
    for u0 in np.arange(-0.7, -1.3, -0.002):  # behind: x / z = u0 with z = -2
        status, px = mt.project_homogeneous(cams[3], np.array([-2.0 * u0, 0.0, -2.0, 1.0]))
        if status == "outside" and -20.0 < px[0] < -5.0:
            break
    else:
        raise AssertionError("no point behind the camera projects into the band left of the image")
    return mt.append_landmark(s, [*(r1 + C1 @ np.array([-2.0 * u0, 0.0, -2.0])), 1.0], 0.5,
                              [(0, 3, _flip(desc, 100, 4), [0.1, 0.0, 1.0]), (1, 3, _flip(desc, 90, 5), [0.1, 0.0, 1.0])])


def _quality0_scene():
    cams = [mt.pinhole()]
    world = mt.toy_world(6, 30, cams, seed=31)
    s = mt.build_scene(*world[:3], cams, *world[3:], seed=32)
    s["landmark_quality"] = s["landmark_quality"].copy()
    s["landmark_quality"][::4] = 0.0
    return s


def _empty_map_scene():
    s = _hand_scene()
    s["landmarks"], s["landmark_quality"] = np.zeros((0, 4)), np.zeros(0)
    s["obs_begin"] = np.zeros(1, np.int32)
    s["obs_pose"] = s["obs_camera"] = np.zeros(0, np.int32)
    s["obs_descriptor"], s["obs_ray"] = np.zeros((0, 48), np.uint8), np.zeros((0, 3))
    s["landmark"] = np.full(10, -1, np.int32)
    return s


SCENES = {"s6": lambda: _window_scene(False), "s6_loop": lambda: _window_scene(True), "hand": _hand_scene,
          "ties0": lambda: _ties_scene(0), "ties1": lambda: _ties_scene(1), "lanes": _lanes_scene,
          "distortions": _distortion_scene, "quality0": _quality0_scene, "empty_map": _empty_map_scene}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, literal's result): built once and shared, never modified."""
    s = SCENES[name]()
    return s, mt.literal(s)


def _batch(og, s):
    cams = []
    for c in s["cameras"]:
        q = og.Camera()
        q.distortion, q.width, q.height = c["distortion"], c["width"], c["height"]
        q.fu, q.fv, q.cu, q.cv = c["fu"], c["fv"], c["cu"], c["cv"]
        for i in range(8):
            q.dist[i] = c["dist"][i]
        cams.append(q)
    return og.match_batch(cameras=cams, **{k: v for k, v in s.items() if k != "cameras"})


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", sorted(SCENES))
def test_literal_and_ordered_agree(og, name):
    """The serial walk and the first-minimum / prefix-minima formulation give the same tables: the
    integers exactly, the doubles bit for bit except record_repr_sum (a regrouped sum)."""
    s, lit = scene(name)
    ord_ = mt.ordered(s)
    for k in mt.INT_KEYS:
        assert np.array_equal(lit[k], ord_[k]), k
    assert np.array_equal(lit["cand_projection"], ord_["cand_projection"]) and np.array_equal(lit["point"], ord_["point"])
    assert mt.worst_relative(ord_["record_repr_sum"], lit["record_repr_sum"]) <= 1e-14


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_margins(og, name):
    """No floating-point comparison of a scene is decided by less than 1e-9."""
    _, lit = scene(name)
    print(f"{name}: margin {lit['margin']:.3e}")
    assert lit["margin"] >= MARGIN


@pytest.mark.parametrize("name", ["s6", "s6_loop"])
def test_window_scenes_reach_their_branches(og, name):
    s, lit = scene(name)
    st = lit["stats"]
    print(name, st)
    passes = np.asarray(s["job_pass"])
    for j in range(len(passes)):
        assert st["n_3d"][j] >= 10 and st["n_not3d"][j] >= 10
    for p in (0, 1):
        assert sum(a for a, q in zip(st["accepted"], passes) if q == p) >= 10
    assert max(st["replaced"]) >= 1  # a landmark with more than 3 kept observations
    if name == "s6":
        assert st["point_not_of_match"] >= 1
    if name == "s6_loop":  # carried landmarks that are re-found: the count-and-leave rule
        assert st["carried_hits"] >= 1
        assert s["landmark_use"].sum() * 3 == len(s["landmark_use"])


def _hand_expected():
    r5 = np.sqrt(5.0)
    return {"cand_n": [[2, 2, -1, -1, -1]] * 2, "cand_is3d": [[1, 0, 0, 0, 0]] * 2,
            "cand_obs": [[[1, 0, -1], [3, 2, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]] * 2,
            "cand_projection": [[[320, 240], [400, 240], [0, 0], [0, 0], [0, 0]]] * 2,
            "match_landmark": [0, 0, -1, -1, -1, -1, -1, 1, -1, -1],
            "match_distance": [3, 2, -1, -1, -1, -1, -1, 2, -1, -1],
            "n_records": [1, 2, 0, 0, 0, 0, 0, 1, 0, 0],
            "record_repr_sum": [r5, 2 * r5, 0, 0, 0, 0, 0, 0, 0, 0],
            "point": [[0, 0, 0, 0]] * 7 + [[1, 0, 5, 1]] + [[0, 0, 0, 0]] * 2}


def _assert_hand(got):
    for k, v in _hand_expected().items():
        if k in mt.INT_KEYS:
            assert np.array_equal(got[k], np.array(v)), k
        else:
            assert mt.worst_relative(got[k], np.array(v, np.float64)) <= BOUND, k


def test_hand_written_case(og):
    s, lit = scene("hand")
    _assert_hand(lit)
    _assert_hand(mt.ordered(s))


def test_crafted_scenes_hold_what_they_are_for(og):
    """Ties, thresholds, the radtan8 landmarks, quality 0, the lanes scene's shapes."""
    for name in ("ties0", "ties1"):
        _, lit = scene(name)
        assert list(lit["cand_n"][0]) == [1, 1, 1, 1]
        assert list(lit["match_landmark"]) == [0, -1, 3] and list(lit["match_distance"]) == [0, -1, 59]
    s, lit = scene("distortions")
    L = len(s["landmarks"])
    radtan8_jobs = [j for j in range(len(s["job_camera"])) if s["job_camera"][j] == 3]
    assert len(radtan8_jobs) == 2 and sorted(c["distortion"] for c in s["cameras"]) == [0, 1, 2, 3]
    for j in radtan8_jobs:
        assert lit["cand_n"][j, L - 2] == -1 and lit["cand_n"][j, L - 1] == 2
    assert (lit["match_landmark"] >= 0).sum() >= 20
    s, lit = scene("quality0")
    zero = s["landmark_quality"] == 0.0
    assert zero.sum() >= 5 and (lit["cand_n"][:, zero] > 0).any() and not lit["cand_is3d"][:, zero].any()
    s, lit = scene("lanes")
    sizes = np.diff(s["kp_begin"])
    assert list(sizes) == [1, 63, 64, 65, 130] * 2 + [10, 10]
    assert s["obs_begin"][1] - s["obs_begin"][0] == 20 and len(s["landmarks"]) == 70
    assert (lit["cand_n"][10:] == -1).all() and (lit["cand_n"][:10] > 0).sum(axis=1).min() >= 20
    assert (lit["match_landmark"][: s["kp_begin"][10]] >= 0).sum() >= 100


def test_symbol_and_struct_layouts(og, tmp_path):
    """The entry point is declared and exported; MatchBatch and MatchResult mirror the header."""
    assert "okvisgpu_match_to_map" in og.EXPORTED_SYMBOLS
    assert hasattr(og.lib(), "okvisgpu_match_to_map")
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    types = {"okvisgpu_match_batch": og.MatchBatch, "okvisgpu_match_result": og.MatchResult}
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
    lib = og.lib()
    b, keep = _batch(og, scene("hand")[0])
    r = og.MatchResult()
    assert lib.okvisgpu_match_to_map(None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.okvisgpu_match_to_map(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------ GPU
def _compare(parity, name, got, ref):
    for k in mt.INT_KEYS:
        assert np.array_equal(got[k], ref[k]), (name, k)
    for k in mt.REAL_KEYS:
        parity(f"match_to_map/{name}/{k}", mt.worst_relative(got[k], ref[k]), BOUND)


def _run(og, ctx, s, fill=None):
    b, keep = _batch(og, s)
    return ctx.match_to_map(b, fill=fill)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["s6", "s6_loop"])
def test_gpu_window(og, gpu_ctx, parity, name):
    """The S6 window (6 keyframes, 150 landmarks, 1000 observations), both cameras, both passes: normal
    mode, and loop-closure mode with a third of the map in use and carried landmarks re-found."""
    s, lit = scene(name)
    _compare(parity, name, _run(og, gpu_ctx, s), lit)


@pytest.mark.gpu
def test_gpu_ties_and_thresholds(og, gpu_ctx, parity):
    """Two landmarks with the keypoint's descriptor: the first wins. Distance 60 is no match, 59 is.
    Both passes; and the hand-written case against its written-out tables."""
    for name in ("ties0", "ties1"):
        s, lit = scene(name)
        got = _run(og, gpu_ctx, s)
        _compare(parity, name, got, lit)
        assert list(got["match_landmark"]) == [0, -1, 3] and list(got["match_distance"]) == [0, -1, 59]
    _assert_hand(_run(og, gpu_ctx, scene("hand")[0]))


@pytest.mark.gpu
def test_gpu_lane_mapping_edges(og, gpu_ctx, parity):
    """Jobs of 1, 63, 64, 65 and 130 keypoints, 70 landmarks, a landmark with 20 observations, jobs no
    landmark is visible from; J = 0; a map without landmarks."""
    s, lit = scene("lanes")
    _compare(parity, "lanes", _run(og, gpu_ctx, s), lit)
    s, lit = scene("empty_map")
    got = _run(og, gpu_ctx, s, fill={k: 77 for k in mt.INT_KEYS + mt.REAL_KEYS})
    _compare(parity, "empty_map", got, lit)
    assert (got["match_landmark"] == -1).all() and not got["n_records"].any() and got["cand_n"].shape == (2, 0)
    none = mt.with_jobs(scene("hand")[0], [])
    got = _run(og, gpu_ctx, none)
    assert all(got[k].size == 0 for k in mt.INT_KEYS + mt.REAL_KEYS)


@pytest.mark.gpu
def test_gpu_distortion_models(og, gpu_ctx, parity):
    """None, radtan, equidistant and radtan8, with a landmark at rho > 9 and one behind the camera
    that projects outside the image."""
    s, lit = scene("distortions")
    _compare(parity, "distortions", _run(og, gpu_ctx, s), lit)


@pytest.mark.gpu
def test_gpu_quality_zero(og, gpu_ctx, parity):
    s, lit = scene("quality0")
    _compare(parity, "quality0", _run(og, gpu_ctx, s), lit)


@pytest.mark.gpu
def test_gpu_batch_independence_and_determinism(og, gpu_ctx):
    """A job alone and as the second of three: identical bytes. Two runs: identical bytes."""
    s, _ = scene("s6")
    full = _run(og, gpu_ctx, s)
    again = _run(og, gpu_ctx, s)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for j in (1, 2):  # a pass-0 and a pass-1 job
        three = mt.sub_scene(s, [0, j, 3])
        alone = mt.sub_scene(s, [j])
        a, b, c = _run(og, gpu_ctx, alone), _run(og, gpu_ctx, three), mt.job_rows(s, full, j)
        for k, v in mt.job_rows(alone, a, 0).items():
            assert v.tobytes() == mt.job_rows(three, b, 1)[k].tobytes() == c[k].tobytes(), (j, k)


@pytest.mark.gpu
def test_gpu_argument_errors(og, gpu_ctx):
    """Out-of-range indices, a non-monotone CSR and a call inside a solve are refused with
    OKVISGPU_ERR_INVALID_ARGUMENT and leave the sentinel-filled outputs alone."""
    s, _ = scene("hand")
    sentinel = {k: 77 for k in mt.INT_KEYS + mt.REAL_KEYS}

    def refused(change, match):
        t = dict(s)
        for k, (i, v) in change.items():
            t[k] = np.array(s[k]).copy()
            t[k][i] = v
        b, keep = _batch(og, t)
        r = og.MatchResult()
        out = {}
        for k, (shape, dt) in {"match_landmark": ((10,), np.int32), "match_distance": ((10,), np.int32),
                               "n_records": ((10,), np.int32), "record_repr_sum": ((10,), np.float64),
                               "point": ((10, 4), np.float64), "cand_n": ((2, 5), np.int32),
                               "cand_is3d": ((2, 5), np.uint8), "cand_obs": ((2, 5, 3), np.int32),
                               "cand_projection": ((2, 5, 2), np.float64)}.items():
            out[k] = np.full(shape, sentinel[k], dt)
            setattr(r, k, out[k].ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dt))))
        rc = og.lib().okvisgpu_match_to_map(gpu_ctx.h, C.byref(b), C.byref(r))
        assert rc == ERR_INVALID_ARGUMENT
        assert match in og.lib().okvisgpu_last_error(gpu_ctx.h).decode()
        for k, a in out.items():
            assert (a == sentinel[k]).all(), k

    refused({"job_camera": (1, 1)}, "job_camera")
    refused({"job_camera": (0, -1)}, "job_camera")
    refused({"obs_camera": (2, 3)}, "obs_camera")
    refused({"obs_pose": (4, 2)}, "obs_pose")
    refused({"landmark": (7, 5)}, "carried landmark")
    refused({"landmark": (7, -2)}, "carried landmark")
    refused({"job_pass": (0, 2)}, "job_pass")
    refused({"kp_begin": (1, 11)}, "kp_begin")
    refused({"kp_begin": (0, 1)}, "kp_begin")
    refused({"obs_begin": (2, 6)}, "obs_begin")
    w = og.SynthWindow(10, 500, 4000, seed=78)
    gpu_ctx.set_problems([w.problem])
    gpu_ctx.solve_begin(og.default_options(max_num_iterations=2))
    try:
        refused({}, "solve_end")
    finally:
        gpu_ctx.solve_end()
    _assert_hand(_run(og, gpu_ctx, s))
