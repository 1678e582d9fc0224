"""okvisgpu_match_frames: the matching loops of Frontend::matchMotionStereo (Frontend.cpp:2057-2149, mode 0)
and Frontend::matchStereo (:2259-2316, mode 1) on the device.

CPU: the numpy restatement (tests/_match_frames.py) in its two formulations, the reference's serial loops
(`literal`) and first-admissible-minimum (`ordered`), agree exactly on every scene the GPU tests use; every
scene decides each floating-point comparison with a margin >= 1e-9 and keeps every acos argument away from
+-1, which makes the exact comparison of the device's integer decisions legitimate; the crafted scenes hold
what they are for and the frames scene reaches its branches; a hand-written case with its tables written
out; the struct layouts and the NULL checks.
GPU: the device against `literal`: integers equal, doubles within 1e-9 max(1, |value|)."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import _match_frames as mf
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
MARGIN = 1e-9
BOUND = 1e-9
IDENT = mf.IDENT
HAND_CAM = {"distortion": 0, "width": 640, "height": 480, "fu": 400.0, "fv": 400.0, "cu": 320.0, "cv": 240.0,
            "dist": [0.0] * 8}


def _flip(desc, n, seed):
    return mf.flip_bits(np.random.default_rng(seed), np.asarray(desc, np.uint8), n)


def _descs(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 48), dtype=np.uint8)


def _tilt(T, a):
    """T with the small rotation a (angles about x, y, z) in place of its rotation."""
    h = 0.5 * np.asarray(a, np.float64)
    return np.array([*T[:3], *h, np.sqrt(1.0 - h @ h)])


def _views(mode, r1, tilt=(0.0, 0.0, 0.0)):
    """(pose0, pose1, ext0, ext1) of two cameras, the first at the origin, the second at r1: two frames with
    identity extrinsics in mode 0, one frame with two extrinsics in mode 1."""
    T1 = _tilt(mf.at(*r1), tilt)
    return (IDENT, T1, IDENT, IDENT) if mode == 0 else (IDENT, IDENT, IDENT, T1)


# ------------------------------------------------------------------------------------------ scenes
def _hand_scene():
    """f = 400, 640 x 480, centre (320, 240), identity rotations, camera 1 half a metre to the right of
    camera 0. A (0, 0, 5), B (1, 0, 4), D (-1, 0.5, 5) and the far C (0, 0, 100), whose parallax of 5 mrad is
    below 6 sigma = 15 mrad (size 8): parallel. Job 0 (mode 0): side 0 = A, B, D, C with use0 = 0 on D; side
    1 = A (3 bits off), B (10 bits off), B again (2 bits off, but without a valid ray), C (1 bit off), D.
    Job 1 (mode 1): the same keypoints, every use0 = 1 and B's ray_valid0 = 0."""
    A, B, Cf, D = (0, 0, 5), (1, 0, 4), (0, 0, 100), (-1, 0.5, 5)
    DA, DB, DC, DD = _descs(70, 4)
    jobs = []
    for mode in (0, 1):
        v = _views(mode, (0.5, 0, 0))
        s0 = mf.side(HAND_CAM, v[0], v[2], [A, B, D, Cf], [DA, DB, DD, DC], use=[1, 1, 0, 1] if mode == 0 else None,
                     valid=None if mode == 0 else [1, 0, 1, 1])
        s1 = mf.side(HAND_CAM, v[1], v[3], [A, B, B, Cf, D], [_flip(DA, 3, 1), _flip(DB, 10, 2), _flip(DB, 2, 3),
                                                               _flip(DC, 1, 4), DD], valid=[1, 1, 0, 1, 1])
        jobs.append(mf.job(mode, 0, 0, *v, s0, s1))
    return mf.scene([HAND_CAM], jobs)


def _hand_expected():
    A, B, Cf, D, O = [0, 0, 5, 1], [1, 0, 4, 1], [0, 0, 100, 1], [-1, 0.5, 5, 1], [0, 0, 0, 0]
    return {"match": [0, 1, -1, 3, 0, -1, 4, 3], "distance": [3, 10, -1, 1, 3, -1, 0, 1],
            "point": [A, B, O, Cf, A, O, D, Cf], "initialisable": [1, 1, 0, 0, 1, 0, 1, 0],
            "quality": [np.arctan(0.1), np.arctan(1 / 4) - np.arctan(0.5 / 4), 0, np.arctan(0.005), 0, 0, 0, 0]}


def _lanes_scene():
    """Side-1 sizes 1, 63, 64, 65 and 130 against side-0 sizes 1, 65 and 130 in both modes, over a pool of
    70 points (a side of 130 holds most points twice, with different descriptor noise: the best is lowered
    within and across rounds); then a job with side 0 empty, one with side 1 empty, one whose use1 is 0."""
    cams = [mf.pinhole()]
    rng = np.random.default_rng(5)
    pool = np.column_stack([rng.uniform(-1.5, 1.5, 70), rng.uniform(-1.0, 1.0, 70), rng.uniform(3.0, 10.0, 70)])
    base = _descs(6, 70)

    def one_side(T_WS, T_SC, n, mul, add):
        idx = (np.arange(n) * mul + add) % 70
        return mf.side(cams[0], T_WS, T_SC, pool[idx], [mf.flip_bits(rng, base[i], int(rng.integers(0, 26))) for i in idx],
                       rng, pixel_noise=0.5, ray_noise=0.3 / 400, size=rng.uniform(6.0, 12.0, n),
                       valid=rng.random(n) < 0.95, use=rng.random(n) < 0.95)

    jobs = []
    for mode in (0, 1):
        v = _views(mode, (0.3, 0.02, 0.05), (0.004, -0.006, 0.003))
        for n0 in (1, 65, 130):
            for n1 in (1, 63, 64, 65, 130):
                jobs.append(mf.job(mode, 0, 0, *v, one_side(v[0], v[2], n0, 11, 5), one_side(v[1], v[3], n1, 9, 5)))
    v = _views(0, (0.3, 0.02, 0.05))
    jobs.append(mf.job(0, 0, 0, *v, mf.empty_side(), one_side(v[1], v[3], 10, 9, 5)))
    jobs.append(mf.job(1, 0, 0, *v, one_side(v[0], v[2], 10, 9, 5), mf.empty_side()))
    off = one_side(v[1], v[3], 70, 9, 5)
    off["use"][:] = 0
    jobs.append(mf.job(0, 0, 0, *v, one_side(v[0], v[2], 10, 9, 5), off))
    return mf.scene(cams, jobs)


def _ties_jobs(mode, sixty_only=False):
    """[same round, across rounds, thresholds]: a side-0 keypoint with descriptor Z seeing P, and side 1 =
    80 unrelated keypoints but two with descriptor Z, at P and 2 cm beside it in the epipolar plane (both
    admissible): at indices (5, 20) and (10, 70). Then keypoints 60 and 59 bits from their partners."""
    cam = mf.pinhole()
    rng = np.random.default_rng(40 + mode)
    v = _views(mode, (0.5, 0, 0))
    Z, X, Y = _descs(41, 3)
    P = np.array([0.2, 0.1, 4.0])
    jobs = []
    for a, b in () if sixty_only else ((5, 20), (10, 70)):
        pts = np.column_stack([rng.uniform(-1, 1, 80), rng.uniform(-1, 1, 80), rng.uniform(3, 8, 80)])
        desc = rng.integers(0, 256, size=(80, 48), dtype=np.uint8)
        pts[a], pts[b], desc[a], desc[b] = P, P + [0.02, 0, 0], Z, Z
        jobs.append(mf.job(mode, 0, 0, *v, mf.side(cam, v[0], v[2], [P], [Z]), mf.side(cam, v[1], v[3], pts, desc)))
    PX, PY = [-0.5, 0.3, 5.0], [0.7, -0.4, 6.0]
    s0 = mf.side(cam, v[0], v[2], [PX] if sixty_only else [PX, PY], [_flip(X, 60, 1)] if sixty_only else
                 [_flip(X, 60, 1), _flip(Y, 59, 2)])
    jobs.append(mf.job(mode, 0, 0, *v, s0, mf.side(cam, v[1], v[3], [PX, PY], [X, Y])))
    return jobs


def _ties_scene():
    return mf.scene([mf.pinhole()], _ties_jobs(0) + _ties_jobs(1))


def _ties605_scene():
    """Threshold 60.5 and a candidate at distance 60: below uint32_t(60.5) = 60 it is not (mode 0), below
    the double 60.5 it is (mode 1)."""
    return mf.scene([mf.pinhole()], _ties_jobs(0, True) + _ties_jobs(1, True), matching_threshold=60.5)


BLOCKED = ("angle", "depth0", "depth1", "triangulation", "ray_valid1")


def _blocked_scene():
    """Per mode and reason one job: side 0 one keypoint with descriptor D seeing G; side 1 = [a blocker 5
    bits from D that is inadmissible for the reason, G's keypoint 20 bits from D]. The blocker lies on the
    side-0 keypoint's ray (so it triangulates) where the reason holds: e0 . e1 = 0.6; depth 0.15 m (mode 1:
    0.075 m) in camera 0 with camera 1 0.1 m behind; the same in camera 1 with camera 1 0.1 m in front; 0.05
    rad out of the epipolar plane; G itself without a valid ray. Then, mode 0: a winner whose keypoint lies
    10 px from its projection, with a second admissible candidate behind it: no match. Both modes: a far
    winner (100 m at 0.5 m baseline), parallel."""
    cam = mf.pinhole()
    D = _descs(50, 1)[0]
    jobs = []
    for mode in (0, 1):
        near = 0.15 if mode == 0 else 0.075
        for reason in BLOCKED:
            r1 = {"depth0": (0.06, 0, -0.1), "depth1": (0.06, 0, 0.1)}.get(reason, (0.5, 0, 0))
            v = _views(mode, r1)
            valid = [1, 1]
            if reason == "angle":
                G, B = np.array([2.0, 0, 4.0]), np.array([0.25, 0, 0.5])
            elif reason == "depth0":
                G, B = np.array([0.3, 0, 1.5]), np.array([0.2, 0, 1.0]) * near
            elif reason == "depth1":
                G, B = np.array([0.3, 0, 1.5]), np.array([0.2, 0, 1.0]) * (near + 0.1)
            elif reason == "triangulation":
                G = np.array([0.3, 0.1, 4.0])
                B = G + [0, 0.2, 0]
            else:
                G = B = np.array([0.3, 0.1, 4.0])
                valid = [0, 1]
            jobs.append(mf.job(mode, 0, 0, *v, mf.side(cam, v[0], v[2], [G], [D]),
                               mf.side(cam, v[1], v[3], [B, G], [_flip(D, 5, 1), _flip(D, 20, 2)], valid=valid)))
    v = _views(0, (0.5, 0, 0))
    G = np.array([0.3, 0.1, 4.0])
    s1 = mf.side(cam, v[1], v[3], [G, G], [_flip(D, 5, 1), _flip(D, 20, 2)])
    s1["keypoint"][0] += [10.0, 0.0]
    jobs.append(mf.job(0, 0, 0, *v, mf.side(cam, v[0], v[2], [G], [D]), s1))
    for mode in (0, 1):
        v = _views(mode, (0.5, 0, 0))
        F = [1.0, 0.5, 100.0]
        jobs.append(mf.job(mode, 0, 0, *v, mf.side(cam, v[0], v[2], [F], [D]), mf.side(cam, v[1], v[3], [F], [_flip(D, 7, 3)])))
    return mf.scene([cam], jobs)


def _distortion_scene():
    """Mode-0 jobs with one camera per distortion model (none, radtan, equidistant, radtan8) over 40 points,
    some side-1 keypoints 6 px off their projection; the radtan8 job has one more pair whose point lies at
    x / z = 3.2 in camera 1 (rho > 9: the winner's projection is Invalid, no match)."""
    cams = [mf.pinhole(0), mf.pinhole(1, (-0.28, 0.07, 2e-4, 1.8e-5)), mf.pinhole(2, (-0.01, 0.02, -0.01, 0.005)),
            mf.pinhole(3, (0.1, -0.05, 1e-3, -5e-4, 0.01, 0.12, -0.04, 8e-3))]
    rng = np.random.default_rng(21)
    v = _views(0, (0.3, 0.02, 0.05), (0.004, -0.006, 0.003))
    jobs = []
    for c, cam in enumerate(cams):
        pts = np.column_stack([rng.uniform(-1.5, 1.8, 40), rng.uniform(-1.0, 1.0, 40), rng.uniform(3.0, 8.0, 40)])
        base = rng.integers(0, 256, size=(40, 48), dtype=np.uint8)
        if c == 3:
            C1, r1 = mf.compose(v[1], v[3])
            pts = np.vstack([pts, r1 + C1 @ np.array([6.4, 0.0, 2.0])])
            base = np.vstack([base, _descs(22, 1)])
        n = len(pts)
        perm = rng.permutation(n)
        s0 = mf.side(cam, v[0], v[2], pts, [mf.flip_bits(rng, d, int(rng.integers(0, 30))) for d in base], rng,
                     ray_noise=0.3 / 400, size=rng.uniform(6.0, 12.0, n))
        s1 = mf.side(cam, v[1], v[3], pts[perm], [mf.flip_bits(rng, d, int(rng.integers(0, 30))) for d in base[perm]], rng,
                     pixel_noise=0.7, ray_noise=0.3 / 400, size=rng.uniform(6.0, 12.0, n))
        s1["keypoint"][::9] += [4.5, -4.0]
        jobs.append(mf.job(0, c, c, *v, s0, s1))
    return mf.scene(cams, jobs)


def _frames_scene():
    """og.SynthWindow(6, 150, 1000, seed=3)'s ground truth: keyframes 1 and 3 against frame 5 in both
    cameras (mode 0) and frame 5's camera 0 against its camera 1 (mode 1). Keypoints
    are the landmarks' projections with pixel noise and noisy descriptors; side 1 also holds look-alikes
    (a true keypoint's descriptor, a few bits off, on an unrelated ray) and keypoints 9 px off their
    projection."""
    import okvisgpu as og
    w = og.SynthWindow(6, 150, 1000, seed=3)
    p = w.problem
    cams = [{"distortion": q.distortion, "width": q.width, "height": q.height, "fu": q.fu, "fv": q.fv, "cu": q.cu,
             "cv": q.cv, "dist": list(q.dist)} for q in (p.cameras[c] for c in range(p.n_cameras))]
    poses, lms, _ = w.ground_truth()
    ext = w.true_extrinsics()
    rng = np.random.default_rng(3)
    pts = lms[:, :3] / lms[:, 3:]
    base = rng.integers(0, 256, size=(len(pts), 48), dtype=np.uint8)

    def image(frame, c, second):
        C, r = mf.compose(poses[frame], ext[c])
        seen = [i for i, q in enumerate(pts)
                if mf.project_homogeneous(cams[c], np.array([*(C.T @ (q - r)), 1.0]))[0] == "ok"]
        n = len(seen)
        s = mf.side(cams[c], poses[frame], ext[c], pts[seen], [mf.flip_bits(rng, base[i], int(rng.integers(0, 36))) for i in seen],
                    rng, pixel_noise=0.5, ray_noise=0.3 / cams[c]["fu"], size=rng.uniform(6.0, 14.0, n),
                    valid=rng.random(n) < 0.97, use=rng.random(n) < 0.8)
        if second:
            s["keypoint"][::11] += [7.0, -6.0]
            m = n // 4
            like = {"keypoint": np.column_stack([rng.uniform(0, cams[c]["width"], m), rng.uniform(0, cams[c]["height"], m)]),
                    "size": rng.uniform(6.0, 14.0, m),
                    "descriptor": np.array([mf.flip_bits(rng, s["descriptor"][i], int(rng.integers(0, 8)))
                                            for i in rng.integers(0, n, m)]),
                    "ray": np.column_stack([rng.uniform(-0.5, 0.5, m), rng.uniform(-0.4, 0.4, m), np.ones(m)]),
                    "ray_valid": np.ones(m, np.uint8), "use": np.ones(m, np.uint8)}
            order = rng.permutation(n + m)
            s = {k: np.concatenate([s[k], like[k]])[order] for k in s}
        return s

    jobs = [mf.job(0, c, c, poses[kf], poses[5], ext[c], ext[c], image(kf, c, False), image(5, c, True))
            for kf in (1, 3) for c in (0, 1)]
    jobs.append(mf.job(1, 0, 1, poses[5], poses[5], ext[0], ext[1], image(5, 0, False), image(5, 1, True)))
    return mf.scene(cams, jobs)


SCENES = {"lanes": _lanes_scene, "ties": _ties_scene, "ties605": _ties605_scene, "blocked": _blocked_scene,
          "hand": _hand_scene, "distortions": _distortion_scene, "frames": _frames_scene}


@functools.lru_cache(maxsize=None)
def scene(name):
    """(scene, literal's result): built once and shared, never modified."""
    s = SCENES[name]()
    return s, mf.literal(s)


def _batch(og, s):
    cams = []
    for c in s["cameras"]:
        q = og.Camera()
        q.distortion, q.width, q.height = c["distortion"], c["width"], c["height"]
        q.fu, q.fv, q.cu, q.cv = c["fu"], c["fv"], c["cu"], c["cv"]
        for i in range(8):
            q.dist[i] = c["dist"][i]
        cams.append(q)
    return og.frame_match_batch(cameras=cams, **{k: v for k, v in s.items() if k != "cameras"})


# ------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", sorted(SCENES))
def test_literal_and_ordered_agree(og, name):
    """The serial walk and the first-admissible-minimum formulation give the same tables, bit for bit."""
    s, lit = scene(name)
    ord_ = mf.ordered(s)
    for k in mf.KEYS:
        assert np.array_equal(lit[k], ord_[k]), k


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_margins(og, name):
    """No floating-point comparison of a scene is decided by less than 1e-9, no acos argument is within
    1e-8 of +-1 (Margin.acos counts that as margin 0), and no result is NaN."""
    _, lit = scene(name)
    print(f"{name}: margin {lit['margin']:.3e}")
    assert lit["margin"] >= MARGIN
    assert np.isfinite(lit["quality"]).all() and np.isfinite(lit["point"]).all()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_points_are_well_conditioned(og, name):
    """triangulateFast's determinant e1.e1 e2.e2 - (e1.e2)^2 cancels to theta^2 for rays theta apart, so one
    rounding (1.1e-16) in it moves the point by about 1.1e-16 / theta^2 of its distance, in the reference as in
    any restatement. Every matched point of a compared scene has a parallax of at least 2 mrad: 3e-11 per
    rounding, which leaves the 1e-9 bound to the implementation."""
    s, lit = scene(name)
    for j in range(len(s["job_mode"])):
        J, r = mf._job(s, j), mf.job_rows(s, lit, j)
        for p in r["point"][r["match"] >= 0][:, :3]:
            assert np.arccos(mf.normalised(p - J["r0"]) @ mf.normalised(p - J["r1"])) >= 2e-3, (j, p)


def test_frames_scene_reaches_its_branches(og):
    s, lit = scene("frames")
    st = lit["stats"]
    print({k: (v if k != "final_failures" else len(v)) for k, v in st.items()})
    assert list(s["job_mode"]) == [0, 0, 0, 0, 1]
    assert st["matches"][0] >= 10 and st["matches"][1] >= 10
    assert st["rejected_geometry"] >= 5 and st["parallel_winners"] >= 1 and len(st["final_failures"]) >= 1


def _assert_hand(got):
    for k, v in _hand_expected().items():
        if k in mf.INT_KEYS:
            assert np.array_equal(got[k], np.array(v)), k
        else:
            assert mf.worst_relative(got[k], np.array(v, np.float64)) <= BOUND, k


def test_hand_written_case(og):
    s, lit = scene("hand")
    assert max(np.diff(s["kp0_begin"]).max(), np.diff(s["kp1_begin"]).max()) <= 5
    _assert_hand(lit)
    _assert_hand(mf.ordered(s))


def _assert_ties(got):
    assert list(got["match"]) == [5, 10, -1, 1] * 2 and list(got["distance"]) == [0, 0, -1, 59] * 2


def _assert_ties605(got):
    assert list(got["match"]) == [-1, 0] and list(got["distance"]) == [-1, 60]


def _assert_blocked(got):
    n = len(BLOCKED)
    assert list(got["match"]) == [1] * (2 * n) + [-1, 0, 0] and list(got["distance"]) == [20] * (2 * n) + [-1, 7, 7]
    assert list(got["initialisable"]) == [1] * (2 * n) + [0, 0, 0]


def test_crafted_scenes_hold_what_they_are_for(og):
    """Lane shapes, ties, thresholds, each blocker's reason, the radtan8 winner beyond rho = 9."""
    s, lit = scene("lanes")
    assert [(a, b) for a, b in zip(np.diff(s["kp0_begin"]), np.diff(s["kp1_begin"]))] == \
        [(n0, n1) for _ in (0, 1) for n0 in (1, 65, 130) for n1 in (1, 63, 64, 65, 130)] + [(0, 10), (10, 0), (10, 70)]
    assert (lit["match"][: s["kp0_begin"][30]] >= 0).sum() >= 200 and (lit["match"][s["kp0_begin"][30]:] == -1).all()
    assert (lit["match"] >= 64).sum() >= 20 and not s["use1"][s["kp1_begin"][32]:].any()
    _assert_ties(scene("ties")[1])
    _assert_ties605(scene("ties605")[1])
    s, lit = scene("blocked")
    _assert_blocked(lit)
    assert lit["stats"]["final_failures"] == [(2 * len(BLOCKED), 0, "far")]
    for j in range(2 * len(BLOCKED)):  # the blocker (side-1 keypoint 0) fails for its reason and no other
        J, mode, reason = mf._job(s, j), j // len(BLOCKED), BLOCKED[j % len(BLOCKED)]
        e0 = mf.normalised(J["C0"] @ s["ray0"][J["a0"]])
        e1 = mf.normalised(J["C1"] @ s["ray1"][J["a1"]])
        sigma = (s["size0"][J["a0"]] / J["f0"] if mode == 0 else
                 max(s["size0"][J["a0"]] / J["f0"], s["size1"][J["a1"]] / J["f1"])) * 0.125
        pt, valid, _ = mf.triangulate_fast(J["r0"], e0, J["r1"], e1, sigma, mf.Margin())
        d0, d1 = (J["C0"].T @ (pt - J["r0"]))[2], (J["C1"].T @ (pt - J["r1"]))[2]
        near = 0.15 if mode == 0 else 0.075
        facts = {"angle": 0.5 < e0 @ e1 < 0.8, "depth0": abs(d0 - near) < 1e-9, "depth1": abs(d1 - near) < 1e-9,
                 "triangulation": not valid, "ray_valid1": not s["ray_valid1"][J["a1"]]}
        ok = {"angle": valid and min(d0, d1) >= 0.2, "depth0": valid and e0 @ e1 >= 0.8 and d1 >= mf.MIN_DEPTH[mode],
              "depth1": valid and e0 @ e1 >= 0.8 and d0 >= mf.MIN_DEPTH[mode], "triangulation": True,
              "ray_valid1": valid and e0 @ e1 >= 0.8}
        assert facts[reason] and ok[reason], (mode, reason)
    s, lit = scene("distortions")
    assert [c["distortion"] for c in s["cameras"]] == [0, 1, 2, 3] and list(s["job_camera1"]) == [0, 1, 2, 3]
    fails = lit["stats"]["final_failures"]
    assert (3, 40, "invalid") in fails and len([f for f in fails if f[2] == "far"]) >= 4
    for j in range(4):
        assert (mf.job_rows(s, lit, j)["match"] >= 0).sum() >= 25


def test_symbol_and_struct_layouts(og, tmp_path):
    """The entry point is declared and exported; FrameMatchBatch and FrameMatchResult mirror the header."""
    assert "okvisgpu_match_frames" in og.EXPORTED_SYMBOLS
    assert hasattr(og.lib(), "okvisgpu_match_frames")
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    types = {"okvisgpu_frame_match_batch": og.FrameMatchBatch, "okvisgpu_frame_match_result": og.FrameMatchResult}
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
    r = og.FrameMatchResult()
    assert lib.okvisgpu_match_frames(None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.okvisgpu_match_frames(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------ GPU
def _compare(parity, name, got, ref):
    for k in mf.INT_KEYS:
        assert np.array_equal(got[k], ref[k]), (name, k)
    for k in mf.REAL_KEYS:
        parity(f"match_frames/{name}/{k}", mf.worst_relative(got[k], ref[k]), BOUND)


def _run(og, ctx, s, fill=None):
    b, keep = _batch(og, s)
    return ctx.match_frames(b, fill=fill)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_gpu_scene(og, gpu_ctx, parity, name):
    """Every scene against `literal`, the outputs pre-filled so that an element left unwritten shows."""
    s, lit = scene(name)
    got = _run(og, gpu_ctx, s, fill={k: 77 for k in mf.KEYS})
    _compare(parity, name, got, lit)
    check = {"hand": _assert_hand, "ties": _assert_ties, "ties605": _assert_ties605, "blocked": _assert_blocked}.get(name)
    if check:
        check(got)


@pytest.mark.gpu
def test_gpu_batch_independence_and_determinism(og, gpu_ctx):
    """A job alone, as the second of three and in the full batch: identical bytes. Two runs: identical bytes."""
    s, _ = scene("frames")
    full = _run(og, gpu_ctx, s)
    again = _run(og, gpu_ctx, s)
    for k in full:
        assert full[k].tobytes() == again[k].tobytes(), k
    for j in (1, 4):  # a mode-0 and the mode-1 job
        three = mf.sub_scene(s, [0, j, 3])
        alone = mf.sub_scene(s, [j])
        a, b, c = _run(og, gpu_ctx, alone), _run(og, gpu_ctx, three), mf.job_rows(s, full, j)
        for k, v in mf.job_rows(alone, a, 0).items():
            assert v.tobytes() == mf.job_rows(three, b, 1)[k].tobytes() == c[k].tobytes(), (j, k)


@pytest.mark.gpu
def test_gpu_argument_errors(og, gpu_ctx):
    """An out-of-range camera or mode, a broken CSR and a call inside a solve are refused with
    OKVISGPU_ERR_INVALID_ARGUMENT and leave the sentinel-filled outputs alone."""
    s, _ = scene("hand")
    n = int(s["kp0_begin"][-1])

    def refused(change, match):
        t = dict(s)
        for k, (i, v) in change.items():
            t[k] = np.array(s[k]).copy()
            t[k][i] = v
        b, keep = _batch(og, t)
        r = og.FrameMatchResult()
        out = {}
        for k, (shape, dt) in {"match": ((n,), np.int32), "distance": ((n,), np.int32), "point": ((n, 4), np.float64),
                               "initialisable": ((n,), np.uint8), "quality": ((n,), np.float64)}.items():
            out[k] = np.full(shape, 77, dt)
            setattr(r, k, out[k].ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(dt))))
        rc = og.lib().okvisgpu_match_frames(gpu_ctx.h, C.byref(b), C.byref(r))
        assert rc == ERR_INVALID_ARGUMENT
        assert match in og.lib().okvisgpu_last_error(gpu_ctx.h).decode()
        for k, a in out.items():
            assert (a == 77).all(), k

    refused({"job_camera0": (1, 1)}, "job_camera0")
    refused({"job_camera1": (0, -1)}, "job_camera1")
    refused({"job_mode": (1, 2)}, "job_mode")
    refused({"kp0_begin": (1, 9)}, "kp0_begin")
    refused({"kp1_begin": (0, 1)}, "kp1_begin")
    w = og.SynthWindow(10, 500, 4000, seed=78)
    gpu_ctx.set_problems([w.problem])
    gpu_ctx.solve_begin(og.default_options(max_num_iterations=2))
    try:
        refused({}, "solve_end")
    finally:
        gpu_ctx.solve_end()
    _assert_hand(_run(og, gpu_ctx, s))


@pytest.mark.gpu
def test_gpu_empty_batch_and_null_outputs(og, gpu_ctx):
    """n_jobs = 0 returns empty arrays; NULL result pointers are accepted; NULL use arrays mean all 1."""
    got = _run(og, gpu_ctx, mf.sub_scene(scene("hand")[0], []))
    assert all(got[k].size == 0 for k in mf.KEYS)
    s, _ = scene("ties")
    b, keep = _batch(og, s)
    r = og.FrameMatchResult()
    assert og.lib().okvisgpu_match_frames(gpu_ctx.h, C.byref(b), C.byref(r)) == 0
    match = np.full(int(s["kp0_begin"][-1]), 77, np.int32)
    r.match = match.ctypes.data_as(C.POINTER(C.c_int32))
    assert og.lib().okvisgpu_match_frames(gpu_ctx.h, C.byref(b), C.byref(r)) == 0
    _assert_ties({"match": match, "distance": scene("ties")[1]["distance"]})
    assert s["use0"].all() and s["use1"].all()
    got = _run(og, gpu_ctx, {**s, "use0": None, "use1": None})
    _assert_ties(got)
