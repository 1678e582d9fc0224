"""TwoPoseExtrinsicsGraphError on the device: okvisgpu_twopose_extrinsics_compute and
okvisgpu_twopose_extrinsics_evaluate (the pose-graph edge of do_extrinsics: true, D = 6 + 6 C).

References (tests/_twopose_extrinsics.py): the oracle's Schur complement of the edge's reprojection
problem with variable extrinsics (H00_, -b0_), the pinned standard kernel okvisgpu_twopose_compute
for the pose block and the outlier / rank / depth rules, and a numpy restatement of
EvaluateWithMinimalJacobians, itself checked against central differences on the CPU.

Tolerances are those of the standard edge (tests/test_gpu_relpose.py), the arithmetic being the same
kind: marginalised system 1e-9 relative to the largest entry (different summation order than the
oracle), against the standard kernel 1e-12 (same per-landmark arithmetic, another order over
landmarks), DeltaX_ 1e-7 relative (condition number of the kept spectrum), evaluation 1e-12 relative
to the block norm, linearisation point 1e-14. J_^T J_ reproduces H00_ up to the reference's own
truncation 1e-8 D max(lambda) of the dropped eigenvalues.
"""
import ctypes as C

import numpy as np
import pytest

import _twopose as tp
import _twopose_extrinsics as tx

IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
MOVED_REF = np.r_[[1.0, -2.0, 0.3], tp.quat_from_axis_angle(np.array([0.1, 0.3, -0.7]))]


def _amax(a):
    return max(float(np.abs(a).max()) if np.size(a) else 0.0, 1e-300)


def _rel(a, b):
    """max |a - b| relative to the largest entry of b."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) / _amax(b) if np.size(b) else 0.0


# ------------------------------------------------------------------------------------- CPU tests
def test_symbols_exported(og):
    for name in ("okvisgpu_twopose_extrinsics_compute", "okvisgpu_twopose_extrinsics_evaluate"):
        assert name in og.EXPORTED_SYMBOLS
        assert hasattr(og.lib(), name)
    assert og.TWOPOSE_MAX_CAMERAS == 6


def test_null_arguments_refused(og):
    L = og.lib()
    d = np.zeros(64)
    u = np.zeros(8, dtype=np.uint8)
    up = u.ctypes.data_as(C.POINTER(C.c_uint8))
    edges = og.TwoPoseEdges()
    ev = og.TwoPoseExtrinsicsEval()
    assert L.okvisgpu_twopose_extrinsics_compute(None, C.byref(edges), og.dptr(d), og.dptr(d), og.dptr(d), up,
                                                 None, None) != 0
    assert L.okvisgpu_twopose_extrinsics_evaluate(None, C.byref(ev), og.dptr(d), None, None, None) != 0
    assert L.okvisgpu_twopose_extrinsics_compute(None, None, og.dptr(d), og.dptr(d), og.dptr(d), up, None, None) != 0
    assert L.okvisgpu_twopose_extrinsics_evaluate(None, None, og.dptr(d), None, None, None) != 0


@pytest.fixture(scope="module")
def cpu_edge(oracle):
    """A computed edge built on the CPU: the oracle's Schur complement decomposed in numpy."""
    e, cams, ex = tp.scene(oracle, 1, n_lm=40)
    H, b0 = tx.schur(oracle, e, cams, ex)
    J, dx = tx.decompose(H, b0)
    return {"edge": e, "ex": ex, "H00": H, "b0": b0, "J": J, "dx": dx,
            "lin": tx.relative_pose(e["ref_pose"], e["other_pose"])}


def test_restatement_at_linearisation_point(cpu_edge):
    """At the compute inputs the error is DeltaX_: r = J_ DeltaX_ and J_^T r = -b0_ (b0_ has no
    component in the dropped directions)."""
    c = cpu_edge
    r, _, _, _ = tx.evaluate(c["edge"]["ref_pose"], c["edge"]["other_pose"], c["ex"], c["dx"], c["J"], c["lin"],
                             c["ex"], [1, 1])
    assert np.abs(r - c["J"] @ c["dx"]).max() <= 1e-12 * _amax(r)
    assert np.abs(c["J"].T @ r + c["b0"]).max() <= 1e-8 * _amax(c["b0"])


def test_restatement_jacobians_numeric(oracle, cpu_edge):
    """jacobiansCorrect semantics (ErrorInterface.cpp:44-163; oracle_check_jacobians): the analytic
    minimal Jacobians of all 2 + C blocks against central differences through the pose manifold's
    plus, away from the linearisation point; bound of tests/test_oracle_twopose.py."""
    c = cpu_edge
    rng = np.random.default_rng(7)
    P = tx.perturbed(oracle, [c["edge"]["ref_pose"], c["edge"]["other_pose"]], rng, 0.05, 0.02)
    X = tx.perturbed(oracle, c["ex"], rng, 0.005, 0.005)
    blocks = [P[0], P[1], X[0], X[1]]

    def ev(bl):
        return tx.evaluate(bl[0], bl[1], np.array(bl[2:]), c["dx"], c["J"], c["lin"], c["ex"], [1, 1])

    r, Jr, Jo, Jx = ev(blocks)
    assert np.abs(r - c["J"] @ c["dx"]).max() > 1e-3 * _amax(r)  # the point is away from the linearisation point
    delta = 1e-7
    for i, Ja in enumerate([Jr, Jo, Jx[0], Jx[1]]):
        Jn = np.zeros_like(Ja)
        for j in range(6):
            d = np.zeros(6)
            d[j] = delta
            bp, bm = list(blocks), list(blocks)
            bp[i], bm[i] = tx.pose_plus(oracle, blocks[i], d), tx.pose_plus(oracle, blocks[i], -d)
            Jn[:, j] = (ev(bp)[0] - ev(bm)[0]) / (2.0 * delta)
        den = min(np.linalg.norm(Ja), np.linalg.norm(Jn))
        assert den > 0
        assert np.linalg.norm(Ja - Jn) / den < 1e-6, i


# ------------------------------------------------------------------------------------- GPU tests
def _compute(og, ctx, edges, cams, ex):
    return ctx.twopose_extrinsics_compute(og.TwoPoseBatch(edges, cams, ex))


@pytest.fixture(scope="module")
def schur_cases(og, oracle, gpu_ctx):
    """The Schur-parity scenes, computed once on the device (one batch) and reduced once by the
    oracle; the evaluation tests reuse them."""
    specs = [(1, 40), (2, 40), (3, 40), (4, 150), (5, 1)]
    edges, refs = [], []
    for seed, n in specs:
        e, cams, ex = tp.scene(oracle, seed, n_lm=n)
        edges.append(e)
        refs.append(tx.schur(oracle, e, cams, ex))
    g = _compute(og, gpu_ctx, edges, cams, ex)
    return {"edges": edges, "cams": cams, "ex": ex, "refs": refs, "gpu": g}


@pytest.fixture(scope="module")
def mixed_scenes(oracle):
    """The scenes of test_gpu_relpose.py::test_twopose_compute_parity: six mixed ones (outliers,
    mono_far, mono_near, up to 155 landmarks), no_other [6], a moved reference keyframe [7]."""
    edges = []
    for seed in range(6):
        e, cams, ex = tp.scene(oracle, 100 + seed, n_lm=30 + 25 * seed, outliers=2 * (seed % 3),
                               mono_far=seed % 2, mono_near=(seed + 1) % 2)
        edges.append(e)
    e, cams, ex = tp.scene(oracle, 200, n_lm=12, no_other=True)
    edges.append(e)
    e, cams, ex = tp.scene(oracle, 201, n_lm=80, ref_pose=MOVED_REF)
    edges.append(e)
    return edges, cams, ex


@pytest.mark.gpu
def test_schur_parity(schur_cases, parity):
    s = schur_cases
    g = s["gpu"]
    D = 18
    for k, (S, b0) in enumerate(s["refs"]):
        H, J, dx = g["H00"][k], g["sqrt_info"][k], g["delta_x"][k]
        parity("twopose_extr.H00_vs_schur", _rel(H, S), 1e-9)
        parity("twopose_extr.b0_vs_schur", _rel(g["b0"][k], b0), 1e-9)
        lam = np.linalg.eigvalsh(S)
        rank = int(tx.kept(lam, D).sum())
        assert int(np.any(J != 0.0, axis=1).sum()) == rank, k
        assert not np.any(J[:D - rank] != 0.0), k  # the zero rows come first (ascending order)
        JtJ = J.T @ J
        bound = 1e-8 * D * lam.max() + 1e-9 * _amax(H)
        parity("twopose_extr.JtJ_vs_H00_over_bound", np.abs(JtJ - H).max() / bound, 1.0)
        parity("twopose_extr.JtJ_dx_plus_b0", np.abs(JtJ @ dx + g["b0"][k]).max() / _amax(g["b0"][k]), 1e-7)
        _, dx0 = tx.decompose(S, b0)
        parity("twopose_extr.delta_x_vs_pinv", _rel(dx, dx0), 1e-7)
        lin = tx.relative_pose(s["edges"][k]["ref_pose"], s["edges"][k]["other_pose"])
        parity("twopose_extr.lin_point", np.abs(g["lin_point"][k] - lin).max(), 1e-14)
        assert np.array_equal(g["camera_seen"][k], [1, 1]), k


@pytest.mark.gpu
def test_pose_block_equals_standard_kernel(og, gpu_ctx, mixed_scenes, parity):
    """Marginalising landmarks only leaves the pose block what TwoPoseStandardGraphError gives: the
    outlier, rank and depth rules and a non-identity T_WS0 carry over from the kernel the oracle pins."""
    edges, cams, ex = mixed_scenes
    batch = og.TwoPoseBatch(edges, cams, ex)
    std = gpu_ctx.twopose_compute(batch)
    g = gpu_ctx.twopose_extrinsics_compute(batch)
    for k in range(len(edges)):
        parity("twopose_extr.pose_block_H00_vs_standard", _rel(g["H00"][k][:6, :6], std["H00"][k]), 1e-12)
        parity("twopose_extr.pose_block_b0_vs_standard", _rel(g["b0"][k][:6], std["b0"][k]), 1e-12)
        assert np.array_equal(g["lin_point"][k], std["lin_point"][k]), k
        assert np.all(np.isfinite(g["sqrt_info"][k])) and np.all(np.isfinite(g["delta_x"][k])), k
    assert np.array_equal(g["lin_point"][6], IDENT)  # no_other
    assert np.array_equal(g["camera_seen"][6], [1, 1])
    assert not np.any(g["H00"][6][:6, :]) and not np.any(g["b0"][6][:6])  # no pose information without S1


@pytest.mark.gpu
def test_outliers_equal_removed_observations(og, oracle, gpu_ctx, parity):
    e, cams, ex = tp.scene(oracle, 11, n_lm=30, outliers=4)
    # scene(): the first `outliers` landmarks' camera-0 observation from the other keyframe is off by (6, -5)
    e2 = tx.drop_observations(e, lambda l, o: l < 4 and o[0] and o[1] == 0)
    assert sum(len(o) for o in e["observations"]) - sum(len(o) for o in e2["observations"]) == 4
    g = _compute(og, gpu_ctx, [e, e2], cams, ex)
    parity("twopose_extr.outliers_H00", _rel(g["H00"][0], g["H00"][1]), 1e-12)
    parity("twopose_extr.outliers_b0", _rel(g["b0"][0], g["b0"][1]), 1e-12)
    # and they did contribute before being dropped: the standard kernel's scene without outliers differs
    clean, _, _ = tp.scene(oracle, 11, n_lm=30)
    gc = _compute(og, gpu_ctx, [clean], cams, ex)
    assert _rel(gc["H00"][0], g["H00"][0]) > 1e-6


@pytest.mark.gpu
def test_mono_landmark_rules(og, oracle, gpu_ctx, parity):
    """Rank-2 landmarks: nearer than 2.99 in S0 they contribute nothing at all (extrinsics blocks
    included); farther they stay in with the clamped pseudo-inverse and everything stays finite."""
    n = 30
    near, cams, ex = tp.scene(oracle, 12, n_lm=n, mono_near=3)
    base = {**near, "landmarks": near["landmarks"][:n], "observations": near["observations"][:n]}
    far, _, _ = tp.scene(oracle, 12, n_lm=n, mono_far=3)
    assert len(near["landmarks"]) == n + 3 and len(far["landmarks"]) == n + 3
    g = _compute(og, gpu_ctx, [near, base, far], cams, ex)
    for key in ("H00", "b0", "delta_x", "sqrt_info"):
        parity("twopose_extr.mono_near_" + key, _rel(g[key][0], g[key][1]), 1e-12)
        assert np.all(np.isfinite(g[key][2])), key
    # (a far one is kept, but its single 2-D observation cancels against its own 3-D marginalisation up
    # to the clamp, so it need not move H00_ measurably: only finiteness is asserted)


@pytest.mark.gpu
def test_rigid_motion_invariance(og, oracle, gpu_ctx, parity):
    e0, cams, ex = tp.scene(oracle, 5, n_lm=30)
    T = np.r_[[3.0, -2.0, 0.5], tp.quat_from_axis_angle(np.array([0.2, -0.4, 1.1]))]
    R = tp.rot(T[3:])

    def move(P):
        return np.r_[R @ P[:3] + T[:3], tx.qmul(T[3:], P[3:])]

    e1 = dict(e0)
    e1["ref_pose"], e1["other_pose"] = move(e0["ref_pose"]), move(e0["other_pose"])
    e1["landmarks"] = np.array([np.r_[R @ l[:3] + T[:3] * l[3], l[3]] for l in e0["landmarks"]])
    g = _compute(og, gpu_ctx, [e0, e1], cams, ex)
    for key in ("H00", "b0", "delta_x", "lin_point"):
        a, b = g[key][0], g[key][1]
        parity("twopose_extr.rigid_motion_" + key, np.abs(a - b).max() / max(1.0, np.abs(a).max()), 1e-8)


@pytest.mark.gpu
def test_camera_counts(og, oracle, gpu_ctx, schur_cases, parity):
    s = schur_cases
    e, cams, ex = s["edges"][0], s["cams"], s["ex"]
    g2 = {k: v[0] for k, v in s["gpu"].items()}
    # C = 1: the left camera alone, D = 12, against the oracle's Schur complement
    left = tx.drop_observations(e, lambda l, o: o[1] != 0)
    g1 = _compute(og, gpu_ctx, [left], cams[:1], ex[:1])
    assert g1["H00"].shape == (1, 12, 12) and np.array_equal(g1["camera_seen"], [[1]])
    S, b0 = tx.schur(oracle, left, cams[:1], ex[:1])
    parity("twopose_extr.C1_H00_vs_schur", _rel(g1["H00"][0], S), 1e-9)
    parity("twopose_extr.C1_b0_vs_schur", _rel(g1["b0"][0], b0), 1e-9)
    _, dx0 = tx.decompose(S, b0)
    parity("twopose_extr.C1_delta_x_vs_pinv", _rel(g1["delta_x"][0], dx0), 1e-7)
    # C = 3: a third camera nobody observes changes no bit of the rest
    g3 = _compute(og, gpu_ctx, [e], cams + [cams[0]], np.vstack([ex, ex[:1]]))
    g3 = {k: v[0] for k, v in g3.items()}
    assert np.array_equal(g3["camera_seen"], [1, 1, 0])
    assert np.array_equal(g3["H00"][:18, :18], g2["H00"])
    assert np.array_equal(g3["b0"][:18], g2["b0"])
    assert np.array_equal(g3["delta_x"][:18], g2["delta_x"])
    assert np.array_equal(g3["sqrt_info"][6:, :18], g2["sqrt_info"])  # 6 more zero rows in front
    assert not np.any(g3["H00"][18:, :]) and not np.any(g3["H00"][:, 18:])
    # J_'s rows belong to eigenvalues (ascending, so the camera's six zero eigenvalues head the list),
    # its columns to parameters: the camera's columns are zero
    assert not np.any(g3["sqrt_info"][:, 18:]) and not np.any(g3["sqrt_info"][:6, :])
    assert not np.any(g3["b0"][18:]) and not np.any(g3["delta_x"][18:])
    assert np.array_equal(g3["lin_point"], g2["lin_point"])


@pytest.mark.gpu
def test_six_cameras(og, oracle, gpu_ctx, parity):
    """C = OKVISGPU_TWOPOSE_MAX_CAMERAS, D = 42: the largest system the LDS layout and the eigen-solve
    take. Three copies of the stereo pair; landmark l is seen by pair l % 3 from the reference and by
    pair (l + 1) % 3 from the other keyframe, so every block fills and the pairs are tied to each
    other (seen by one pair only, the relative pose of the pairs is barely observable and eigenvalues
    land near the threshold; here the spectrum is as clean as the stereo scenes': rank 35, kept
    eigenvalues >= 1.2e-4 max, dropped <= 1e-15 max, checked on the CPU)."""
    e, cams, ex = tp.scene(oracle, 6, n_lm=70)
    obs = [[(o[0], o[1] + 2 * ((l + (1 if o[0] else 0)) % 3)) + tuple(o[2:]) for o in lo]
           for l, lo in enumerate(e["observations"])]
    e6, cams6, ex6 = {**e, "observations": obs}, cams * 3, np.vstack([ex] * 3)
    g = _compute(og, gpu_ctx, [e6], cams6, ex6)
    S, b0 = tx.schur(oracle, e6, cams6, ex6)
    D = 42
    H, J, dx = g["H00"][0], g["sqrt_info"][0], g["delta_x"][0]
    assert H.shape == (D, D) and np.array_equal(g["camera_seen"][0], [1] * 6)
    parity("twopose_extr.C6_H00_vs_schur", _rel(H, S), 1e-9)
    parity("twopose_extr.C6_b0_vs_schur", _rel(g["b0"][0], b0), 1e-9)
    lam = np.linalg.eigvalsh(S)
    ratio = lam / lam.max()
    assert not np.any((ratio > 1e-12) & (ratio < 1e-5)), "the scene's spectrum has no clear gap at the threshold"
    assert int(np.any(J != 0.0, axis=1).sum()) == int(tx.kept(lam, D).sum())
    JtJ = J.T @ J
    parity("twopose_extr.C6_JtJ_vs_H00_over_bound",
           np.abs(JtJ - H).max() / (1e-8 * D * lam.max() + 1e-9 * _amax(H)), 1.0)
    parity("twopose_extr.C6_JtJ_dx_plus_b0", np.abs(JtJ @ dx + g["b0"][0]).max() / _amax(g["b0"][0]), 1e-7)
    parity("twopose_extr.C6_delta_x_vs_pinv", _rel(dx, tx.decompose(S, b0)[1]), 1e-7)


@pytest.mark.gpu
def test_too_many_cameras_unsupported(og, gpu_ctx, schur_cases):
    s = schur_cases
    cams7 = [s["cams"][i % 2] for i in range(7)]
    batch = og.TwoPoseBatch([s["edges"][0]], cams7, np.vstack([s["ex"][i % 2] for i in range(7)]))
    D = 6 + 6 * 7
    out = {"delta_x": np.full((1, D), 7.5), "sqrt_info": np.full((1, D, D), 7.5), "lin_point": np.full((1, 7), 7.5),
           "camera_seen": np.full((1, 7), 9, dtype=np.uint8), "H00": np.full((1, D, D), 7.5), "b0": np.full((1, D), 7.5)}
    rc = og.lib().okvisgpu_twopose_extrinsics_compute(
        gpu_ctx.h, C.byref(batch.struct), og.dptr(out["delta_x"]), og.dptr(out["sqrt_info"]), og.dptr(out["lin_point"]),
        out["camera_seen"].ctypes.data_as(C.POINTER(C.c_uint8)), og.dptr(out["H00"]), og.dptr(out["b0"]))
    assert rc == 2  # OKVISGPU_ERR_UNSUPPORTED
    for k, v in out.items():
        assert np.all(v == (9 if k == "camera_seen" else 7.5)), k
    with pytest.raises(og.OkvisGpuError):
        gpu_ctx.twopose_extrinsics_compute(batch)


@pytest.mark.gpu
def test_batch_independence_and_determinism(og, gpu_ctx, mixed_scenes):
    edges, cams, ex = mixed_scenes
    none = {"ref_pose": edges[7]["ref_pose"], "other_pose": edges[7]["other_pose"], "landmarks": np.zeros((0, 4)),
            "observations": []}
    batch = edges + [none]
    assert len(batch) == 9
    a = _compute(og, gpu_ctx, batch, cams, ex)
    b = _compute(og, gpu_ctx, batch, cams, ex)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    for k in (5, 7, 8):  # 155 landmarks + mono; moved reference; no landmarks
        alone = _compute(og, gpu_ctx, [batch[k]], cams, ex)
        for key in a:
            assert np.array_equal(alone[key][0], a[key][k]), (k, key)
    # an edge without landmarks: all zeros, identity linearisation point, no camera seen
    for key in ("H00", "b0", "delta_x", "sqrt_info", "camera_seen"):
        assert not np.any(a[key][8]), key
    assert np.array_equal(a["lin_point"][8], IDENT)
    # an empty batch is valid
    empty = _compute(og, gpu_ctx, [], cams, ex)
    assert empty["H00"].shape == (0, 18, 18)
    # H00 and b0 may be NULL
    part = {k: np.zeros_like(v) for k, v in a.items()}
    bt = og.TwoPoseBatch(batch, cams, ex)
    rc = og.lib().okvisgpu_twopose_extrinsics_compute(
        gpu_ctx.h, C.byref(bt.struct), og.dptr(part["delta_x"]), og.dptr(part["sqrt_info"]), og.dptr(part["lin_point"]),
        part["camera_seen"].ctypes.data_as(C.POINTER(C.c_uint8)), None, None)
    assert rc == 0
    for key in ("delta_x", "sqrt_info", "lin_point", "camera_seen"):
        assert np.array_equal(part[key], a[key]), key


def _check_eval(g, ref, parity, tag):
    r0, Jr0, Jo0, Jx0 = ref
    parity(f"twopose_extr.eval_r{tag}", np.linalg.norm(g["r"] - r0) / np.linalg.norm(r0), 1e-12)
    parity(f"twopose_extr.eval_J_ref{tag}", np.linalg.norm(g["J_ref"] - Jr0) / np.linalg.norm(Jr0), 1e-12)
    parity(f"twopose_extr.eval_J_other{tag}", np.linalg.norm(g["J_other"] - Jo0) / np.linalg.norm(Jo0), 1e-12)
    for c in range(len(Jx0)):
        n = np.linalg.norm(Jx0[c])
        if n == 0.0:
            assert not np.any(g["J_extrinsics"][c]), c
        else:
            parity(f"twopose_extr.eval_J_extrinsics{tag}", np.linalg.norm(g["J_extrinsics"][c] - Jx0[c]) / n, 1e-12)


@pytest.mark.gpu
def test_evaluate(og, oracle, gpu_ctx, schur_cases, mixed_scenes, parity):
    s = schur_cases
    ex = s["ex"]
    medges, cams, _ = mixed_scenes
    edges = s["edges"] + [medges[7]]  # + the moved reference keyframe
    gm = _compute(og, gpu_ctx, [medges[7]], cams, ex)
    comp = {k: np.concatenate([s["gpu"][k], gm[k]]) for k in gm}
    n = len(edges)
    ref0 = np.array([e["ref_pose"] for e in edges])
    oth0 = np.array([e["other_pose"] for e in edges])

    # at the compute inputs: r = J_ DeltaX_ and J_^T r = -b0_
    g = gpu_ctx.twopose_extrinsics_evaluate(ref0, oth0, ex, comp, ex)
    for k in range(n):
        J, dx, b0 = comp["sqrt_info"][k], comp["delta_x"][k], comp["b0"][k]
        parity("twopose_extr.eval_r_at_lin_point", np.abs(g["r"][k] - J @ dx).max() / _amax(b0), 1e-8)
        parity("twopose_extr.eval_Jt_r_plus_b0", np.abs(J.T @ g["r"][k] + b0).max() / _amax(b0), 1e-8)

    # away from them
    rng = np.random.default_rng(9)
    ref = tx.perturbed(oracle, ref0, rng, 0.05, 0.02)
    oth = tx.perturbed(oracle, oth0, rng, 0.05, 0.02)
    X = tx.perturbed(oracle, ex, rng, 0.005, 0.005)
    g = gpu_ctx.twopose_extrinsics_evaluate(ref, oth, X, comp, ex)
    for k in range(n):
        want = tx.evaluate(ref[k], oth[k], X, comp["delta_x"][k], comp["sqrt_info"][k], comp["lin_point"][k], ex,
                           comp["camera_seen"][k])
        _check_eval({key: v[k] for key, v in g.items()}, want, parity, "")

    # NULL outputs are accepted one at a time, and the others do not change
    names = ("r", "J_ref", "J_other", "J_extrinsics")
    for skip in names:
        want = tuple(x for x in names if x != skip)
        part = gpu_ctx.twopose_extrinsics_evaluate(ref, oth, X, comp, ex, want=want)
        assert set(part) == set(want)
        for key in want:
            assert np.array_equal(part[key], g[key]), (skip, key)


@pytest.mark.gpu
def test_evaluate_unseen_camera(og, oracle, gpu_ctx, schur_cases, parity):
    s = schur_cases
    cams3, ex3 = s["cams"] + [s["cams"][0]], np.vstack([s["ex"], s["ex"][:1]])
    e = s["edges"][1]
    comp = _compute(og, gpu_ctx, [e], cams3, ex3)
    assert np.array_equal(comp["camera_seen"], [[1, 1, 0]])
    rng = np.random.default_rng(10)
    ref = tx.perturbed(oracle, [e["ref_pose"]], rng, 0.05, 0.02)
    oth = tx.perturbed(oracle, [e["other_pose"]], rng, 0.05, 0.02)
    X = tx.perturbed(oracle, ex3, rng, 0.005, 0.005)  # the unseen camera's block moves too
    g = gpu_ctx.twopose_extrinsics_evaluate(ref, oth, X, comp, ex3)
    assert not np.any(g["J_extrinsics"][0][2])
    want = tx.evaluate(ref[0], oth[0], X, comp["delta_x"][0], comp["sqrt_info"][0], comp["lin_point"][0], ex3, [1, 1, 0])
    _check_eval({key: v[0] for key, v in g.items()}, want, parity, "_unseen")
    # its r contribution is exactly 0: the same edge with C = 2 gives the same bits
    comp2 = {k: v[1:2] for k, v in s["gpu"].items()}
    g2 = gpu_ctx.twopose_extrinsics_evaluate(ref, oth, X[:2], comp2, s["ex"])
    assert np.array_equal(g["r"][0][6:], g2["r"][0])
    assert not np.any(g["r"][0][:6])
