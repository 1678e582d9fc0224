"""okvisgpu_lidar_deskew and okvisgpu_voxel_downsample: the LiDAR pre-processing of
ThreadedSlam::processFrame (ThreadedSlam.cpp:785-818) on the device: LidarMotionUndistortion::deskew
over the BatchedLidarPropagator (the per-ray states are also Trajectory::getStates') and
VoxelDownSample<float>.

CPU: the two numpy restatements of tests/_lidar.py against each other (bitwise), the per-query form
against _imu_propagate.propagate, a rest case, the reference's own voxel test property, and the
boundary (symbols, NULL arguments, struct layouts). GPU: both calls against the per-query restatement
at the bounds of the functor-level contract: pose, speed and omega_S within 1e-12
max(1, |ref|), point_f64 within 1e-11 max(1, |r_WS|, |ray|), the float point equal to float32(ref) but
for at most 1e-3 of the components, those by one ulp; valid, n_before, keep and n_kept exact."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _imu_propagate as ipr
import _lidar as ld
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
NS = 5_000_000  # 200 Hz
# the bound of the tie to _imu_propagate.propagate: 100 x the largest deviation measured on the CPU
# (test_per_query_form_equals_imu_propagation's docstring)
TIE_MEASURED = 1.0e-15
TIE_BOUND = 100 * TIE_MEASURED
OUTPUTS = ("valid", "point", "point_f64", "pose", "speed", "omega_S", "n_before")


# ------------------------------------------------------------------------------------------ inputs
def _crafted_scans(big=True):
    """The crafted batch: scans by name. 70 scans; `big` adds the scan of 5,000 queries."""
    rng = np.random.default_rng(20261020)
    s = {}
    # N = 2, t_start on sample 0: at t_start as the first point, inside, on the last stamp, beyond it
    s["n2"] = ld.make_scan(rng, 2, 0, [0, 1, 2_500_000, NS - 1, NS, NS, NS + 1, 3 * NS])
    # N = 3, t_start inside interval 0: before t_start, at t_start as first valid and as later points (a run
    # of equal stamps), inside the first interval, one ns either side of a stamp, on stamps, beyond
    t0 = 1_234_567
    s["n3"] = ld.make_scan(rng, 3, t0, [0, t0 - 1, t0, t0, t0, t0 + 1, 3_000_000, 3_000_000, NS - 1, NS, NS + 1,
                                        2 * NS - 1, 2 * NS, 2 * NS + 1, 5 * NS])
    # N = 41, t_start inside interval 3
    t0 = 3 * NS + 2_000_000
    off = np.concatenate([[NS, 3 * NS, t0 - 1], t0 + np.sort(rng.integers(1, 37 * NS - 2_000_000, 150)),
                          np.arange(4, 41) * NS, np.arange(4, 41) * NS - 1, np.arange(4, 40) * NS + 1,
                          [17 * NS + 5] * 4, [40 * NS] * 3, [40 * NS + 1, 50 * NS]])
    s["n41"] = ld.make_scan(rng, 41, t0, off)
    # N = 41, t_start on sample 5, the first point later than t_start
    s["on_sample"] = ld.make_scan(rng, 41, 5 * NS, np.concatenate([[5 * NS + 1, 5 * NS + 1, 6 * NS],
                                                                   rng.integers(5 * NS + 2, 40 * NS, 60)]))
    # a duplicated IMU stamp: ts[5] = ts[4]
    s["dup"] = ld.make_scan(rng, 9, 2 * NS + 7, np.concatenate([[3 * NS, 4 * NS - 1, 4 * NS, 4 * NS + 1, 5 * NS,
                                                                 5 * NS + 1, 6 * NS, 8 * NS],
                                                                rng.integers(2 * NS + 8, 8 * NS, 30)]),
                            duplicate_stamp=4)
    s["no_queries"] = ld.make_scan(rng, 5, 100, [])
    s["nothing"] = ld.make_scan(rng, 2, 0, [])
    s["nothing"]["ts"], s["nothing"]["ga"] = s["nothing"]["ts"][:0], s["nothing"]["ga"][:0]
    for j in range(70 - len(s) - (1 if big else 0)):
        N = int(rng.integers(2, 12))
        t0 = int(rng.integers(0, NS))
        s[f"r{j}"] = ld.make_scan(rng, N, t0, rng.integers(0, (N - 1) * NS + 3, int(rng.integers(1, 9))))
    if big:
        t0 = 777
        s["big"] = ld.make_scan(rng, 41, t0, rng.integers(t0, 40 * NS + 1, 5000))
    return s


@pytest.fixture(scope="module")
def crafted():
    """(Scans, index of every scan by name, the per-query restatement's outputs)."""
    s = _crafted_scans()
    scans = ld.Scans(list(s.values()))
    assert len(scans.scans) == 70
    return scans, {k: i for i, k in enumerate(s)}, scans.reference()


def _voxel_clouds():
    """The crafted clouds by name: (points float32 [n, 3], voxel size, use or None)."""
    rng = np.random.default_rng(87)
    f32 = np.float32
    c = {}
    c["empty"] = (np.zeros((0, 3), f32), 0.1, None)
    c["one"] = (np.array([[1.5, -2.5, 0.25]], f32), 0.1, None)
    c["one_voxel"] = (rng.uniform(0.01, 0.99, (500, 3)).astype(f32), 1.0, None)
    g = np.arange(11, dtype=f32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    c["lattice"] = (lattice, 5.0, None)
    k = np.arange(-40, 41, dtype=f32) * f32(0.05)  # k * 0.05f at voxel 0.05: the correctly rounded quotient
    c["faces"] = (np.stack(np.meshgrid(k, k[:9], k[:3], indexing="ij"), axis=-1).reshape(-1, 3), 0.05, None)
    c["around_zero"] = (np.array([[0.4, 0.4, 0.4], [-0.4, -0.4, -0.4], [0.4, -0.4, 0.4], [-0.6, 0.4, 0.4],
                                  [0.6, 0.4, 0.4]], f32), 0.5, None)  # truncation toward zero: the first three share a voxel
    c["contention"] = ((rng.integers(0, 2, (20000, 3)) + rng.uniform(0.1, 0.9, (20000, 3))).astype(f32), 1.0, None)
    c["spread"] = (rng.uniform(-200, 200, (20000, 3)).astype(f32), 0.05, None)
    twin = rng.uniform(-3, 3, (300, 3)).astype(f32)
    c["twin_a"] = (twin, 0.5, None)
    c["twin_b"] = (twin.copy(), 0.5, None)
    pts = rng.uniform(-2, 2, (400, 3)).astype(f32)
    first = ld.voxel_downsample(pts, 0.5)
    use = np.ones(400, np.uint8)
    use[np.flatnonzero(first)[::2]] = 0  # removes some voxels' first points
    use[rng.integers(0, 400, 40)] = 0
    c["masked"] = (pts, 0.5, use)
    bad = rng.uniform(-1, 1, (64, 3)).astype(f32)
    bad[3, 0], bad[7, 1], bad[11, 2], bad[20, 0], bad[21, 1] = np.nan, np.inf, -np.inf, 1e12, -1e12
    bad[30] = [2147483520.0 * 0.01, 0.0, 0.0]  # the largest float below 2^31, times the voxel size: near the edge
    c["non_finite"] = (bad, 0.01, None)
    return c


def _voxel_pack(clouds):
    begin = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in clouds])]).astype(np.int32)
    points = np.concatenate([p for p, _, _ in clouds]).astype(np.float32).reshape(-1, 3)
    sizes = np.array([v for _, v, _ in clouds], dtype=np.float64)
    use = None
    if any(u is not None for _, _, u in clouds):
        use = np.concatenate([np.ones(len(p), np.uint8) if u is None else u for p, _, u in clouds])
    return begin, points, sizes, use


@pytest.fixture(scope="module")
def voxel_crafted():
    c = _voxel_clouds()
    packed = _voxel_pack(list(c.values()))
    return c, {k: i for i, k in enumerate(c)}, packed, ld.voxel_downsample_clouds(*packed)


# ------------------------------------------------------------------------------------------ CPU
def test_symbols_null_arguments_and_struct_layouts(og, tmp_path):
    """Both entry points are declared, exported and refuse NULL without a device; the four ctypes structs
    mirror the header in size and in every field's offset."""
    lib = og.lib()
    for name in ("okvisgpu_lidar_deskew", "okvisgpu_voxel_downsample"):
        assert name in og.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
        assert getattr(lib, name)(None, None, None) != 0
    out = subprocess.run(["nm", "-D", "--defined-only", og.LIB_PATH], capture_output=True, text=True).stdout
    assert " T okvisgpu_lidar_deskew" in out and " T okvisgpu_voxel_downsample" in out
    if not shutil.which("gcc"):
        pytest.skip("gcc unavailable")
    py = {"okvisgpu_lidar_deskew_batch": og.LidarDeskewBatch, "okvisgpu_lidar_deskew_result": og.LidarDeskewResult,
          "okvisgpu_voxel_downsample_batch": og.VoxelDownsampleBatch,
          "okvisgpu_voxel_downsample_result": og.VoxelDownsampleResult}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {"]
    for t, cls in py.items():
        src.append(f'  printf("{t} %zu\\n", sizeof({t}));')
        for f, _ in cls._fields_:
            src.append(f'  printf("{t}.{f} %zu\\n", offsetof({t}, {f}));')
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for t, cls in py.items():
        assert int(got[t]) == C.sizeof(cls), t
        for f, _ in cls._fields_:
            assert int(got[f"{t}.{f}"]) == getattr(cls, f).offset, (t, f)


def _literal_scans():
    """The crafted scans the literal form can run: without the points at exactly t_start that are not the
    scan's first point (there the reference runs off its IMU deque;
    test_literal_runs_off_the_deque_at_t_start). Scan n2 keeps its first point at t_start."""
    s = _crafted_scans(big=False)
    n3 = s["n3"]
    later = np.flatnonzero(n3["qt"] == n3["t_start"])
    assert later[0] > 0 and s["n2"]["qt"][0] == s["n2"]["t_start"]
    n3["qt"], n3["ray"] = np.delete(n3["qt"], later), np.delete(n3["ray"], later, axis=0)
    return s


def test_literal_and_per_query_forms_agree_bitwise():
    """The reference's serial loop (persistent iterator, t_end_, per-call hasStarted, all bias-Jacobian
    members) and the per-query form give the same values to the last bit: they differ only in terms
    multiplied by Delta_b = 0 and in blends with r = 1."""
    n_valid = 0
    for name, s in _literal_scans().items():
        if len(s["ts"]) == 0:
            continue
        lit = ld.deskew_literal(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"], s["ray"],
                                s["pose_live"], s["T_SL"])
        per = ld.deskew_scan(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"], s["ray"],
                             s["pose_live"], s["T_SL"])
        for k in ("valid", "pose", "speed", "omega_S", "point_f64"):
            assert np.array_equal(lit[k], per[k]), (name, k)
        assert np.isfinite(per["pose"]).all()
        n_valid += int(per["valid"].sum())
    assert n_valid > 500


def test_literal_runs_off_the_deque_at_t_start():
    """The deviation of DESIGN §5: for a point at exactly t_start that is not the scan's first, the
    reference's loop finds no step with dt > 0 and reads past the IMU deque; the per-query form returns
    the state itself."""
    s = _crafted_scans(big=False)["n3"]
    with pytest.raises(ld.RanOffTheDeque):
        ld.deskew_literal(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"], s["ray"], s["pose_live"],
                          s["T_SL"])
    per = ld.deskew_scan(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"])
    at = np.flatnonzero(s["qt"] == s["t_start"])
    assert len(at) == 3 and per["n_before"] == 2
    for i in at:
        assert per["valid"][i] == 1 and per["pose"][i].tobytes() == s["pose0"].tobytes()
        assert per["speed"][i].tobytes() == s["sb0"][:3].tobytes() and not per["omega_S"][i].any()


def test_per_query_form_equals_imu_propagation(og):
    """The per-query form at one query against _imu_propagate.propagate with g = 9.81 over [t_start, T]:
    the same recurrence, up to the sum of the steps' dt against Duration::toSec of the whole span and the
    evaluation order of the position sum.
    Measured on the CPU (seed 41, 40 scans x 12 queries): max |diff| / max(1, |ref|) = 9.99e-16 over pose
    and speed; asserted 100 x 1.0e-15."""
    ip = og.ImuParams()
    ip.a_max, ip.g_max, ip.g = 176.0, 7.8, ld.G
    ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c = 12.0e-4, 8.0e-3, 4.0e-6, 4.0e-5
    rng = np.random.default_rng(41)
    worst, n = 0.0, 0
    for _ in range(40):
        N = int(rng.integers(2, 42))
        t0 = int(rng.integers(0, NS))
        offs = np.concatenate([rng.integers(t0 + 1, (N - 1) * NS + 1, 10), [(N - 1) * NS, NS]])
        s = ld.make_scan(rng, N, t0, offs, reach=5.0)
        per = ld.deskew_scan(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"])
        for i, T in enumerate(s["qt"]):
            steps, T1, sb1, _, _ = ipr.propagate(s["ts"], s["ga"], ip, s["pose0"], s["sb0"], s["t_start"], int(T),
                                                 covariance=False)
            assert steps > 0 and per["valid"][i]
            for got, ref in ((per["pose"][i], T1), (per["speed"][i], sb1[:3])):
                worst = max(worst, (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
            n += 1
    print(f"tie to imu_propagate (CPU): worst {worst:.3e} over {n} queries")
    assert worst <= TIE_BOUND, worst


def test_rest_case():
    """At rest (omega = 0, a = (0, 0, 9.81), v0 = 0, identity attitude, zero biases) every pose is pose0
    and every point is T_live^-1 T_WS0 T_SL ray, within 1e-12 max(1, |.|)."""
    rng = np.random.default_rng(5)
    s = ld.make_scan(rng, 21, 1_000_000, rng.integers(1_000_000, 20 * NS + 1, 200))
    s["pose0"] = np.array([3.0, -2.0, 1.5, 0.0, 0.0, 0.0, 1.0])
    s["sb0"] = np.zeros(9)
    s["ga"] = np.tile([0.0, 0.0, 0.0, 0.0, 0.0, 9.81], (21, 1))
    per = ld.deskew_scan(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"], s["ray"], s["pose_live"],
                         s["T_SL"])
    assert per["valid"].all()
    assert (np.abs(per["pose"] - s["pose0"]) <= 1e-12 * np.maximum(1.0, np.abs(s["pose0"]))).all()
    assert (np.abs(per["speed"]) <= 1e-12).all() and not per["omega_S"].any()
    for i in range(len(s["qt"])):
        ref = ld.transform_point(s["pose_live"], s["pose0"], s["T_SL"], s["ray"][i])
        assert (np.abs(per["point_f64"][i] - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))).all()


def test_voxel_restatement_has_the_references_test_property():
    """okvis_mapping/test/voxelGridTests.cpp:35-88: the 11^3 unit lattice at voxel 5.0 keeps 27 points,
    each an input point and the first of its voxel."""
    pts, size, _ = _voxel_clouds()["lattice"]
    keep = ld.voxel_downsample(pts, size)
    assert keep.sum() == 27
    ok, vox = ld.voxel_of(pts, size)
    assert ok.all()
    for i in np.flatnonzero(keep):
        same = np.flatnonzero((vox == vox[i]).all(axis=1))
        assert same[0] == i
    # truncation toward zero: the voxels around 0 are double width
    pts, size, _ = _voxel_clouds()["around_zero"]
    assert ld.voxel_downsample(pts, size).tolist() == [1, 0, 0, 1, 1]
    # lattice points k * 0.05f at voxel 0.05 sit on voxel faces: the restatement's float32 quotient is the
    # correctly rounded one (the double quotient of two floats rounds to it: 53 >= 2 * 24 + 2 bits)
    pts, size, _ = _voxel_clouds()["faces"]
    _, vox = ld.voxel_of(pts, size)
    exact = (pts.astype(np.float64) / np.float64(np.float32(size))).astype(np.float32)
    assert np.array_equal(vox, np.trunc(exact).astype(np.int32))


# ------------------------------------------------------------------------------------------ GPU
def _compare_deskew(parity, name, got, ref, scans):
    """The device's outputs against the restatement's at the bounds of the module docstring."""
    assert np.array_equal(got["valid"], ref["valid"]) and np.array_equal(got["n_before"], ref["n_before"])
    rel = lambda a, b: (np.abs(a - b) / np.maximum(1.0, np.abs(b))).max() if a.size else 0.0
    for k in ("pose", "speed", "omega_S"):
        parity(f"lidar_deskew/{name}/{k}", rel(got[k], ref[k]), 1e-12)
    if "point_f64" in got:
        scale = np.maximum(1.0, np.maximum(np.linalg.norm(ref["pose"][:, :3], axis=1), np.linalg.norm(scans.ray, axis=1)))
        err = np.abs(got["point_f64"] - ref["point_f64"]).max(axis=1) / scale if len(scale) else np.zeros(1)
        parity(f"lidar_deskew/{name}/point_f64", err.max(), 1e-11)
    if "point" in got:
        _float_points(parity, f"lidar_deskew/{name}/point", got["point"], ref["point"])
    invalid = ref["valid"] == 0
    for k in got:
        if k != "n_before":
            assert not got[k][invalid].any(), k


def _float_points(parity, name, got, ref):
    """Equal float32 values but for components one ulp apart; their share at most 1e-3."""
    assert got.dtype == np.float32 and ref.dtype == np.float32
    differ = got != ref
    if differ.any():
        one_ulp = np.minimum(np.abs(np.nextafter(ref, np.float32(np.inf)) - ref),
                             np.abs(np.nextafter(ref, np.float32(-np.inf)) - ref))
        assert (np.abs(got - ref)[differ] <= one_ulp[differ]).all(), name
    parity(name + "/share_differing", differ.mean() if differ.size else 0.0, 1e-3)


def _deskew(ctx, og, scans, outputs=None, rays=True, fill=None):
    b, keep = scans.batch(og, rays=rays)
    return ctx.lidar_deskew(b, fill=fill, outputs=outputs)


@pytest.mark.gpu
def test_gpu_deskew_crafted_batch(og, gpu_ctx, crafted, parity):
    """The crafted batch of 70 scans (two wavefronts of the chain kernel), one of 5,000 queries (several
    workgroups of the point kernel), against the per-query restatement; twice, for the same bytes."""
    scans, index, ref = crafted
    # the restatement's two association orders of the transform chain stay within the float cap themselves
    alt = np.concatenate([ld.deskew_scan(s["pose0"], s["sb0"], s["t_start"], s["ts"], s["ga"], s["qt"], s["ray"],
                                         s["pose_live"], s["T_SL"], order="vector")["point"]
                          for s in (scans.scans[index["big"]], scans.scans[index["n41"]])])
    same = np.concatenate([ref["point"][scans.query_begin[index[k]]:scans.query_begin[index[k] + 1]]
                           for k in ("big", "n41")])
    _float_points(parity, "lidar_deskew/restatement_orders", alt, same)
    got = _deskew(gpu_ctx, og, scans)
    assert set(got) == set(OUTPUTS)
    _compare_deskew(parity, "crafted", got, ref, scans)
    assert ref["valid"].sum() > 5000 and (ref["valid"] == 0).sum() > 10 and ref["n_before"].sum() > 3
    i = index["n3"]
    q = slice(scans.query_begin[i], scans.query_begin[i + 1])
    at = np.flatnonzero(scans.qt[q] == scans.t_start[i]) + q.start
    assert len(at) == 3
    for j in at:  # pose and speed at t_start are the input bits
        assert got["pose"][j].tobytes() == scans.pose0[i].tobytes()
        assert got["speed"][j].tobytes() == scans.sb0[i, :3].tobytes() and got["valid"][j] == 1
    again = _deskew(gpu_ctx, og, scans)
    for k in OUTPUTS:
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.gpu
def test_gpu_deskew_alone_and_null_outputs(og, gpu_ctx, crafted, parity):
    """A scan alone gives the bytes it gives inside the batch; n_scans = 0; every output NULL in turn, and
    the getStates form without rays."""
    scans, index, ref = crafted
    full = _deskew(gpu_ctx, og, scans)
    for name in ("n2", "n3", "n41", "dup", "big", "r5", "no_queries"):
        i = index[name]
        alone = _deskew(gpu_ctx, og, scans.subset([i]))
        q = slice(scans.query_begin[i], scans.query_begin[i + 1])
        for k in OUTPUTS:
            part = full[k][i:i + 1] if k == "n_before" else full[k][q]
            assert alone[k].tobytes() == part.tobytes(), (name, k)
    none = _deskew(gpu_ctx, og, ld.Scans([]))
    assert all(v.size == 0 for v in none.values())
    small = scans.subset([index[k] for k in ("n3", "n41", "no_queries", "dup")])
    sref = small.reference()
    sfull = _deskew(gpu_ctx, og, small, fill={k: 7 for k in OUTPUTS})
    for drop in OUTPUTS:
        outs = [k for k in OUTPUTS if k != drop]
        got = _deskew(gpu_ctx, og, small, outputs=outs, fill={k: 7 for k in OUTPUTS})
        assert set(got) == set(outs)
        for k in outs:
            assert got[k].tobytes() == sfull[k].tobytes(), (drop, k)
    states = [k for k in OUTPUTS if not k.startswith("point")]
    got = _deskew(gpu_ctx, og, small, rays=False)
    assert set(got) == set(states)
    for k in states:
        assert got[k].tobytes() == sfull[k].tobytes(), k
    _compare_deskew(parity, "small", sfull, sref, small)


@pytest.mark.gpu
def test_gpu_deskew_argument_errors(og, crafted):
    """Each argument error names its offender and leaves the outputs untouched; the calls are refused between
    solve_begin and solve_end."""
    scans, index, _ = crafted
    names = ("n3", "n41", "no_queries", "dup")
    small = scans.subset([index[k] for k in names])
    lib = og.lib()
    ctx = og.Context(0)
    try:
        def refused(match, rays=True, **over):
            b, keep = small.batch(og, rays=rays, **over)
            nq = int(small.query_begin[-1])
            out = {"valid": np.full(nq, 9, np.uint8), "point": np.full((nq, 3), 9, np.float32),
                   "point_f64": np.full((nq, 3), 9.0), "pose": np.full((nq, 7), 9.0), "speed": np.full((nq, 3), 9.0),
                   "omega_S": np.full((nq, 3), 9.0), "n_before": np.full(len(names), 9, np.int32)}
            r = og.LidarDeskewResult()
            og._set_arrays(r, out)
            rc = lib.okvisgpu_lidar_deskew(ctx.h, C.byref(b), C.byref(r))
            assert rc == ERR_INVALID_ARGUMENT
            msg = lib.okvisgpu_last_error(ctx.h).decode()
            assert match in msg, msg
            for k, a in out.items():
                assert (a == 9).all(), k

        late = small.t_start.copy()
        late[1] = small.ts[small.sample_begin[1]] - 1
        refused("scan 1: first sample", t_start=late)
        few = small.sample_begin.copy()
        few[1] = few[0] + 1  # scan 0 keeps one sample
        refused("scan 0 has queries but fewer than two samples", sample_begin=few)
        back = small.qt.copy()
        q1 = small.query_begin[1]
        back[q1 + 4] = back[q1 + 3] - 1
        refused("scan 1: query stamps decrease at query 4", query_t=back)
        ts = small.ts.copy()
        s3 = small.sample_begin[3]
        ts[s3 + 2] = ts[s3 + 1] - 1
        refused("scan 3: sample stamps decrease at sample 2", sample_t=ts)
        bad = small.query_begin.copy()
        bad[2] = bad[1] - 1
        refused("query_begin not monotone at scan 1", query_begin=bad)
        shifted = small.sample_begin.copy()
        shifted[0] = 1
        refused("sample_begin must start at 0", sample_begin=shifted)
        refused("g is not finite", g=float("nan"))
        refused("g is not finite", g=float("inf"))
        refused("ray, pose_live and T_SL", rays=False)

        b, keep = small.batch(og)
        r = og.LidarDeskewResult()
        assert lib.okvisgpu_lidar_deskew(ctx.h, C.byref(b), C.byref(r)) == 0  # every output NULL
        assert lib.okvisgpu_lidar_deskew(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_lidar_deskew(ctx.h, None, C.byref(r)) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_lidar_deskew(ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
        b.n_scans = -1
        assert lib.okvisgpu_lidar_deskew(ctx.h, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        b.n_scans = len(names)
        b.pose0 = None
        assert lib.okvisgpu_lidar_deskew(ctx.h, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT

        vb, vkeep = og.voxel_downsample_batch([0, 2], np.zeros((2, 3), np.float32), [0.1])
        w = og.SynthWindow(10, 500, 4000, seed=78)
        ctx.set_problems([w.problem])
        ctx.solve_begin(og.default_options(max_num_iterations=2))
        try:
            refused("solve_end")
            with pytest.raises(og.OkvisGpuError, match="solve_end"):
                ctx.voxel_downsample(vb)
        finally:
            ctx.solve_end()
        assert ctx.voxel_downsample(vb)["n_kept"].tolist() == [1]
    finally:
        ctx.close()


def _voxel(ctx, og, packed, fill=None):
    begin, points, sizes, use = packed
    b, keep = og.voxel_downsample_batch(begin, points, sizes, use)
    return ctx.voxel_downsample(b, fill=fill)


@pytest.mark.gpu
def test_gpu_voxel_crafted_clouds(og, gpu_ctx, voxel_crafted):
    """The crafted clouds in one batch: keep and n_kept exactly the restatement's; the same bytes on two
    runs and for every cloud alone."""
    clouds, index, packed, (keep, n_kept) = voxel_crafted
    got = _voxel(gpu_ctx, og, packed, fill={"keep": 5, "n_kept": 5})
    assert np.array_equal(got["keep"], keep) and np.array_equal(got["n_kept"], n_kept)
    begin = packed[0]
    expect = {"empty": 0, "one": 1, "one_voxel": 1, "lattice": 27, "around_zero": 3, "contention": 8}
    for name, n in expect.items():
        assert got["n_kept"][index[name]] == n, name
    a, b = index["twin_a"], index["twin_b"]
    assert got["n_kept"][a] == got["n_kept"][b] > 100  # the cloud is part of the key
    assert np.array_equal(got["keep"][begin[a]:begin[a + 1]], got["keep"][begin[b]:begin[b + 1]])
    i = index["non_finite"]
    assert not got["keep"][begin[i]:begin[i + 1]][[3, 7, 11, 20, 21]].any()
    assert got["n_kept"][index["spread"]] > 19000
    again = _voxel(gpu_ctx, og, packed)
    assert got["keep"].tobytes() == again["keep"].tobytes() and got["n_kept"].tobytes() == again["n_kept"].tobytes()
    for name, (pts, size, use) in clouds.items():
        alone = _voxel(gpu_ctx, og, _voxel_pack([(pts, size, use)]))
        i = index[name]
        assert alone["keep"].tobytes() == got["keep"][begin[i]:begin[i + 1]].tobytes(), name
        assert alone["n_kept"][0] == got["n_kept"][i], name
    masked = _voxel(gpu_ctx, og, _voxel_pack([clouds["masked"]]))
    assert not (masked["keep"] & (clouds["masked"][2] == 0)).any()


@pytest.mark.gpu
def test_gpu_voxel_argument_errors(og, gpu_ctx):
    """A voxel size that is not finite and positive names its cloud and leaves the outputs alone; NULL
    outputs and an empty batch are fine."""
    lib = og.lib()
    pts = np.random.default_rng(3).uniform(-1, 1, (10, 3)).astype(np.float32)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        b, keep = og.voxel_downsample_batch([0, 4, 10], pts, [0.1, bad])
        with pytest.raises(og.OkvisGpuError, match="cloud 1"):
            gpu_ctx.voxel_downsample(b)
        out = {"keep": np.full(10, 9, np.uint8), "n_kept": np.full(2, 9, np.int32)}
        r = og.VoxelDownsampleResult()
        og._set_arrays(r, out)
        assert lib.okvisgpu_voxel_downsample(gpu_ctx.h, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        assert (out["keep"] == 9).all() and (out["n_kept"] == 9).all()
    b, keep = og.voxel_downsample_batch([0, 7, 10], pts, [0.1, 0.2])
    with pytest.raises(og.OkvisGpuError, match="monotone at cloud 1"):
        b2, keep2 = og.voxel_downsample_batch([0, 7, 5], pts, [0.1, 0.2])
        gpu_ctx.voxel_downsample(b2)
    r = og.VoxelDownsampleResult()
    assert lib.okvisgpu_voxel_downsample(gpu_ctx.h, C.byref(b), C.byref(r)) == 0  # both outputs NULL
    assert lib.okvisgpu_voxel_downsample(gpu_ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
    assert lib.okvisgpu_voxel_downsample(gpu_ctx.h, None, C.byref(r)) == ERR_INVALID_ARGUMENT
    b.n_clouds = 0
    assert lib.okvisgpu_voxel_downsample(gpu_ctx.h, C.byref(b), C.byref(r)) == 0
    empty = gpu_ctx.voxel_downsample(og.voxel_downsample_batch([0, 0, 0], np.zeros((0, 3), np.float32), [0.1, 0.1])[0],
                                     fill={"n_kept": 5})
    assert empty["n_kept"].tolist() == [0, 0]


@pytest.mark.gpu
def test_gpu_lidar_calls_interleaved_on_one_context(og, crafted, voxel_crafted):
    """deskew, imu_propagate, voxel_downsample and deskew again on one context: each result is, byte for
    byte, what the same call gives alone on a fresh context (the calls share batchScratch)."""
    if og.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    scans, index, _ = crafted
    small = scans.subset([index[k] for k in ("n3", "n41", "no_queries", "dup", "r1", "r2")])
    _, _, packed, _ = voxel_crafted
    ip = og.ImuParams()
    ip.a_max, ip.g_max, ip.g = 176.0, 7.8, 9.81
    ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c = 12.0e-4, 8.0e-3, 4.0e-6, 4.0e-5
    items = ipr.random_items(np.random.default_rng(9), 70)

    def propagate(ctx):
        poses, sbs = items[0].copy(), items[1].copy()
        steps, P, J = ctx.imu_propagate(ip, poses, sbs, *items[2:], covariance=True, jacobian=True)
        return {"steps": steps, "poses": poses, "sbs": sbs, "P": P, "J": J}

    calls = {"deskew": lambda ctx: _deskew(ctx, og, small), "imu_propagate": propagate,
             "voxel": lambda ctx: _voxel(ctx, og, packed)}
    shared = og.Context(0)
    try:
        for name in ("deskew", "imu_propagate", "voxel", "deskew"):
            got = calls[name](shared)
            fresh = og.Context(0)
            try:
                alone = calls[name](fresh)
            finally:
                fresh.close()
            assert got.keys() == alone.keys() and len(got) > 0, name
            for k in got:
                assert got[k].tobytes() == alone[k].tobytes(), (name, k)
    finally:
        shared.close()
