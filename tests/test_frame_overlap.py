"""okvisgpu_frame_overlap: the keypoint-coverage masks of ViSlamBackend::overlapFraction (kind 0), the two
parts of Frontend::doWeNeedANewKeyframe (kinds 1 and 2) and ViSlamBackend::trackingQuality (kind 3) on the
device.

CPU: the disc tables of the contract, the literal circle routine against the table form under clipping, the
centre conversion at its ties, properties of the restatement (tests/_overlap.py) and the boundary (symbol,
NULL arguments, struct layouts, a C99 consumer). GPU: every output against the restatement, counts with ==
and doubles bit for bit, NaN included."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _overlap as ov
from _paths import REPO

ERR_INVALID_ARGUMENT = 1
TABLES = {0: [0], 1: [1, 0], 2: [2, 1, 0], 3: [3, 2, 2, 0], 4: [4, 3, 3, 2, 0], 5: [5, 4, 4, 4, 3, 0],
          6: [6, 5, 5, 5, 4, 3, 0], 10: [10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0]}


# ------------------------------------------------------------------------------------------ inputs
def _special_points(rows, cols):
    """Corners, edges, negative coordinates, points beyond the width and the height, the tie centres."""
    return np.array([[0, 0], [cols - 1, rows - 1], [0, rows - 1], [cols - 1, 0], [cols / 2, 0], [0, rows / 2],
                     [cols - 0.5, rows / 3], [cols / 3, rows - 0.5], [-3.2, -7.7], [-44.0, 100.0], [100.0, -39.0],
                     [cols + 30, 100], [100, rows + 44], [cols + 300, rows + 300], [5.0, 15.0], [25.0, 35.0],
                     [45.0, 5.0], [cols - 7.0, 25.0], [cols - 0.1, rows - 0.1], [35.0, rows - 5.0]], np.float32)


def _frame(rng, rows, cols, n, pool, n_images=2, base=1):
    """A frame of n_images images with n keypoints each: about a third of the keypoints carry an id of `pool`
    (shared across frames, so an id can sit on two keypoints and on both cameras), a third an id of their
    own, a third none."""
    images = []
    for _ in range(n_images):
        kp = np.column_stack([rng.uniform(-15, cols + 15, n), rng.uniform(-15, rows + 15, n)]).astype(np.float32)
        sp = _special_points(rows, cols)[:n]
        kp[:len(sp)] = sp
        which = rng.integers(0, 3, n)
        lm = np.where(which == 0, rng.choice(pool, n), 0).astype(np.uint64)
        own = np.uint64(base) + rng.integers(0, 1 << 30, n).astype(np.uint64)
        lm = np.where(which == 1, own, lm).astype(np.uint64)
        images.append(ov.image(rows, cols, kp, lm, rng.integers(0, 2, n)))
    return images


def _case1_frames():
    rng = np.random.default_rng(20261021)
    pool = np.concatenate([np.arange(1, 121), (1 << 41) + np.arange(7, 67) * 1024]).astype(np.uint64)
    return [_frame(rng, 480, 752, 300, pool, base=(1 << 33) * (f + 1)) for f in range(6)]


@pytest.fixture(scope="module")
def case1():
    """6 frames x 2 images of 752 x 480 (grid 48 x 75: three words per row), 300 keypoints per image, all 30
    ordered pairs at factor 0.09 (R = 4): (frames, jobs, the restatement's outputs)."""
    frames = _case1_frames()
    jobs = [(0, a, b, 0.09) for a in range(6) for b in range(6) if a != b]
    return frames, jobs, ov.reference(frames, jobs)


def _batch(og, frames, jobs, group_begin=None, flag=True, **over):
    a = ov.pack(frames)
    a.update(job_kind=[j[0] for j in jobs], job_frame_a=[j[1] for j in jobs], job_frame_b=[j[2] for j in jobs],
             job_radius_factor=[j[3] for j in jobs], group_begin=group_begin)
    if not flag:
        a["flag"] = None
    a.update(over)
    return og.frame_overlap_batch(**a)


def _run(ctx, og, frames, jobs, group_begin=None, fill=None, **over):
    b, keep = _batch(og, frames, jobs, group_begin, **over)
    return ctx.frame_overlap(b, fill=fill)


def _same(got, ref, where=""):
    """Counts with ==, doubles bit for bit."""
    for k, r in ref.items():
        g = got[k]
        if r.dtype == np.float64:
            assert np.array_equal(ov.bits(g), ov.bits(r)), (where, k, g, r)
        else:
            assert g.dtype == r.dtype and np.array_equal(g, r), (where, k, g, r)


FILL = {"overlap": 9.0, "count": 9, "n_matched": 9, "n_keypoints": 9, "group_best": 9, "group_max": 9.0}


# ------------------------------------------------------------------------------------------ CPU
def test_half_width_tables_and_the_r4_disc():
    for radius, table in TABLES.items():
        assert ov.half_widths(radius) == table, radius
    img = np.zeros((21, 21), np.uint8)
    ov.circle(img, 10, 10, 4)
    assert np.count_nonzero(img) == 49
    assert [int(np.count_nonzero(row)) for row in img[6:15]] == [1, 5, 7, 7, 9, 7, 7, 5, 1]


def test_literal_circle_equals_the_table_form_under_clipping():
    rng = np.random.default_rng(1)
    for trial in range(2000):
        height, width = int(rng.integers(1, 60)), int(rng.integers(1, 90))
        radius = int(rng.integers(0, 12))
        cx, cy = int(rng.integers(-14, width + 14)), int(rng.integers(-14, height + 14))
        a = np.zeros((height, width), np.uint8)
        b = np.zeros((height, width), np.uint8)
        ov.circle(a, cx, cy, radius)
        ov.table_disc(b, cx, cy, radius)
        assert np.array_equal(a, b), (height, width, radius, cx, cy)
    e = np.zeros((0, 0), np.uint8)
    ov.circle(e, 3, 3, 2)  # a grid without pixels takes any disc


def test_centre_conversion_at_its_ties():
    for pt, c in ((5.0, 0), (15.0, 2), (25.0, 2), (35.0, 4), (45.0, 4), (745.0, 74), (751.9, 75), (-5.0, 0),
                  (-15.0, -2), (-7.7, -1)):
        assert ov.centre(pt) == c, pt
    assert ov.centre(float("nan")) is None and ov.centre(float("inf")) is None and ov.centre(3.0e10) is None
    img = np.zeros((48, 75), np.uint8)
    ov.paint(img, (751.9, 100.0), 0)  # centre 75: off a 75-column grid
    assert not img.any()


def test_restatement_properties(case1):
    frames, jobs, ref = case1
    # every keypoint carries a landmark: overlapFraction(A, A) is 1.0
    full = [ov.image(im["rows"], im["cols"], im["kp"], np.arange(1, len(im["kp"]) + 1) + 1000 * i)
            for i, im in enumerate(frames[0])]
    v, count, n_matched = ov.overlap_fraction(full, full, 0.09)
    assert v == 1.0 and count[0] == count[1] == count[2] == count[3] > 0 and n_matched == [600, 600]
    # no common id: exactly 0.0, the counts as painted
    other = [ov.image(im["rows"], im["cols"], im["kp"], im["lm"] + np.uint64(1 << 50)) for im in full]
    v, count, n_matched = ov.overlap_fraction(full, other, 0.09)
    assert v == 0.0 and count[0] == 0 and count[1] > 0 and n_matched == [0, 0]
    # matches within detections, in every generated case: I = popcount(matches)
    for fr in frames:
        for im in fr:
            det = ov._detections(im, 0.09)
            mat = np.zeros_like(det)
            for k in np.flatnonzero(im["lm"]):
                ov.paint(mat, im["kp"][k], 4)
            assert not (mat & ~det).any()
    assert (ref["count"][:, 0] <= ref["count"][:, 1]).all() and (ref["count"][:, 2] <= ref["count"][:, 3]).all()
    assert (ref["overlap"] > 0).all() and (ref["overlap"] < 1).all()  # the pairs do share landmarks
    # 0 / 0 as the contract states it
    assert ov.bits(ov._ratio(0, 0)) == ov.NAN_BITS


def test_symbol_null_arguments_and_struct_layouts(og, tmp_path):
    """The entry point is declared, exported and refuses NULL without a device; the two ctypes structs mirror
    the header in size and in every field's offset (a C99 program under -Wall -Werror -pedantic prints them)."""
    lib = og.lib()
    assert "okvisgpu_frame_overlap" in og.EXPORTED_SYMBOLS
    b, r = og.FrameOverlapBatch(), og.FrameOverlapResult()
    assert lib.okvisgpu_frame_overlap(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
    assert lib.okvisgpu_frame_overlap(None, None, None) == ERR_INVALID_ARGUMENT
    out = subprocess.run(["nm", "-D", "--defined-only", og.LIB_PATH], capture_output=True, text=True).stdout
    assert " T okvisgpu_frame_overlap" in out
    py = {"okvisgpu_frame_overlap_batch": og.FrameOverlapBatch, "okvisgpu_frame_overlap_result": og.FrameOverlapResult}
    src = ["#include <stdio.h>", "#include <stddef.h>", '#include "okvisgpu.h"', "int main(void) {"]
    for t, cls in py.items():
        src.append(f'  printf("{t} %lu\\n", (unsigned long)sizeof({t}));')
        for f, _ in cls._fields_:
            src.append(f'  printf("{t}.{f} %lu\\n", (unsigned long)offsetof({t}, {f}));')
    src += ["  return 0;", "}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines())
    for t, cls in py.items():
        assert int(got[t]) == C.sizeof(cls), t
        for f, _ in cls._fields_:
            assert int(got[f"{t}.{f}"]) == getattr(cls, f).offset, (t, f)


@pytest.fixture(scope="module")
def consumer(og, tmp_path_factory):
    """tests/cpp/overlap_consumer.c built as C99 under -Wall -Werror -pedantic and linked against the library."""
    exe = tmp_path_factory.mktemp("overlap") / "overlap_consumer"
    libdir = os.path.dirname(og.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    os.path.join(REPO, "tests", "cpp", "overlap_consumer.c"), "-o", str(exe), "-L", libdir, "-lokvisgpu",
                    "-Wl,-rpath," + libdir], check=True)
    return str(exe)


def test_c99_consumer_without_a_device(consumer):
    run = subprocess.run([consumer], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "null context refused" in run.stdout


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_c99_consumer(consumer):
    """The consumer's one kind-0 job: frame 0 = {7, -, 9}, frame 1 = {7, 11, 9}, so M = {7, 9}."""
    import json
    run = subprocess.run([consumer, "gpu"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got = json.loads(run.stdout.strip().splitlines()[-1])
    a = [ov.image(480, 752, [[100, 100], [300, 200]], [7, 0]), ov.image(480, 752, [[50, 60]], [9])]
    b = [ov.image(480, 752, [[110, 95], [700, 400]], [7, 11]), ov.image(480, 752, [[55, 66]], [9])]
    ref = ov.reference([a, b], [(0, 0, 1, 0.09)], [0, 1])
    assert got["count"] == ref["count"][0].tolist() == [98, 147, 98, 147]
    assert got["n_matched"] == [2, 2] and got["n_keypoints"] == 3 and got["group_best"] == 0
    assert got["overlap"] == ref["overlap"][0] == got["group_max"] == 98 / 147


@pytest.mark.gpu
def test_gpu_kind0_all_ordered_pairs(og, gpu_ctx, case1):
    """Case 1: the 30 ordered pairs, every output the restatement's."""
    frames, jobs, ref = case1
    got = _run(gpu_ctx, og, frames, jobs, fill=FILL)
    _same(got, ref)
    assert (got["n_matched"] > 30).all() and len(set(got["overlap"].tolist())) > 10


@pytest.mark.gpu
def test_gpu_larger_discs_across_word_boundaries(og, gpu_ctx):
    """1300 x 500 at factor 0.2: a 50 x 130 grid (five words per row), R = 10."""
    rng = np.random.default_rng(5)
    pool = np.arange(1, 150).astype(np.uint64)
    frames = [_frame(rng, 500, 1300, 300, pool, base=(1 << 33) * (f + 1)) for f in range(3)]
    jobs = [(0, a, b, 0.2) for a in range(3) for b in range(3) if a != b]
    _same(_run(gpu_ctx, og, frames, jobs, fill=FILL), ov.reference(frames, jobs))


@pytest.mark.gpu
def test_gpu_other_radii(og, gpu_ctx, case1):
    """Factor 0.001 (R = 0: single pixels) and 0.13 (R = 6), and both in one batch with R = 4."""
    frames = case1[0][:3]
    jobs = [(0, a, b, f) for f in (0.001, 0.13) for a in range(3) for b in range(3) if a != b] + [(0, 0, 1, 0.09)]
    ref = ov.reference(frames, jobs)
    _same(_run(gpu_ctx, og, frames, jobs, fill=FILL), ref)
    assert (ref["count"][:6, 1] <= 600).all()  # R = 0: at most one pixel per keypoint


@pytest.mark.gpu
def test_gpu_kind0_degenerate_cases(og, gpu_ctx, case1):
    """An empty image on one camera, a frame without keypoints, a pair without a common id, A = B, and a pair
    whose common landmark sits on keypoints that are all off the grid on one side (0 / 0 and std::min)."""
    f0, f1 = case1[0][0], case1[0][1]
    none = np.zeros((0, 2), np.float32)
    ids = lambda n, at: np.arange(at, at + n).astype(np.uint64)
    # camera 1 is empty but still lists keypoints with ids that frame 1 knows: they take no part
    empty_cam = [f0[0], ov.image(0, 0, f1[1]["kp"][:40], f1[1]["lm"][:40])]
    no_kp = [ov.image(480, 752, none, []), ov.image(480, 752, none, [])]
    strangers = [ov.image(480, 752, im["kp"], ids(300, (1 << 52) + 1000 * i)) for i, im in enumerate(f0)]
    off = np.array([[-400.0, -400.0], [9000.0, 100.0], [100.0, 9000.0]], np.float32)
    off_grid = [ov.image(480, 752, off, [77, 78, 0]), ov.image(480, 752, off, [0, 0, 79])]
    on_grid = [ov.image(480, 752, [[100, 100], [300, 200]], [77, 5]), ov.image(480, 752, [[50, 60]], [6])]
    frames = [f0, f1, empty_cam, no_kp, strangers, off_grid, on_grid]
    jobs = [(0, 2, 1, 0.09), (0, 1, 2, 0.09), (0, 3, 0, 0.09), (0, 0, 3, 0.09), (0, 3, 3, 0.09), (0, 0, 4, 0.09),
            (0, 4, 0, 0.09), (0, 0, 0, 0.09), (0, 4, 4, 0.09), (0, 5, 6, 0.09), (0, 6, 5, 0.09), (0, 5, 5, 0.09)]
    ref = ov.reference(frames, jobs)
    got = _run(gpu_ctx, og, frames, jobs, fill=FILL)
    _same(got, ref)
    o = got["overlap"]
    assert 0 < o[0] < 1 and got["count"][0, 1] > 0  # the empty camera's ids did not enter M
    assert ov.bits(o[2:7]).tolist() == [0] * 5  # no common id: exactly 0.0 ...
    assert got["count"][5, 1] > 0 and got["count"][5, 0] == 0  # ... with the counts as painted
    assert o[7] < 1.0 and o[8] == 1.0  # A = B: 1.0 once every keypoint carries a landmark
    # side A off the grid: 0 / 0 is o_A and (o_B < NaN) is false; as side B the NaN loses to the number
    assert ov.bits(o[9]) == ov.NAN_BITS and got["count"][9].tolist()[:2] == [0, 0]
    assert o[10] == got["count"][10, 0] / got["count"][10, 1] and 0 < o[10] < 1
    assert ov.bits(o[11]) == ov.NAN_BITS


@pytest.mark.gpu
def test_gpu_ids(og, gpu_ctx):
    """Ids above 2^40, one id on several keypoints and on both cameras, and frames whose ids are all congruent
    modulo the table size (256 keypoints: 512 slots) at several strides."""
    rng = np.random.default_rng(11)
    pts = lambda n: np.column_stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)])
    big, top = (1 << 40) + 12345, np.uint64(1 << 63)
    u = lambda *parts: np.concatenate([np.asarray(q, dtype=np.uint64) for q in parts])
    a = [ov.image(480, 752, pts(128), u([big] * 5, top + np.arange(123, dtype=np.uint64))),
         ov.image(480, 752, pts(128), u([big] * 3, [0] * 125))]
    b = [ov.image(480, 752, pts(128), u([7, big], [0] * 126)),
         ov.image(480, 752, pts(128), top + np.arange(60, 188, dtype=np.uint64))]
    frames = [a, b]
    for stride in (512, 1 << 20, 1 << 32, 0x9E3779B97F4A7C15 % (1 << 50)):
        with np.errstate(over="ignore"):
            lm = np.uint64(3) + np.arange(256, dtype=np.uint64) * np.uint64(stride)
        frames.append([ov.image(480, 752, pts(128), lm[:128]), ov.image(480, 752, pts(128), lm[128:])])
        half = lm.copy()
        half[::2] += np.uint64(1)  # every other id differs in its lowest bit only
        frames.append([ov.image(480, 752, pts(128), half[:128]), ov.image(480, 752, pts(128), half[128:])])
    n = len(frames)
    jobs = [(0, 0, 1, 0.09), (0, 1, 0, 0.09)] + [(0, i, i + 1, 0.09) for i in range(2, n, 2)] + \
           [(0, i + 1, i, 0.09) for i in range(2, n, 2)] + [(1, 0, 1, 0.09), (0, 2, 4, 0.09)]
    ref = ov.reference(frames, jobs)
    got = _run(gpu_ctx, og, frames, jobs, fill=FILL)
    _same(got, ref)
    assert got["n_matched"][0].tolist() == [8 + 63, 1 + 63]
    assert (got["n_matched"][2:6] == 128).all()  # half of each strided frame's ids are shared


@pytest.mark.gpu
def test_gpu_kinds_1_and_2_and_group_max(og, gpu_ctx, case1):
    """doWeNeedANewKeyframe: the current frame (kind 2) and the other-frames loop (kind 1) as one group whose
    group_max ignores the NaN of a frame without keypoints."""
    frames = list(case1[0][:4])
    none = np.zeros((0, 2), np.float32)
    frames.append([ov.image(480, 752, none, []), ov.image(480, 752, none, [])])  # 0 / 0
    frames.append([case1[0][4][0], ov.image(0, 0, case1[0][1][1]["kp"][:30], case1[0][1][1]["lm"][:30])])
    jobs = [(2, 0, 0, 0.09), (2, 4, 0, 0.09), (2, 5, 0, 0.09)] + [(1, 0, b, 0.09) for b in (1, 4, 2, 3)] + \
           [(1, 5, 1, 0.09), (1, 1, 5, 0.09), (1, 4, 1, 0.09)]
    groups = [0, 3, 7, 8, 10]
    ref = ov.reference(frames, jobs, groups)
    got = _run(gpu_ctx, og, frames, jobs, groups, fill=FILL)
    _same(got, ref)
    assert ov.bits(got["overlap"][[1, 4]]).tolist() == [ov.NAN_BITS] * 2
    assert got["group_max"][1] == np.nanmax(got["overlap"][3:7]) > 0
    assert got["n_keypoints"].tolist()[:3] == [600, 0, 330]
    # kind 1 reads the ids of A's empty image too (:1219; kind 0 does not, :2922): frame 1 finds its own there
    assert got["n_matched"][7, 1] >= np.count_nonzero(case1[0][1][1]["lm"][:30]) > 0


@pytest.mark.gpu
def test_gpu_kind3_tracking_quality(og, gpu_ctx):
    """7 flagged keypoints give 0.0 and 8 the ratio; one flagged keypoint at R = 4 paints 49 - 50, clamped to 0;
    a flag on a keypoint without an id is honoured."""
    rng = np.random.default_rng(3)
    n = 60
    pts = lambda: np.column_stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)])

    def frame(n_flagged):
        flag = np.zeros(2 * n, np.uint8)
        flag[rng.choice(2 * n, n_flagged, replace=False)] = 1
        return [ov.image(480, 752, pts(), np.zeros(n), flag[:n]), ov.image(480, 752, pts(), np.arange(1, n + 1), flag[n:])]

    one = [ov.image(400, 752, [[300.0, 200.0], [100.0, 100.0]], [0, 9], [1, 0])]  # grid 40 x 75: radius 4.0 at 0.1
    frames = [frame(7), frame(8), frame(40), one, [ov.image(0, 0, [[1.0, 1.0]] * 9, [0] * 9, [1] * 9)]]
    jobs = [(3, f, 0, 0.09) for f in range(5)] + [(3, 2, 0, 0.13), (3, 2, 0, 0.001), (3, 3, 0, 0.1)]
    ref = ov.reference(frames, jobs)
    got = _run(gpu_ctx, og, frames, jobs, fill=FILL)
    _same(got, ref)
    assert got["n_matched"][:, 0].tolist()[:5] == [7, 8, 40, 1, 9]
    assert ov.bits(got["overlap"][0]) == 0 and got["count"][0, 0] > 0
    assert got["overlap"][1] == got["count"][1, 0] / got["count"][1, 1] > 0
    assert got["count"][7].tolist() == [0, 40 * 75 - 50, 0, 0]  # 49 pixels - int(16 pi), clamped
    assert ov.bits(got["overlap"][4]) == ov.NAN_BITS  # nine flags on an empty image: 0 / 0


@pytest.mark.gpu
def test_gpu_group_best(og, gpu_ctx, case1):
    """Equal overlaps: the last wins; all 0.0: the last wins; an empty and an all-NaN group: -1."""
    frames = list(case1[0][:3])
    strangers = [ov.image(480, 752, im["kp"], np.arange(1, 301).astype(np.uint64) + np.uint64((1 << 52) + 1000 * i))
                 for i, im in enumerate(frames[0])]
    none = np.zeros((0, 2), np.float32)
    frames += [strangers, [ov.image(480, 752, none, []), ov.image(480, 752, none, [])]]
    jobs = [(0, 1, 0, 0.09), (0, 2, 0, 0.09), (0, 1, 0, 0.09), (0, 3, 0, 0.09),  # equal overlaps at 0 and 2
            (0, 3, 0, 0.09), (0, 3, 1, 0.09), (0, 3, 2, 0.09),  # all 0.0
            (2, 4, 0, 0.09), (2, 4, 0, 0.09),  # all NaN
            (0, 2, 0, 0.09), (2, 4, 0, 0.09), (0, 1, 0, 0.09)]
    groups = [0, 4, 7, 7, 9, 12]
    ref = ov.reference(frames, jobs, groups)
    got = _run(gpu_ctx, og, frames, jobs, groups, fill=FILL)
    _same(got, ref)
    o = got["overlap"]
    assert o[0] == o[2] and got["group_best"].tolist()[1:4] == [6, -1, -1]
    assert got["group_best"][0] == (2 if o[0] >= o[1] else 1) and got["group_best"][4] in (9, 11)
    assert ov.bits(got["group_max"]).tolist()[1:4] == [0, 0, 0]


@pytest.mark.gpu
def test_gpu_batch_independence_and_repeatability(og, gpu_ctx, case1):
    """Every job of case 1 alone gives the bits it gives inside the batch; the batch twice gives the same bytes."""
    frames, jobs, ref = case1
    first = _run(gpu_ctx, og, frames, jobs)
    again = _run(gpu_ctx, og, frames, jobs)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    for j, job in enumerate(jobs):
        alone = _run(gpu_ctx, og, frames, [job])
        for k in ("overlap", "count", "n_matched", "n_keypoints"):
            assert alone[k][0].tobytes() == first[k][j].tobytes(), (j, k)


@pytest.mark.gpu
def test_gpu_argument_errors(og, case1):
    """Each argument error returns its code, names its offender and leaves the pre-filled outputs untouched;
    valid edge batches pass; the call is refused between solve_begin and solve_end, and a solve around such a
    call gives the bits of a solve without it."""
    frames = list(case1[0][:2]) + [[case1[0][2][0]]]  # frame 2 has one image
    jobs = [(0, 0, 1, 0.09), (1, 0, 1, 0.09), (2, 2, 0, 0.09), (3, 1, 0, 0.09)]
    groups = [0, 2, 4]
    lib = og.lib()
    ctx = og.Context(0)
    try:
        def refused(match, jobs=jobs, groups=groups, **over):
            b, keep = _batch(og, frames, jobs, groups, **over)
            nj, ng = b.n_jobs, b.n_groups
            out = {"overlap": np.full(nj, 9.0), "count": np.full((nj, 4), 9, np.int32),
                   "n_matched": np.full((nj, 2), 9, np.int32), "n_keypoints": np.full(nj, 9, np.int32),
                   "group_best": np.full(ng, 9, np.int32), "group_max": np.full(ng, 9.0)}
            r = og.FrameOverlapResult()
            og._set_arrays(r, out)
            rc = lib.okvisgpu_frame_overlap(ctx.h, C.byref(b), C.byref(r))
            assert rc == ERR_INVALID_ARGUMENT, (match, rc)
            msg = lib.okvisgpu_last_error(ctx.h).decode()
            assert match in msg, msg
            for k, a in out.items():
                assert (a == 9).all(), (match, k)

        p = ov.pack(frames)
        job = lambda kind, a, b, f: [(kind, a, b, f)] + jobs[1:]
        bad = p["image_begin"].copy()
        bad[0] = 1
        refused("image_begin must start at 0", image_begin=bad)
        bad = p["kp_begin"].copy()
        bad[3] = bad[2] - 1
        refused("kp_begin not monotone at image 2", kp_begin=bad)
        refused("group_begin not monotone at group 1", groups=[0, 3, 2])
        refused("group_begin must start at 0", groups=[1, 2, 4])
        refused("group_begin exceeds n_jobs", groups=[0, 2, 5])
        bad = p["rows"].copy()
        bad[1] = -480
        refused("negative rows or cols of image 1", rows=bad)
        bad = p["cols"].copy()
        bad[4] = -1
        refused("negative rows or cols of image 4", cols=bad)
        refused("job 0: frame_a 3 out of range", jobs=job(0, 3, 1, 0.09))
        refused("job 0: frame_a -1 out of range", jobs=job(2, -1, 0, 0.09))
        refused("job 0: frame_b 7 out of range", jobs=job(1, 0, 7, 0.09))
        refused("job 0: unknown kind 4", jobs=job(4, 0, 1, 0.09))
        refused("job 0: unknown kind -1", jobs=job(-1, 0, 1, 0.09))
        refused("job 0: frames 0 and 2 differ in image count", jobs=job(0, 0, 2, 0.09))
        refused("job 3: kind 3 needs flag", flag=False)
        for f in (float("nan"), float("inf"), -0.01):
            refused("job 0: radius factor is not finite and >= 0", jobs=job(0, 0, 1, f))
        refused("job 0: radius above OKVISGPU_OVERLAP_MAX_RADIUS on image 0", jobs=job(0, 0, 1, 30.0))
        bad = p["cols"].copy()
        bad[2] = 56000  # 48 rows x 175 words
        refused("image 2: a 48 x 5600 grid needs more than OKVISGPU_OVERLAP_MASK_WORDS", cols=bad)
        refused("job_frame_b missing", job_frame_b=None)

        b, keep = _batch(og, frames, jobs, groups)
        r = og.FrameOverlapResult()
        assert lib.okvisgpu_frame_overlap(ctx.h, C.byref(b), C.byref(r)) == 0  # every output NULL
        assert lib.okvisgpu_frame_overlap(None, C.byref(b), C.byref(r)) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_frame_overlap(ctx.h, None, C.byref(r)) == ERR_INVALID_ARGUMENT
        assert lib.okvisgpu_frame_overlap(ctx.h, C.byref(b), None) == ERR_INVALID_ARGUMENT
        for field in ("n_frames", "n_jobs", "n_groups"):
            b2, keep2 = _batch(og, frames, jobs, groups)
            setattr(b2, field, -1)
            assert lib.okvisgpu_frame_overlap(ctx.h, C.byref(b2), C.byref(r)) == ERR_INVALID_ARGUMENT, field
        for field in ("image_begin", "rows", "kp_begin", "keypoint", "landmark", "job_kind", "job_frame_a",
                      "job_radius_factor", "group_begin"):
            b2, keep2 = _batch(og, frames, jobs, groups)
            setattr(b2, field, None)
            assert lib.okvisgpu_frame_overlap(ctx.h, C.byref(b2), C.byref(r)) == ERR_INVALID_ARGUMENT, field
            assert "missing" in lib.okvisgpu_last_error(ctx.h).decode(), field
        # valid edges: no jobs (groups are then empty), frames without images, images without keypoints
        got = _run(ctx, og, frames, [], [0, 0, 0], fill=FILL)
        assert got["group_best"].tolist() == [-1, -1] and got["group_max"].tolist() == [0.0, 0.0]
        bare = [[], [], [ov.image(480, 752, np.zeros((0, 2)), [])]]
        bare_jobs = [(0, 0, 1, 0.09), (2, 0, 0, 0.09), (3, 1, 0, 0.09), (2, 2, 0, 0.09), (3, 2, 0, 0.09)]
        _same(_run(ctx, og, bare, bare_jobs, fill=FILL), ov.reference(bare, bare_jobs))
        # the largest grid the budget takes: 8,192 words per mask
        wide = [[ov.image(640, 40960, [[20000.0, 300.0], [31.0, 5.0], [40955.0, 639.0]], [4, 0, 5])]]
        wide_jobs = [(2, 0, 0, 0.09), (0, 0, 0, 0.09)]
        _same(_run(ctx, og, wide, wide_jobs, fill=FILL), ov.reference(wide, wide_jobs))

        # between solve_begin and solve_end the call is refused, and the solve does not notice
        opts = og.default_options(max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0,
                                  parameter_tolerance=0.0)
        res = []
        for with_calls in (False, True):
            w = og.SynthWindow(10, 500, 4000, seed=78)
            ctx.set_problems([w.problem])
            if with_calls:
                _same(_run(ctx, og, frames, jobs, groups), ov.reference(frames, jobs, groups))
            ctx.solve_begin(opts)
            try:
                if with_calls:
                    refused("solve_end")
                    with pytest.raises(og.OkvisGpuError, match="solve_end"):
                        ctx.frame_overlap(b)
                ctx.solve_iterate(3)
            finally:
                s = ctx.solve_end()[0]
            res.append((s["final_cost"], s["num_iterations"], w.poses().copy()))
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1] == 3 and np.array_equal(res[0][2], res[1][2])
        _same(_run(ctx, og, frames, jobs, groups), ov.reference(frames, jobs, groups))
    finally:
        ctx.close()
