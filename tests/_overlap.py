"""The keypoint-coverage masks of the reference restated in numpy: the references of
tests/test_frame_overlap.py for okvisgpu_frame_overlap.

Four functions, each the reference's loop line for line: overlap_fraction (ViSlamBackend::overlapFraction,
ViSlamBackend.cpp:2903-2989), others_overlap and current_overlap (the two parts of
Frontend::doWeNeedANewKeyframe, Frontend.cpp:1245-1280 and :1202-1231) and tracking_quality
(ViSlamBackend::trackingQuality, ViSlamBackend.cpp:261-300, with the caller's "observed elsewhere" test as
the keypoint's flag). Masks are uint8 images, cv::circle is `circle`, a pixel-by-pixel transcription of
OpenCV's 8-connected integer Circle() for cv::FILLED with its `inside` fast path and its early-out tests,
landmark sets are Python sets, counts are np.count_nonzero. The device goes through half-width tables, bit
spans and a hash table, so the two routes share nothing but the contract.

A frame is a list of images; an image is a dict of rows, cols, kp [n, 2] float32 (cv::KeyPoint::pt), lm [n]
uint64 (landmarkId, 0 = none) and flag [n] uint8."""
import numpy as np

MASK_WORDS = 8192  # OKVISGPU_OVERLAP_MASK_WORDS
MAX_RADIUS = 1024  # OKVISGPU_OVERLAP_MAX_RADIUS
NAN_BITS = -0x8000000000000  # 0xFFF8000000000000 as int64: 0 / 0 on x86-64


# ------------------------------------------------------------------------------------- the disc
def circle(img, cx, cy, radius):
    """Circle(img, center, radius, color, fill = true) of OpenCV's drawing.cpp, colour 255."""
    height, width = img.shape
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    inside = radius <= cx < width - radius and radius <= cy < height - radius

    def hline(y, x1, x2):  # ICV_HLINE: x1 .. x2 inclusive
        for x in range(x1, x2 + 1):
            img[y, x] = 255

    while dx >= dy:
        y11, y12, y21, y22 = cy - dy, cy + dy, cy - dx, cy + dx
        x11, x12, x21, x22 = cx - dx, cx + dx, cx - dy, cx + dy
        if inside:
            hline(y11, x11, x12)
            hline(y12, x11, x12)
            hline(y21, x21, x22)
            hline(y22, x21, x22)
        elif x11 < width and x12 >= 0 and y21 < height and y22 >= 0:
            x11 = max(x11, 0)
            x12 = min(x12, width - 1)
            if 0 <= y11 < height:
                hline(y11, x11, x12)
            if 0 <= y12 < height:
                hline(y12, x11, x12)
            if x21 < width and x22 >= 0:
                x21 = max(x21, 0)
                x22 = min(x22, width - 1)
                if 0 <= y21 < height:
                    hline(y21, x21, x22)
                if 0 <= y22 < height:
                    hline(y22, x21, x22)
        dy += 1
        err += plus
        plus += 2
        mask = (1 if err <= 0 else 0) - 1
        err -= minus & mask
        dx += mask
        minus -= mask & 2


def half_widths(radius):
    """The table form of the contract: hw[|oy|] = the disc's half width in row oy."""
    hw = [0] * (radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, 2 * radius - 1
    while dx >= dy:
        hw[dy] = max(hw[dy], dx)
        hw[dx] = max(hw[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return hw


def table_disc(img, cx, cy, radius):
    """The disc from the table, cut to the image."""
    height, width = img.shape
    hw = half_widths(radius)
    for oy in range(-radius, radius + 1):
        y = cy + oy
        if 0 <= y < height:
            x0, x1 = max(cx - hw[abs(oy)], 0), min(cx + hw[abs(oy)], width - 1)
            if x0 <= x1:
                img[y, x0:x1 + 1] = 255


def centre(p):
    """cv::Point(keypoint.pt * 0.1) of one component: the Point2f product is formed in double and stored as
    float, the conversion is cvRound (ties to even). None where cvRound is undefined (the contract: such a
    keypoint paints nothing)."""
    f = np.float32(np.float64(np.float32(p)) * 0.1)
    if not np.isfinite(f) or abs(f) >= 2.0 ** 30:
        return None
    return int(np.rint(f))


def paint(img, pt, radius):
    """cv::circle(img, pt * 0.1, radius, 255, cv::FILLED)."""
    cx, cy = centre(pt[0]), centre(pt[1])
    if cx is None or cy is None:
        return
    circle(img, cx, cy, radius)


# ------------------------------------------------------------------------------------- frames
def image(rows, cols, kp, lm, flag=None):
    kp = np.ascontiguousarray(kp, dtype=np.float32).reshape(-1, 2)
    lm = np.ascontiguousarray(lm, dtype=np.uint64).reshape(-1)
    flag = np.zeros(len(lm), np.uint8) if flag is None else np.ascontiguousarray(flag, dtype=np.uint8).reshape(-1)
    assert len(kp) == len(lm) == len(flag)
    return {"rows": int(rows), "cols": int(cols), "kp": kp, "lm": lm, "flag": flag}


def _empty(im):
    return im["rows"] == 0 or im["cols"] == 0


def _grid(im, factor):
    rows, cols = im["rows"] // 10, im["cols"] // 10
    radius = float(min(rows, cols)) * float(factor)
    return rows, cols, radius


_DETECTIONS = {}


def _detections(im, factor):
    """The detections image of one camera image: every keypoint's disc. Kept per (image, factor): the
    reference repaints the same mask for every pair the frame takes part in."""
    key = (id(im), float(factor))
    if key not in _DETECTIONS:
        rows, cols, radius = _grid(im, factor)
        img = np.zeros((rows, cols), np.uint8)
        for k in range(len(im["kp"])):
            paint(img, im["kp"][k], int(radius))
        _DETECTIONS[key] = (im, img)  # (the image is held so that its id stays its own)
    return _DETECTIONS[key][1]


def _ratio(i, u):
    with np.errstate(all="ignore"):
        return np.float64(i) / np.float64(u)


def overlap_fraction(A, B, factor):
    """overlapFraction(frameA, frameB): (overlap, [I_A, U_A, I_B, U_B], [matched_A, matched_B])."""
    assert len(A) == len(B), "must be same number of frames"
    frames = (A, B)
    landmarks = (set(), set())
    for f in range(2):
        for im in frames[f]:
            if _empty(im):
                continue
            for k in range(len(im["kp"])):
                if im["lm"][k] != 0:
                    landmarks[f].add(int(im["lm"][k]))
    matches = landmarks[0] & landmarks[1]
    count, n_matched = [0, 0, 0, 0], [0, 0]
    overlap = [None, None]
    for f in range(2):
        for im in frames[f]:
            if _empty(im):
                continue
            rows, cols, radius = _grid(im, factor)
            det = _detections(im, factor)
            mat = np.zeros((rows, cols), np.uint8)
            for k in range(len(im["kp"])):
                if int(im["lm"][k]) in matches:
                    n_matched[f] += 1
                    paint(mat, im["kp"][k], int(radius))
            count[2 * f] += int(np.count_nonzero(mat & det))
            count[2 * f + 1] += int(np.count_nonzero(mat | det))
        overlap[f] = _ratio(count[2 * f], count[2 * f + 1])
    if len(matches) == 0:
        return np.float64(0.0), count, n_matched
    return (overlap[1] if overlap[1] < overlap[0] else overlap[0]), count, n_matched  # std::min


def others_overlap(A, B, factor):
    """One round of the "other frames" loop of doWeNeedANewKeyframe: B painted against the ids of A."""
    lm_ids = set()
    for im in A:
        for k in range(len(im["kp"])):
            if im["lm"][k] != 0:
                lm_ids.add(int(im["lm"][k]))
    count, n_matched = [0, 0, 0, 0], [0, 0]
    for im in B:
        rows, cols, radius = _grid(im, factor)
        det = _detections(im, factor)
        mat = np.zeros((rows, cols), np.uint8)
        for k in range(len(im["kp"])):
            lm = int(im["lm"][k])
            if lm != 0 and lm in lm_ids:
                n_matched[1] += 1
                paint(mat, im["kp"][k], int(radius))
        count[2] += int(np.count_nonzero(mat & det))
        count[3] += int(np.count_nonzero(mat | det))
    return _ratio(count[2], count[3]), count, n_matched


def current_overlap(A, factor):
    """The current-frame part of doWeNeedANewKeyframe."""
    count, n_matched = [0, 0, 0, 0], [0, 0]
    for im in A:
        rows, cols, radius = _grid(im, factor)
        det = _detections(im, factor)
        mat = np.zeros((rows, cols), np.uint8)
        for k in range(len(im["kp"])):
            if im["lm"][k] != 0:
                n_matched[0] += 1
                paint(mat, im["kp"][k], int(radius))
        count[0] += int(np.count_nonzero(mat & det))
        count[1] += int(np.count_nonzero(mat | det))
    return _ratio(count[0], count[1]), count, n_matched


def tracking_quality(A, factor):
    """trackingQuality with flag = "the landmark exists and is observed from another frame"."""
    intersection, union, matched_points = 0, 0, 0
    for im in A:
        rows, cols, radius = _grid(im, factor)
        mat = np.zeros((rows, cols), np.uint8)
        for k in range(len(im["kp"])):
            if im["flag"][k] != 0:
                matched_points += 1
                paint(mat, im["kp"][k], int(radius))
        point_area = int(radius * radius * np.pi)
        intersection += max(0, int(np.count_nonzero(mat)) - point_area)
        union += rows * cols - point_area
    overlap = np.float64(0.0) if matched_points < 8 else _ratio(intersection, union)
    return overlap, [intersection, union, 0, 0], [matched_points, 0]


# ------------------------------------------------------------------------------------- batches
def pack(frames):
    """The frame arrays of okvisgpu_frame_overlap_batch: dict of image_begin, rows, cols, kp_begin, keypoint,
    landmark, flag."""
    images = [im for fr in frames for im in fr]
    two = lambda a, cols, dt: np.concatenate(a).astype(dt) if a else np.zeros((0,) + cols, dt)
    return {"image_begin": np.cumsum([0] + [len(fr) for fr in frames]).astype(np.int32),
            "rows": np.array([im["rows"] for im in images], np.int32),
            "cols": np.array([im["cols"] for im in images], np.int32),
            "kp_begin": np.cumsum([0] + [len(im["kp"]) for im in images]).astype(np.int32),
            "keypoint": two([im["kp"] for im in images], (2,), np.float32),
            "landmark": two([im["lm"] for im in images], (), np.uint64),
            "flag": two([im["flag"] for im in images], (), np.uint8)}


def reference(frames, jobs, group_begin=None):
    """The outputs of okvisgpu_frame_overlap for jobs = [(kind, frame_a, frame_b, factor)]."""
    n = len(jobs)
    out = {"overlap": np.zeros(n), "count": np.zeros((n, 4), np.int32), "n_matched": np.zeros((n, 2), np.int32),
           "n_keypoints": np.zeros(n, np.int32)}
    for j, (kind, a, b, factor) in enumerate(jobs):
        A = frames[a]
        if kind == 0:
            r = overlap_fraction(A, frames[b], factor)
        elif kind == 1:
            r = others_overlap(A, frames[b], factor)
        elif kind == 2:
            r = current_overlap(A, factor)
        else:
            r = tracking_quality(A, factor)
        out["overlap"][j], out["count"][j], out["n_matched"][j] = r
        out["n_keypoints"][j] = sum(len(im["kp"]) for im in A)
    if group_begin is not None:
        ng = len(group_begin) - 1
        out["group_best"] = np.full(ng, -1, np.int32)
        out["group_max"] = np.zeros(ng)
        for g in range(ng):
            overlap, m = 0.0, np.float64(0.0)
            for j in range(group_begin[g], group_begin[g + 1]):
                v = out["overlap"][j]
                if v >= overlap:  # mostOverlappedStateId (:2800)
                    out["group_best"][g] = j
                    overlap = v
                m = v if m < v else m  # std::max (:1279)
            out["group_max"][g] = m
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
