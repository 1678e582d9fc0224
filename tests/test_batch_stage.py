"""The staging of the entry points that bring arrays up and down per call (csrc/batch_stage.hpp: the call-scoped
batches of csrc/batch_calls.cpp and the calls on the resident batch of csrc/resident_calls.cpp, with the host
loops of csrc/window_export.hpp).

CPU: BatchLayout alone, and the export loops alone, each in a stand-alone program built with the address and
undefined-behaviour sanitizers; plain heap blocks stand for the pinned stage and the device buffer and two memcpy
for the two copies.
GPU: the entry points share one pinned stage and one device buffer per context, so they are called interleaved
on one context (small, large, small: a regrow, then a reuse of a larger buffer holding another call's bytes) and
every result must be the bytes the same call gives alone on a fresh context."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from _paths import REPO

CSRC = os.path.join(REPO, "okvis2-x_amd", "csrc")

LAYOUT_PROGRAM = r"""
#include "batch_stage.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

using okg::BatchLayout;

static int failures = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("line %d: %s\n", __LINE__, #x);                  \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// the fields a kernel's descriptor would hold
struct Dev {
  const double* in_a;
  const uint32_t* in_desc;    // staged from bytes: 12 words per 48-byte row
  const int32_t* in_filled;   // no source: filled through host()
  const uint8_t* in_empty;    // zero count
  const uint8_t* in_absent;   // optional and absent: never declared
  double* io_pose;
  int32_t* io_kept;           // read back, not delivered (null destination)
  int32_t* out_i;
  uint8_t* out_b;
  double* out_skipped;        // null destination
  int32_t* out_empty;         // zero count
  double* scr_a;
  uint8_t* scr_b;
};

// a destination with guard bytes on both sides
struct Guarded {
  std::vector<unsigned char> mem;
  size_t n;
  explicit Guarded(size_t bytes) : mem(bytes + 128, 0xA5), n(bytes) {}
  unsigned char* data() { return mem.data() + 64; }
  bool guardsIntact() const {
    for (size_t i = 0; i < 64; ++i)
      if (mem[i] != 0xA5 || mem[64 + n + i] != 0xA5) return false;
    return true;
  }
};

static unsigned char pat(int slot, size_t i) { return (unsigned char)(17 * slot + 3 * i + 1); }

int main() {
  const size_t NA = 37, ND = 5, NF = 9, NP = 3, NK = 6, NI = 41, NB = 300, NS = 7, SA = 11, SB = 513;
  std::vector<double> a(NA);
  for (size_t i = 0; i < NA; ++i) a[i] = 0.5 * (double)i - 3.0;
  std::vector<uint8_t> desc(48 * ND);
  for (size_t i = 0; i < desc.size(); ++i) desc[i] = (uint8_t)(i * 7 + 1);
  std::vector<double> pose(7 * NP);
  for (size_t i = 0; i < pose.size(); ++i) pose[i] = 1.0 / (double)(i + 1);
  std::vector<int32_t> kept(NK);
  for (size_t i = 0; i < NK; ++i) kept[i] = (int32_t)(100 + i);
  const std::vector<double> a0 = a, pose0 = pose;
  const std::vector<uint8_t> desc0 = desc;
  const std::vector<int32_t> kept0 = kept;
  Guarded dPose(56 * NP), dI(4 * NI), dB(NB);

  Dev D{};
  BatchLayout S;
  // declared in shuffled kind order
  S.scratch(D.scr_a, SA);
  const auto oI = S.out(D.out_i, dI.data(), NI);
  const auto iA = S.in(D.in_a, a.data(), NA);
  const auto ioP = S.inout(D.io_pose, pose.data(), dPose.data(), 7 * NP);
  const auto oSkip = S.out(D.out_skipped, nullptr, NS);
  const auto iF = S.in(D.in_filled, nullptr, NF);
  S.in(D.in_empty, nullptr, 0);
  S.scratch(D.scr_b, SB);
  const auto oE = S.out(D.out_empty, nullptr, 0);
  const auto ioK = S.inout(D.io_kept, kept.data(), nullptr, NK);
  const auto oB = S.out(D.out_b, dB.data(), NB);
  const auto iD = S.in(D.in_desc, desc.data(), 12 * ND);
  (void)oE;
  S.commit();

  // one contiguous upload range from 0 and one contiguous download range, which overlap in the inouts
  const size_t up = S.upEnd(), db = S.downBegin(), de = S.downEnd(), size = S.size();
  CHECK(db % 256 == 0);
  CHECK(0 < db && db < up && up < de && de < size);

  // the host block holds exactly [0, downEnd), the device block exactly [0, size): an access past either is
  // the sanitizer's to report
  char* host = static_cast<char*>(std::aligned_alloc(256, (de + 255) / 256 * 256));
  char* dev = static_cast<char*>(std::aligned_alloc(256, (size + 255) / 256 * 256));
  std::memset(host, 0xDD, de);
  std::memset(dev, 0xEE, size);
  S.begin(host, dev);
  CHECK(S.hostBase() == host && S.devBase() == dev);
  for (size_t i = 0; i < NF; ++i) S.host(iF)[i] = (int32_t)(7 * i);

  struct Field { const void* p; size_t bytes; int kind; };  // kind: 0 in, 1 inout, 2 out, 3 scratch
  const Field f[] = {{D.in_a, 8 * NA, 0},     {D.in_desc, 48 * ND, 0}, {D.in_filled, 4 * NF, 0}, {D.in_empty, 0, 0},
                     {D.io_pose, 56 * NP, 1}, {D.io_kept, 4 * NK, 1},  {D.out_i, 4 * NI, 2},     {D.out_b, NB, 2},
                     {D.out_skipped, 8 * NS, 2}, {D.out_empty, 0, 2},  {D.scr_a, 8 * SA, 3},     {D.scr_b, SB, 3}};
  const size_t nf = sizeof(f) / sizeof(f[0]);
  for (size_t i = 0; i < nf; ++i) {
    CHECK(f[i].p != nullptr);
    const size_t off = (size_t)(static_cast<const char*>(f[i].p) - dev), end = off + f[i].bytes;
    CHECK(off % 256 == 0);
    const size_t lo = f[i].kind == 0 ? 0 : f[i].kind == 3 ? de : db;
    const size_t hi = f[i].kind <= 1 ? up : f[i].kind == 2 ? de : size;
    CHECK(lo <= off && end <= hi);
    if (f[i].kind == 0) CHECK(end <= db);  // an input is not read back
    if (f[i].kind == 2) CHECK(off >= up);  // an output is not uploaded
    for (size_t j = 0; j < i; ++j) {       // distinct and disjoint, empty arrays included
      const size_t oj = (size_t)(static_cast<const char*>(f[j].p) - dev);
      CHECK(off != oj);
      CHECK(end <= oj || oj + f[j].bytes <= off);
    }
  }
  CHECK(D.in_absent == nullptr);
  // typed host access names the same offsets
  CHECK((char*)S.host(iA) - host == (const char*)D.in_a - dev);
  CHECK((char*)S.host(oB) - host == (const char*)D.out_b - dev);

  // the copy up: [0, upEnd) and nothing else
  std::memcpy(dev, host, up);
  CHECK(std::memcmp(D.in_a, a0.data(), 8 * NA) == 0);
  CHECK(std::memcmp(D.in_desc, desc0.data(), 48 * ND) == 0);
  CHECK(std::memcmp(D.io_pose, pose0.data(), 56 * NP) == 0);
  CHECK(std::memcmp(D.io_kept, kept0.data(), 4 * NK) == 0);
  for (size_t i = 0; i < NF; ++i) CHECK(D.in_filled[i] == (int32_t)(7 * i));
  for (size_t i = up; i < size; ++i)
    if ((unsigned char)dev[i] != 0xEE) {
      CHECK(!"a byte past upEnd was uploaded");
      break;
    }

  // the "kernel": every byte of every inout, out and scratch array
  unsigned char* w[] = {(unsigned char*)D.io_pose, (unsigned char*)D.io_kept, (unsigned char*)D.out_i,
                        (unsigned char*)D.out_b,   (unsigned char*)D.out_skipped, (unsigned char*)D.scr_a,
                        (unsigned char*)D.scr_b};
  const size_t wb[] = {56 * NP, 4 * NK, 4 * NI, NB, 8 * NS, 8 * SA, SB};
  for (int k = 0; k < 7; ++k)
    for (size_t i = 0; i < wb[k]; ++i) w[k][i] = pat(k, i);

  // the copy down: [downBegin, downEnd) and nothing else; then the delivery
  std::memcpy(host + db, dev + db, de - db);
  S.deliver();
  auto holds = [](const unsigned char* p, int k, size_t n) {
    for (size_t i = 0; i < n; ++i)
      if (p[i] != pat(k, i)) return false;
    return true;
  };
  CHECK(holds(dPose.data(), 0, 56 * NP) && dPose.guardsIntact());
  CHECK(holds(dI.data(), 2, 4 * NI) && dI.guardsIntact());
  CHECK(holds(dB.data(), 3, NB) && dB.guardsIntact());
  // null destinations: read through host(), delivered nowhere
  CHECK(holds((const unsigned char*)S.host(ioK), 1, 4 * NK));
  CHECK(holds((const unsigned char*)S.host(oSkip), 4, 8 * NS));
  CHECK(holds((const unsigned char*)S.host(ioP), 0, 56 * NP));
  CHECK(holds((const unsigned char*)S.host(oI), 2, 4 * NI));
  // the sources are the caller's: an inout with another destination leaves its source alone
  CHECK(a == a0 && desc == desc0 && pose == pose0 && kept == kept0);
  // the staged inputs below downBegin were not overwritten by the copy down
  CHECK(std::memcmp(S.host(iA), a0.data(), 8 * NA) == 0);
  CHECK(std::memcmp(S.host(iD), desc0.data(), 48 * ND) == 0);
  std::free(host);
  std::free(dev);

  {  // inputs only: nothing to read back; outputs only: nothing to upload
    Dev E{};
    BatchLayout I, O;
    I.in(E.in_a, a.data(), NA);
    I.scratch(E.scr_a, SA);
    I.commit();
    CHECK(I.downBegin() == I.downEnd() && I.downEnd() == I.upEnd() && I.upEnd() >= 8 * NA && I.size() > I.upEnd());
    O.out(E.out_i, nullptr, NI);
    O.commit();
    CHECK(O.upEnd() == 0 && O.downBegin() == 0 && O.downEnd() == O.size() && O.size() >= 4 * NI);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
"""


def test_batch_layout_under_sanitizers(tmp_path):
    """Slots declared in shuffled kind order give one contiguous upload range and one contiguous download
    range; every patched field is 256-aligned and inside the range of its kind; empty arrays are distinct and
    non-null; an inout lies in both ranges; null destinations and undeclared optionals are left alone; a write
    to every device output byte arrives at its destination and only there."""
    _run_under_sanitizers(tmp_path, "layout", LAYOUT_PROGRAM)


EXPORT_PROGRAM = r"""
#include "window_export.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      std::printf("line %d: %s\n", __LINE__, #x);                  \
      ++failures;                                                  \
    }                                                              \
  } while (0)

// n doubles holding `fill`, with guard doubles on both sides
struct Guarded {
  std::vector<double> mem;
  size_t n;
  Guarded(size_t count, double fill) : mem(count + 16, -12345.0), n(count) {
    for (size_t i = 0; i < n; ++i) mem[8 + i] = fill;
  }
  double* data() { return mem.data() + 8; }
  double operator[](size_t i) const { return mem[8 + i]; }
  bool guardsIntact() const {
    for (size_t i = 0; i < 8; ++i)
      if (mem[i] != -12345.0 || mem[8 + n + i] != -12345.0) return false;
    return true;
  }
};

int main() {
  const int fdim = 7, fpad = 8, dn = 5;
  const int32_t nat[fpad] = {3, -1, 0, 4, -1, 1, 2, 0};  // rows 1 and 4 are gap rows; [7] is padding, not read
  const double poison = std::nan(""), untouched = 777.0;

  {  // vector scatter: every natural element written from its row, nothing else
    double v[fpad];
    for (int r = 0; r < fdim; ++r) v[r] = 10.0 * r + 1.0;
    v[7] = poison;
    Guarded out(dn, untouched);
    okg::scatterNatural(v, nat, fdim, out.data());
    for (int r = 0; r < fdim; ++r)
      if (nat[r] >= 0) CHECK(out[nat[r]] == 10.0 * r + 1.0);
    CHECK(out.guardsIntact());
    // the first five rows only: natural elements 1 and 2 (rows 5 and 6) stay as they were
    Guarded part(dn, untouched);
    okg::scatterNatural(v, nat, 5, part.data());
    CHECK(part[3] == 1.0 && part[0] == 21.0 && part[4] == 31.0);
    CHECK(part[1] == untouched && part[2] == untouched && part.guardsIntact());
  }

  {  // symmetric scatter: the lower triangle of rows 0..6 is the only part of M that is read
    std::vector<double> M((size_t)fpad * fpad, poison);
    for (int r = 0; r < fdim; ++r)
      for (int q = 0; q <= r; ++q) M[(size_t)r * fpad + q] = 100.0 * r + q + 1.0;
    Guarded out((size_t)dn * dn, untouched);
    okg::scatterNaturalSym(M.data(), nat, fdim, fpad, dn, out.data());
    CHECK(out.guardsIntact());
    for (int r = 0; r < fdim; ++r)
      for (int q = 0; q <= r; ++q) {
        if (nat[r] < 0 || nat[q] < 0) continue;
        CHECK(out[(size_t)nat[r] * dn + nat[q]] == 100.0 * r + q + 1.0);
        CHECK(out[(size_t)nat[q] * dn + nat[r]] == 100.0 * r + q + 1.0);
      }
    for (int a = 0; a < dn; ++a)
      for (int b = 0; b < dn; ++b) {
        const double x = out[(size_t)a * dn + b];
        CHECK(x == x && x != untouched);            // filled, and from no poisoned element
        CHECK(x == out[(size_t)b * dn + a]);        // symmetric
        const int r = (int)(x - 1.0) / 100, q = (int)(x - 1.0) % 100;
        CHECK(r != 1 && r != 4 && q != 1 && q != 4);  // no gap row or column arrived
      }
  }

  {  // record split
    const size_t n = 3;
    const int K = 11, R = 4;
    std::vector<double> rec(n * K);
    for (size_t f = 0; f < n; ++f)
      for (int i = 0; i < K; ++i) rec[f * K + i] = 1000.0 * f + i;
    auto rOk = [&](const Guarded& r) {
      for (size_t f = 0; f < n; ++f)
        for (int i = 0; i < R; ++i)
          if (r[f * R + i] != 1000.0 * f + i) return false;
      return r.guardsIntact();
    };
    auto jOk = [&](const Guarded& J) {
      for (size_t f = 0; f < n; ++f)
        for (int i = R; i < K; ++i)
          if (J[f * (K - R) + (i - R)] != 1000.0 * f + i) return false;
      return J.guardsIntact();
    };
    auto allAre = [](const Guarded& g, double x) {
      for (size_t i = 0; i < g.n; ++i)
        if (g[i] != x) return false;
      return g.guardsIntact();
    };
    Guarded r(n * R, untouched), J(n * (K - R), untouched);
    okg::splitRecords(rec.data(), n, K, R, r.data(), J.data());
    CHECK(rOk(r) && jOk(J));
    Guarded r1(n * R, untouched), J1(n * (K - R), untouched);
    okg::splitRecords(rec.data(), n, K, R, nullptr, J1.data());
    CHECK(jOk(J1));
    okg::splitRecords(rec.data(), n, K, R, r1.data(), nullptr);
    CHECK(rOk(r1));
    // no records: a null source is not read and the outputs stay as they were
    Guarded r0(n * R, untouched), J0(n * (K - R), untouched);
    okg::splitRecords(nullptr, 0, K, R, r0.data(), J0.data());
    okg::splitRecords(nullptr, 0, K, R, nullptr, nullptr);
    CHECK(allAre(r0, untouched) && allAre(J0, untouched));
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
"""


def _run_under_sanitizers(tmp_path, name, program):
    if not shutil.which("g++"):
        pytest.skip("g++ unavailable")
    src = tmp_path / (name + ".cpp")
    src.write_text(program)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, str(src), "-o",
                    str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_window_export_under_sanitizers(tmp_path):
    """The host loops of csrc/window_export.hpp alone (no HIP): the natural-order scatter of a vector and of a
    symmetric matrix over an order with two gap rows and a padded stride (values, untouched elements, guard
    bytes, symmetry, nothing read from the upper triangle or the padding), and the record split with either
    output null and with no records."""
    _run_under_sanitizers(tmp_path, "window_export", EXPORT_PROGRAM)


# ------------------------------------------------------------------------------------------ GPU
def _flat(out):
    """The arrays of a call's result, as bytes."""
    if isinstance(out, dict):
        return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}
    return {str(i): np.ascontiguousarray(v).tobytes() for i, v in enumerate(out) if v is not None}


def _calls(og, oracle):
    """name -> ctx -> result: the smallest scenes of the entry points' own tests."""
    import _twopose as tp
    import test_imu_propagate as tip
    import test_match_frames as tmf
    import test_match_to_map as tmm
    import test_place as tpl

    hand = tpl.MATCH_SCENES["hand"]()
    s6 = tmm.SCENES["s6"]()
    capped = tpl.REFINE_SCENES["capped"]()
    ip = tip._params(og)
    crafted = tip._pack(tip._crafted(ip)[0])
    edge, cams, ex = tp.scene(oracle, 101, n_lm=55, outliers=2, mono_far=1, mono_near=0)  # a mixed scene
    frames = tmf.SCENES["hand"]()
    return {
        "place_match": lambda ctx: ctx.place_match(tpl._match_batch(og, hand)[0], fill={k: 77 for k in tpl.pl.MATCH_KEYS}),
        "match_to_map": lambda ctx: tmm._run(og, ctx, s6),
        "place_refine": lambda ctx: tpl._run_refine(og, ctx, capped),
        "imu_propagate": lambda ctx: tip._run(ctx, ip, crafted),
        "twopose_compute": lambda ctx: ctx.twopose_compute(og.TwoPoseBatch([edge], cams, ex)),
        "match_frames": lambda ctx: tmf._run(og, ctx, frames),
    }


@pytest.mark.gpu
def test_gpu_interleaved_calls_share_one_buffer(og, oracle):
    """place_match, match_to_map, place_refine, imu_propagate, twopose_compute, match_frames and place_match
    again on one context: each result is, byte for byte, what the same call gives alone on a fresh context.
    (The fresh contexts are made one after the other: two contexts exist at any time.)"""
    if og.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    calls = _calls(og, oracle)
    order = ["place_match", "match_to_map", "place_refine", "imu_propagate", "twopose_compute", "match_frames",
             "place_match"]
    shared = og.Context(0)
    try:
        for name in order:
            got = _flat(calls[name](shared))
            fresh = og.Context(0)
            try:
                alone = _flat(calls[name](fresh))
            finally:
                fresh.close()
            assert got.keys() == alone.keys() and len(got) > 0, name
            for k in got:
                assert got[k] == alone[k], (name, k)
    finally:
        shared.close()


# ---- the calls on the resident batch (csrc/resident_calls.cpp) use the same two buffers
COVIS_KEYS = ("counts", "n_observed", "visible", "n_pairs", "n_visible", "any", "path")
LANDMARK_KEYS = ("quality", "initialised", "reset", "n_initialised", "n_reset", "in_front")
PARAMS = ("poses", "speed_biases", "landmarks", "imu_state")  # what a call may write of the caller's arrays


def _by_window(results, keys):
    return {f"{w}.{k}": np.ascontiguousarray(r[k]).tobytes() for w, r in enumerate(results) for k in keys}


def _params(qs):
    return {f"{w}.{k}": getattr(q, k).tobytes() for w, q in enumerate(qs) for k in PARAMS}


def _resident_windows(og):
    """Three small windows, so that every base offset of the last one is non-zero: the crafted covisibility
    window below one 64-landmark word, the smallest window on the tiled count path, the 10-keyframe window."""
    import test_covisibilities as tcv
    return [tcv._crafted(og), tcv._window(og, "tiled"), tcv._window(og, "s10")]


def _update_landmarks_without_errors(og, ctx, qs):
    """okvisgpu_update_landmarks with obs_error NULL in every window (the Python wrapper always asks for it)."""
    import ctypes as C
    ups = (og.LandmarkUpdate * len(qs))()
    out = []
    for u, q in zip(ups, qs):
        d = {"quality": np.zeros(len(q.landmarks)), "initialised": np.zeros(len(q.landmarks), dtype=np.uint8),
             "reset": np.zeros(len(q.landmarks), dtype=np.uint8)}
        u.quality = og.dptr(d["quality"])
        u.initialised = d["initialised"].ctypes.data_as(C.POINTER(C.c_uint8))
        u.reset = d["reset"].ctypes.data_as(C.POINTER(C.c_uint8))
        out.append(d)
    assert og.lib().okvisgpu_update_landmarks(ctx.h, ups) == 0
    for u, d in zip(ups, out):
        d["n_initialised"], d["n_reset"], d["in_front"] = int(u.n_initialised), int(u.n_reset), int(u.in_front)
    return out


def _resident_steps(og, oracle):
    """(name, (ctx, qs) -> the call's result as bytes), in the order they run on the shared context."""
    batch = _calls(og, oracle)

    def covis(ctx, qs, masks=None):
        res = ctx.covisibilities(masks, n_windows=3)
        assert [r["path"] for r in res] == [0, 1, 0]
        return _by_window(res, COVIS_KEYS)

    def masks(qs):  # (no mask for the middle window: its part of the staged mask is zero-filled)
        return [(np.arange(len(qs[0].landmarks)) % 3 == 0).astype(np.uint8), None,
                (np.arange(len(qs[2].landmarks)) % 5 == 1).astype(np.uint8)]

    def named(prefix, arrays):
        return {f"{prefix}.{i}": np.ascontiguousarray(a).tobytes() for i, a in enumerate(arrays)}

    return [
        ("covisibilities", covis),
        ("place_match", lambda ctx, qs: _flat(batch["place_match"](ctx))),
        ("update_landmarks(obs_error)",
         lambda ctx, qs: {**_by_window(ctx.update_landmarks(n_windows=3), LANDMARK_KEYS + ("obs_error",)), **_params(qs)}),
        ("eval_imu", lambda ctx, qs: {**named("imu", ctx.eval_imu(qs[2].struct.n_imu, window=2)), **_params(qs)}),
        ("covisibilities(masks)", lambda ctx, qs: covis(ctx, qs, masks(qs))),
        ("linearize_reduce", lambda ctx, qs: named("lin", ctx.linearize_reduce(window=2))),
        ("match_frames", lambda ctx, qs: _flat(batch["match_frames"](ctx))),
        ("update_landmarks",
         lambda ctx, qs: {**_by_window(_update_landmarks_without_errors(og, ctx, qs), LANDMARK_KEYS), **_params(qs)}),
        ("eval_relpose+eval_reprojection",
         lambda ctx, qs: {**named("relpose", ctx.eval_relpose(qs[2].struct.n_relpose, window=2)),
                          **named("reprojection", ctx.eval_reprojection(qs[2].struct.n_observations, window=2))}),
        ("gauss_newton_step", lambda ctx, qs: named("gn", ctx.gauss_newton_step(window=2))),
    ]


@pytest.mark.gpu
def test_gpu_resident_calls_share_the_buffers_of_the_batch_calls(og, oracle):
    """One context holds three windows; covisibilities, update_landmarks (with and without obs_error), eval_imu,
    linearize_reduce, eval_relpose, eval_reprojection and gauss_newton_step of the last window run on it
    interleaved with place_match and match_frames, which use the same pinned stage and device buffer. Each result
    (with the parameter arrays a call may write) is, byte for byte, what the same call gives on a fresh context
    holding the same three problems. Every call starts from the same parameter values on both sides: the shared
    context's arrays are restored and uploaded again, the fresh context gets fresh copies."""
    if og.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    from _problem import OwnedProblem
    base = _resident_windows(og)
    assert [q.struct.n_landmarks > 0 and q.struct.n_imu > 0 for q in base] == [True] * 3
    snaps = [q.snapshot() for q in base]
    qs = [OwnedProblem.copy_of(q.struct) for q in base]
    shared = og.Context(0)
    try:
        shared.set_problems([q.struct for q in qs])
        for name, call in _resident_steps(og, oracle):
            for q, s in zip(qs, snaps):
                q.restore(s)
            shared.update_params()
            got = call(shared, qs)
            fresh = og.Context(0)
            try:
                ps = [OwnedProblem.copy_of(q.struct) for q in base]
                fresh.set_problems([p.struct for p in ps])
                alone = call(fresh, ps)
            finally:
                fresh.close()
            assert got.keys() == alone.keys() and len(got) > 0, name
            for k in got:
                assert got[k] == alone[k], (name, k)
    finally:
        shared.close()
