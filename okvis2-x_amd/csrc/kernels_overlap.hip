// kernels_overlap.hip — the keypoint-coverage masks of ViSlamBackend::overlapFraction
// (ViSlamBackend.cpp:2903-2989), ViSlamBackend::trackingQuality (:261-300) and
// Frontend::doWeNeedANewKeyframe (Frontend.cpp:1186-1295) for a batch of jobs on gfx950
// (okvisgpu_frame_overlap; the contract is the header's).
//
//  k_overlap_init    zeroes the id tables, the per-job counts and the error word.
//  k_overlap_insert  one lane per keypoint: its non-zero landmark id into its frame's open-addressed
//                    table (a slot is claimed by a 64-bit CAS on the id itself, empty = 0); a slot is
//                    `live` once a keypoint of a non-empty image holds it. Membership does not depend on
//                    the insertion order.
//  k_overlap_paint   one workgroup per (job, side, image): both masks in LDS as G_r x ceil(G_c / 32)
//                    words; lanes stride over the image's keypoints, decide "matched" (a probe of the
//                    other frame's table, the id, or the flag) and OR the clipped span of every disc row
//                    into the masks. After the barrier popcount(m & d) and popcount(m | d), summed per
//                    wavefront, one integer add per wavefront and count.
//  k_overlap_finish  one lane per job forms the double. k_overlap_groups: one lane per group folds its
//                    jobs in order.
//
// Only integer ORs and adds cross lanes, so a job's counts do not depend on arrival order or on the
// batch; the one floating-point operation per job is a division of two of its counts.
#include "launch.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

namespace {

using u64 = unsigned long long;
constexpr int kOverlapWG = 256;

// Fibonacci hashing: consecutive ids (the reference's landmark counter) and ids with a common stride
// both spread over the table
__device__ __forceinline__ uint32_t idSlot(u64 id, uint32_t mask) {
  return (uint32_t)((id * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// id (non-zero) among the ids of the frame whose table is [t0, t0 + size); needLive: held by a keypoint of
// a non-empty image
__device__ __forceinline__ bool idInFrame(const OverlapDev& V, int t0, int size, u64 id, bool needLive) {
  const uint32_t mask = (uint32_t)size - 1u;
  uint32_t s = idSlot(id, mask);
  for (int probe = 0; probe < size; ++probe, s = (s + 1u) & mask) {
    const u64 key = gmem(V.table)[t0 + (int)s];
    if (key == id) return !needLive || gmem(V.live)[t0 + (int)s] != 0;
    if (key == 0) return false;
  }
  return false;
}

__device__ __forceinline__ int waveSum(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
  return v;  // lane 0's
}

// cvRound(float(double(pt) * 0.1)); false where cvRound is undefined or the disc cannot reach a grid
__device__ __forceinline__ bool centreOf(float pt, int& c) {
  const float f = (float)((double)pt * 0.1);
  if (!(fabsf(f) < 1073741824.0f)) return false;  // NaN, infinities, beyond 2^30
  c = __float2int_rn(f);
  return true;
}

}  // namespace

__global__ __launch_bounds__(kOverlapWG) void k_overlap_init(const OverlapDev V) {
  const int t = (int)(blockIdx.x * kOverlapWG + threadIdx.x);
  if (t < V.table_total) {
    gmemw(V.table)[t] = 0;
    gmemw(V.live)[t] = 0;
  }
  if (t < 4 * V.n_jobs) gmemw(V.count)[t] = 0;
  if (t < 2 * V.n_jobs) gmemw(V.n_matched)[t] = 0;
  if (t == 0) gmemw(V.err)[0] = 0;
}

__global__ __launch_bounds__(kOverlapWG) void k_overlap_insert(const OverlapDev V) {
  const int k = (int)(blockIdx.x * kOverlapWG + threadIdx.x);
  if (k >= V.n_kp) return;
  const u64 id = gmem(V.lm)[k];
  if (id == 0) return;
  const int im = gmem(V.kp_image)[k], f = gmem(V.img_frame)[im];
  const int t0 = gmem(V.tab_begin)[f], size = gmem(V.tab_begin)[f + 1] - t0;
  const uint32_t mask = (uint32_t)size - 1u;
  uint32_t s = idSlot(id, mask);
  for (int probe = 0; probe < size; ++probe, s = (s + 1u) & mask) {
    const u64 old = atomicCAS(&V.table[t0 + (int)s], 0ull, id);
    if (old == 0 || old == id) {
      if (gmem(V.img_live)[im]) gmemw(V.live)[t0 + (int)s] = 1;  // (every writer stores the same byte)
      return;
    }
  }
  atomicOr(V.err, 1);  // more ids than slots: cannot happen with two slots per keypoint
}

__global__ __launch_bounds__(kOverlapWG) void k_overlap_paint(const OverlapDev V) {
  extern __shared__ uint32_t sMask[];  // matches [nw], detections [nw]; kind 3: matches [nw], its total
  const OverlapItem it = V.items[blockIdx.x];
  const int t = (int)threadIdx.x;
  const int Gr = gmem(V.img_gr)[it.image], Gc = gmem(V.img_gc)[it.image];
  const int W = (Gc + 31) >> 5, nw = Gr * W;
  uint32_t* sm = sMask;
  uint32_t* sd = sMask + nw;
  const bool both = it.kind != 3;
  for (int e = t; e < (both ? 2 * nw : nw + 1); e += kOverlapWG) sMask[e] = 0;
  __syncthreads();

  int t0 = 0, size = 1;
  if (it.other >= 0) {
    t0 = gmem(V.tab_begin)[it.other];
    size = gmem(V.tab_begin)[it.other + 1] - t0;
  }
  const auto hw = gmem(V.hw + it.hw_off);
  const int R = it.R;
  const int k0 = gmem(V.kp_begin)[it.image], k1 = gmem(V.kp_begin)[it.image + 1];
  int nMatched = 0;
  for (int k = k0 + t; k < k1; k += kOverlapWG) {
    bool matched;
    if (it.kind == 3) {
      matched = gmem(V.flag)[k] != 0;
    } else {
      const u64 id = gmem(V.lm)[k];
      matched = id != 0 && (it.kind == 2 || idInFrame(V, t0, size, id, it.kind == 0));
    }
    nMatched += matched;
    if (!both && !matched) continue;
    int cx, cy;
    const auto p = gmem(V.kp + 2 * (size_t)k);
    if (!centreOf(p[0], cx) || !centreOf(p[1], cy)) continue;
    const int y0 = cy - R > 0 ? cy - R : 0, y1 = cy + R < Gr - 1 ? cy + R : Gr - 1;
    for (int y = y0; y <= y1; ++y) {
      const int oy = y - cy, h = hw[oy < 0 ? -oy : oy];
      const int x0 = cx - h > 0 ? cx - h : 0, x1 = cx + h < Gc - 1 ? cx + h : Gc - 1;
      if (x0 > x1) continue;
      const int w0 = x0 >> 5, w1 = x1 >> 5;
      for (int w = w0; w <= w1; ++w) {
        const int lo = w == w0 ? (x0 & 31) : 0, hi = w == w1 ? (x1 & 31) : 31;
        const uint32_t bits = (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
        if (both) atomicOr(&sd[y * W + w], bits);
        if (matched) atomicOr(&sm[y * W + w], bits);
      }
    }
  }
  __syncthreads();

  int nI = 0, nU = 0;
  for (int e = t; e < nw; e += kOverlapWG) {
    const uint32_t m = sm[e], d = both ? sd[e] : 0u;
    nI += __popc(both ? (m & d) : m);
    nU += __popc(m | d);
  }
  nI = waveSum(nI);
  nU = waveSum(nU);
  nMatched = waveSum(nMatched);
  const bool lead = (t & 63) == 0;
  int32_t* cnt = V.count + 4 * (size_t)it.job + (both ? 2 * it.side : 0);
  if (lead && nMatched) atomicAdd(&V.n_matched[2 * (size_t)it.job + (both ? it.side : 0)], nMatched);
  if (both) {
    if (lead && nI) atomicAdd(&cnt[0], nI);
    if (lead && nU) atomicAdd(&cnt[1], nU);
    return;
  }
  // kind 3: the clamp needs the image's total
  if (lead && nI) atomicAdd(reinterpret_cast<int*>(&sMask[nw]), nI);
  __syncthreads();
  if (t == 0) {
    const int painted = (int)sMask[nw] - it.area;
    atomicAdd(&cnt[0], painted > 0 ? painted : 0);
    atomicAdd(&cnt[1], Gr * Gc - it.area);
  }
}

__global__ __launch_bounds__(kOverlapWG) void k_overlap_finish(const OverlapDev V) {
  const int j = (int)(blockIdx.x * kOverlapWG + threadIdx.x);
  if (j >= V.n_jobs) return;
  const int kind = gmem(V.job_kind)[j];
  const int32_t* c = V.count + 4 * (size_t)j;
  const int32_t* nm = V.n_matched + 2 * (size_t)j;
  // x86-64's 0 / 0, whatever this device's division gives
  auto ratio = [](int a, int b) {
    return (a == 0 && b == 0) ? __longlong_as_double((long long)0xFFF8000000000000ull) : __ddiv_rn((double)a, (double)b);
  };
  double v;
  if (kind == 0) {
    if (nm[0] == 0) {
      v = 0.0;  // no common id (:2949)
    } else {
      const double oa = ratio(c[0], c[1]), ob = ratio(c[2], c[3]);
      v = (ob < oa) ? ob : oa;
    }
  } else if (kind == 1) {
    v = ratio(c[2], c[3]);
  } else if (kind == 2) {
    v = ratio(c[0], c[1]);
  } else {
    v = nm[0] < 8 ? 0.0 : ratio(c[0], c[1]);
  }
  gmemw(V.overlap)[j] = v;
}

__global__ __launch_bounds__(64) void k_overlap_groups(const OverlapDev V) {
  const int g = (int)(blockIdx.x * 64 + threadIdx.x);
  if (g >= V.n_groups) return;
  int best = -1;
  double run = 0.0, m = 0.0;
  for (int j = gmem(V.group_begin)[g]; j < gmem(V.group_begin)[g + 1]; ++j) {
    const double v = V.overlap[j];
    if (v >= run) {
      best = j;
      run = v;
    }
    m = (m < v) ? v : m;
  }
  gmemw(V.group_best)[g] = best;
  gmemw(V.group_max)[g] = m;
}

void launch_frame_overlap(const OverlapDev& V, hipStream_t s) {
  if (V.n_jobs <= 0) return;
  const int n0 = V.table_total > 4 * V.n_jobs ? V.table_total : 4 * V.n_jobs;
  k_overlap_init<<<(n0 + kOverlapWG - 1) / kOverlapWG, kOverlapWG, 0, s>>>(V);
  if (V.n_kp > 0) k_overlap_insert<<<(V.n_kp + kOverlapWG - 1) / kOverlapWG, kOverlapWG, 0, s>>>(V);
  if (V.n_items > 0)
    k_overlap_paint<<<V.n_items, kOverlapWG, sizeof(uint32_t) * 2 * (size_t)V.max_words, s>>>(V);
  k_overlap_finish<<<(V.n_jobs + kOverlapWG - 1) / kOverlapWG, kOverlapWG, 0, s>>>(V);
  if (V.n_groups > 0) k_overlap_groups<<<(V.n_groups + 63) / 64, 64, 0, s>>>(V);
}

}  // namespace okg
