// kernels_covis.hip — co-observation counts: ViGraph::computeCovisibilities
// (okvis_ceres/src/ViGraph.cpp:727-785) for every window of the batch.
//
// counts[i][j] = the landmarks with an observation in state i and one in state j. The planner's visit
// CSR (lm_visit_begin, visit_pose) already holds each landmark's distinct poses, so the visibility
// matrix B [landmark][state] is 0/1 and counts = B^T B. Its columns are kept as bit-vectors over the
// window's landmarks: counts[i][j] = popcount(v_i & v_j), n_observed[i] = popcount(v_i).
//   k_covis_bits          one wavefront per 64 consecutive landmarks of one window: v, one word per state
//   k_covis_counts_lds    the pair popcounts by one workgroup holding the window's bitset in LDS (path 0)
//   k_covis_counts_tiled  the same by state-tile pairs streaming word chunks (path 1); covisFitsLds picks
// All integers, no global atomics (bits are ORed in LDS, where the order does not matter), every output
// element written by exactly one lane: the result does not depend on the schedule and the two paths
// give the same numbers.
#include <hip/hip_runtime.h>

#include "device_problem.hpp"
#include "launch.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

namespace {
using u64 = unsigned long long;
constexpr int kBitsStates = 512;  // states per pass of k_covis_bits: one LDS word each
constexpr int kBitsAhead = 4;     // visits a lane loads before it uses them
}  // namespace

// One wavefront (a workgroup of its own) per word. Lane l walks the visits of landmark 64 * word + l
// and ORs bit l into the LDS word of each visit's state; the wavefront then stores the words,
// bits[state][word]. A window of more than kBitsStates states takes several passes over the state
// ranges; visits are sorted by pose, so a lane's walk resumes where the pass before stopped. A lane
// loads kBitsAhead visits at a time: they do not depend on each other, and the loop is as long as the
// longest run of visits, not as the state count. Integer OR does not depend on order. Excluded
// landmarks, the tail lanes of the last word and landmarks without observations have an empty walk
// and set no bit; every word of the window's states is written.
__global__ __launch_bounds__(64) void k_covis_bits(const DevProblem* __restrict__ Pp,
                                                   const CovisWin* __restrict__ wins, int n_wins,
                                                   const int32_t* __restrict__ word_rec, int n_words_total,
                                                   const uint8_t* __restrict__ excluded, u64* __restrict__ bits) {
  __shared__ u64 sw[kBitsStates];
  const DevProblem& P = *Pp;
  const int lane = (int)threadIdx.x;
  const int g = (int)blockIdx.x;
  if (g >= n_words_total) return;
  const int rec = gmem(word_rec)[g];
  if (rec < 0 || rec >= n_wins) return;  // (never with the tables the runtime builds)
  const CovisWin W = wins[rec];
  const int word = g - W.word_begin;
  if (word < 0 || word >= W.n_words) return;  // (never with the table the runtime builds)
  int v = 0, ve = 0;
  {
    const int k = word * 64 + lane, l = W.lm_begin + k;
    if (k < W.n_lm && l >= 0 && l < P.n_lm && !(excluded && gmem(excluded)[l])) {
      v = min(max(gmem(P.lm_visit_begin)[l], 0), P.n_visit);
      ve = min(max(gmem(P.lm_visit_begin)[l + 1], v), P.n_visit);
    }
  }
  const u64 bit = 1ull << lane;
  for (int c0 = 0; c0 < W.n_state; c0 += kBitsStates) {  // (uniform: one record per workgroup)
    const int cn = min(kBitsStates, W.n_state - c0), lim = c0 + cn;
    for (int k = lane; k < cn; k += 64) sw[k] = 0;
    __syncthreads();
    while (v < ve) {
      int p[kBitsAhead];
      for (int u = 0; u < kBitsAhead; ++u) p[u] = gmem(P.visit_pose)[min(v + u, ve - 1)] - W.pose_begin;
      int used = 0;
      for (int u = 0; u < kBitsAhead; ++u)
        if (used == u && v + u < ve && p[u] < lim) {  // a state of this pass, or one before it (never: sorted): passed over
          if (p[u] >= c0) atomicOr(&sw[p[u] - c0], bit);
          used = u + 1;
        }
      v += used;
      if (used < kBitsAhead) break;  // the run ended, or its next visit is a later pass's
    }
    __syncthreads();
    for (int k = lane; k < cn; k += 64) gmemw(bits)[W.bits_off + (int64_t)(c0 + k) * W.n_words + word] = sw[k];
    __syncthreads();
  }
}

// One pair (i >= j): to [i][j] and [j][i]; the diagonal's popcount is n_observed, its count 0.
__device__ __forceinline__ void covisStore(const CovisWin& W, int i, int j, int c, int32_t* counts, int32_t* n_observed) {
  auto out = gmemw(counts + W.counts_off);
  if (i == j) {
    gmemw(n_observed)[W.state_off + i] = c;
    out[(int64_t)i * W.n_state + i] = 0;
  } else {
    out[(int64_t)i * W.n_state + j] = c;
    out[(int64_t)j * W.n_state + i] = c;
  }
}

// Path 0: one workgroup per window, its whole bitset in LDS (rows at the odd stride covisRowStride:
// a half-wave's rows j, j + 1, ... lie on distinct banks, row i is a broadcast). Lanes take the pairs
// i >= j in triangular order.
__global__ __launch_bounds__(256) void k_covis_counts_lds(const CovisWin* __restrict__ wins,
                                                          const int32_t* __restrict__ items, unsigned lds_bytes,
                                                          const u64* __restrict__ bits, int32_t* counts,
                                                          int32_t* n_observed) {
  extern __shared__ __align__(16) u64 sbits[];
  const CovisWin W = wins[gmem(items)[blockIdx.x]];
  const int S = W.n_state, nw = W.n_words, ld = covisRowStride(nw);
  if (S <= 0 || nw <= 0 || covisLdsBytes(S, nw) > lds_bytes) return;  // (never: the launcher sized the LDS for its items)
  const auto src = gmem(bits + W.bits_off);
  for (int k = (int)threadIdx.x; k < S * nw; k += (int)blockDim.x) {
    const int s = k / nw;
    sbits[s * ld + (k - s * nw)] = src[k];
  }
  __syncthreads();
  const int npair = S * (S + 1) / 2;  // S <= kCovisLdsBudget / 8
  for (int p = (int)threadIdx.x; p < npair; p += (int)blockDim.x) {
    int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > p) --i;
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    const int j = p - i * (i + 1) / 2;
    const u64 *a = sbits + i * ld, *b = sbits + j * ld;
    int c = 0;
    for (int w = 0; w < nw; ++w) c += __popcll(a[w] & b[w]);
    covisStore(W, i, j, c, counts, n_observed);
  }
}

// Path 1: one workgroup per (row tile ti, column tile tj <= ti) of kCovisTile states; the words of
// the two row sets pass through LDS in chunks of kCovisChunk (zero beyond the window's states and
// words). Thread t holds the pair (t / 32, t % 32) of the tile and moves word t % 32 of row t / 32 of
// both row sets, loading the next chunk into registers while the tile is counted on the current one.
// Row i of a half-wave is a broadcast, its 32 rows j lie on distinct banks (stride 33).
__global__ __launch_bounds__(kCovisTile * kCovisTile) void k_covis_counts_tiled(const CovisWin* __restrict__ wins,
                                                                                const int32_t* __restrict__ items,
                                                                                const u64* __restrict__ bits,
                                                                                int32_t* counts, int32_t* n_observed) {
  constexpr int T = kCovisTile, CH = kCovisChunk, LD = CH + 1;
  static_assert(T == 32 && CH == 32, "the thread mapping below is for 32 x 32 tiles of 32-word chunks");
  __shared__ u64 sa[T * LD], sb[T * LD];
  const auto it = gmem(items + 3 * (size_t)blockIdx.x);
  const CovisWin W = wins[it[0]];
  const int ti = it[1], tj = it[2];
  const int S = W.n_state, nw = W.n_words;
  const int tid = (int)threadIdx.x, lj = tid & 31, li = tid >> 5;
  const int gi = ti * T + li, gj = tj * T + lj;
  const int ra = gi, rb = tj * T + li;  // the rows this thread moves
  const auto src = gmem(bits + W.bits_off);
  auto load = [&](int c0, u64& a, u64& b) {
    const int w = c0 + lj;
    a = (ra < S && w < nw) ? src[(int64_t)ra * nw + w] : 0ull;
    b = (rb < S && w < nw) ? src[(int64_t)rb * nw + w] : 0ull;
  };
  const bool live = gi >= gj && gi < S && gj < S;  // below the diagonal only inside a diagonal tile
  int acc = 0;
  u64 na, nb;
  load(0, na, nb);
  for (int c0 = 0; c0 < nw; c0 += CH) {
    sa[li * LD + lj] = na;
    sb[li * LD + lj] = nb;
    __syncthreads();
    if (c0 + CH < nw) load(c0 + CH, na, nb);
    if (live) {
#pragma unroll 8
      for (int w = 0; w < CH; ++w) acc += __popcll(sa[li * LD + w] & sb[lj * LD + w]);
    }
    __syncthreads();
  }
  if (live) covisStore(W, gi, gj, acc, counts, n_observed);
}

void launch_covis_bits(const DevProblem& P, const CovisWin* wins, int n_wins, const int32_t* word_rec, int n_words_total,
                       const uint8_t* excluded, unsigned long long* bits, hipStream_t s) {
  if (n_wins > 0 && n_words_total > 0)
    hipLaunchKernelGGL(k_covis_bits, dim3(n_words_total), dim3(64), 0, s, P.self, wins, n_wins, word_rec, n_words_total,
                       excluded, bits);
}

void launch_covis_counts(const CovisWin* wins, const int32_t* items0, int n0, size_t lds_bytes, const int32_t* items1,
                         int n1, const unsigned long long* bits, int32_t* counts, int32_t* n_observed, hipStream_t s) {
  if (n0 > 0)
    hipLaunchKernelGGL(k_covis_counts_lds, dim3(n0), dim3(256), lds_bytes, s, wins, items0, (unsigned)lds_bytes, bits,
                       counts, n_observed);
  if (n1 > 0)
    hipLaunchKernelGGL(k_covis_counts_tiled, dim3(n1), dim3(kCovisTile * kCovisTile), 0, s, wins, items1, bits, counts,
                       n_observed);
}

}  // namespace okg
