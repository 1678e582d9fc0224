// kernels_lidar.hip — the LiDAR pre-processing of ThreadedSlam::processFrame (ThreadedSlam.cpp:785-818)
// for a batch on gfx950: LidarMotionUndistortion::deskew (LidarMotionUndistortion.cpp:27-85) with the
// BatchedLidarPropagator behind it (ViInterface.cpp:635-798), and VoxelDownSample
// (VoxelGridFilter.hpp:46-67).
//
//  k_lidar_chain    one lane per scan (64 per wavefront), as k_imu_propagate_lane: the committed chain
//                   of the propagator, one step per IMU interval from t_start on. Only Delta_q,
//                   acc_integral and acc_doubleintegral are carried (the bias Jacobians are multiplied
//                   by Delta_b = 0 in the reference); the state before every interval goes to one
//                   10-double row of the table.
//  k_lidar_points   one lane per query (LiDAR point): binary search for the interval k of the query's
//                   stamp, row k of the table, one interpolated step (:674-715), getState (:762-798)
//                   and the transform into the live sensor frame. Lanes of a wavefront have
//                   neighbouring stamps, so the row and the two samples are mostly the same addresses;
//                   each is loaded once per lane.
//  k_voxel_init / k_voxel_insert / k_voxel_keep
//                   one open-addressed table over (cloud, voxel) for the whole batch: claim a slot by
//                   CAS, integer min of the point index per slot, keep[i] = the slot's minimum is i.
//                   Integer min and CAS make the mask independent of arrival order; no thread waits for
//                   another's progress.
//
// A scan's and a cloud's result does not depend on the batch: no lane reads another item's data and
// no floating-point value is combined across lanes.
#include <climits>

#include "imu_chain.hpp"
#include "launch.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

namespace {

// step(k, tau, T) for ts[k] < T <= ts[k+1] and tau < T (ViInterface.cpp:660-715): cur / nxt are the
// samples k and k + 1, tau the end of the committed chain. The interpolation rules are the
// propagator's own (:674-691, not stepSample's); the step is the lane step of imu_chain.hpp on its carried
// state Delta_q_, acc_integral_, acc_doubleintegral_. Returns omega_S_true in w.
__device__ __forceinline__ void lidarStep(const RawSample& cur, const RawSample& nxt, int64_t tau, int64_t T,
                                          const double* bg, const double* ba, LaneChain& S, double* w) {
  double om0[3], ac0[3], om1[3], ac1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    om0[j] = cur.ga[j];
    ac0[j] = cur.ga[3 + j];
    om1[j] = nxt.ga[j];
    ac1[j] = nxt.ga[3 + j];
  }
  double dt;
  if (T < nxt.t) {  // inside the interval: interpolate the second measurement (:674-681), dt from tau
    dt = durToSec(T - tau);
    const double r = dt / durToSec(nxt.t - cur.t);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      om1[j] = (1.0 - r) * om0[j] + r * om1[j];
      ac1[j] = (1.0 - r) * ac0[j] + r * ac1[j];
    }
  } else {
    dt = durToSec(nxt.t - tau);
  }
  {  // the first step of a call starts at tau (:686-691); exact (r = 1) when tau is the sample's stamp
    const double r = dt / durToSec(T - cur.t);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      om0[j] = r * om0[j] + (1.0 - r) * om1[j];
      ac0[j] = r * ac0[j] + (1.0 - r) * ac1[j];
    }
  }
  PropStep s;
  s.dt = dt;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    s.w[j] = 0.5 * (om0[j] + om1[j]) - bg[j];
    s.a[j] = 0.5 * (ac0[j] + ac1[j]) - ba[j];
    w[j] = s.w[j];
  }
  double C[9];  // R(Delta_q) before the step: a table row holds Dq only
  qrot(S.Dq, C);
  Q& Dq = S.Dq;
  double* const ai = S.ai;
  double* const adi = S.adi;
#include "imu_chain_lane_body.hpp"
}

__device__ __forceinline__ void storeRow(double* table, size_t row, const LaneChain& S) {
  const auto o = gmemw(table + (size_t)kLidarRow * row);
  o[0] = S.Dq.x; o[1] = S.Dq.y; o[2] = S.Dq.z; o[3] = S.Dq.w;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o[4 + j] = S.ai[j];
    o[7 + j] = S.adi[j];
  }
}

// x -> C x + r for a pose [r, q xyzw] with q normalised as Transformation::set does
__device__ __forceinline__ void loadPose(const double* p, double* r, double* Cm) {
  const auto g = gmem(p);
  r[0] = g[0]; r[1] = g[1]; r[2] = g[2];
  qrot(qnormalize(Q{g[3], g[4], g[5], g[6]}), Cm);
}

}  // namespace

// ---- the committed chain: one lane per scan
__global__ __launch_bounds__(64) void k_lidar_chain(const LidarDeskewDev L) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= L.n_scans) return;
  const int sbeg = gmem(L.sbegin)[i], N = gmem(L.sbegin)[i + 1] - sbeg;
  if (N <= 0 || gmem(L.qbegin)[i + 1] == gmem(L.qbegin)[i]) return;  // no query reads a row of this scan
  const auto sbp = gmem(L.sb0 + 9 * (size_t)i);
  const double bg[3] = {sbp[3], sbp[4], sbp[5]}, ba[3] = {sbp[6], sbp[7], sbp[8]};
  LaneChain S{Q{0.0, 0.0, 0.0, 1.0}, {0, 0, 0}, {0, 0, 0}};
  int64_t tau = gmem(L.t_start)[i];
  RawSample cur = loadRawSample(L.ts, L.ga, sbeg, N, 0), nxt = loadRawSample(L.ts, L.ga, sbeg, N, 1);
  for (int k = 0; k < N; ++k) {
    const RawSample ahead = loadRawSample(L.ts, L.ga, sbeg, N, k + 2);
    storeRow(L.table, (size_t)sbeg + k, S);  // the state before interval k
    if (k + 1 < N && nxt.t > tau) {          // else skipped (:683-685)
      double w[3];
      lidarStep(cur, nxt, tau, nxt.t, bg, ba, S, w);
      tau = nxt.t;
    }
    cur = nxt;
    nxt = ahead;
  }
}

// ---- one lane per query
constexpr int kLidarPointsWG = 256;

__global__ __launch_bounds__(kLidarPointsWG) void k_lidar_points(const LidarDeskewDev L) {
  const int q = (int)(blockIdx.x * kLidarPointsWG + threadIdx.x);
  if (q >= L.n_query) return;
  const int i = gmem(L.q_scan)[q];
  const int64_t T = gmem(L.qt)[q], t0 = gmem(L.t_start)[i];
  const int sbeg = gmem(L.sbegin)[i], N = gmem(L.sbegin)[i + 1] - sbeg;  // N >= 2: the host has checked
  const auto tsp = gmem(L.ts + sbeg);
  const auto p0 = gmem(L.pose0 + 7 * (size_t)i);
  const auto sbp = gmem(L.sb0 + 9 * (size_t)i);

  // before t_start: skipped by deskew (:61); past the last sample: appendTo returns false (:653)
  const bool valid = T >= t0 && T <= tsp[N - 1];
  double pose[7] = {0, 0, 0, 0, 0, 0, 0}, v[3] = {0, 0, 0}, w[3] = {0, 0, 0};
  if (valid && T == t0) {  // the state itself (:52-57): the input bits
#pragma unroll
    for (int j = 0; j < 7; ++j) pose[j] = p0[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = sbp[j];
  } else if (valid) {
    // k = the largest index with ts[k] < T: ts[0] <= t_start < T <= ts[N - 1]
    int lo = 0, hi = N - 1;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (tsp[mid] < T) lo = mid; else hi = mid;
    }
    const int k = lo;  // <= N - 2
    const RawSample cur = loadRawSample(L.ts, L.ga, sbeg, N, k), nxt = loadRawSample(L.ts, L.ga, sbeg, N, k + 1);
    const auto row = gmem(L.table + (size_t)kLidarRow * ((size_t)sbeg + k));
    LaneChain S{Q{row[0], row[1], row[2], row[3]}, {row[4], row[5], row[6]}, {row[7], row[8], row[9]}};
    const double bg[3] = {sbp[3], sbp[4], sbp[5]}, ba[3] = {sbp[6], sbp[7], sbp[8]};
    lidarStep(cur, nxt, cur.t > t0 ? cur.t : t0, T, bg, ba, S, w);
    // getState (:762-798) with Delta_b = 0
    const double Dt = durToSec(T - t0);
    const double gW[3] = {0.0, 0.0, L.g};
    const Q q0 = qnormalize(Q{p0[3], p0[4], p0[5], p0[6]});
    double C0[9], Cadi[3], Cai[3];
    qrot(q0, C0);
    mv3(C0, S.adi, Cadi);
    mv3(C0, S.ai, Cai);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      pose[j] = (p0[j] + sbp[j] * Dt - 0.5 * gW[j] * Dt * Dt) + Cadi[j];
      v[j] = (sbp[j] - gW[j] * Dt) + Cai[j];
    }
    const Q q1 = qnormalize(qmul(q0, S.Dq));
    pose[3] = q1.x; pose[4] = q1.y; pose[5] = q1.z; pose[6] = q1.w;
  }

  if (L.valid) gmemw(L.valid)[q] = valid ? 1 : 0;
  if (L.pose) {
    const auto o = gmemw(L.pose + 7 * (size_t)q);
#pragma unroll
    for (int j = 0; j < 7; ++j) o[j] = pose[j];
  }
  if (L.speed) {
    const auto o = gmemw(L.speed + 3 * (size_t)q);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
  if (L.omega) {
    const auto o = gmemw(L.omega + 3 * (size_t)q);
    o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
  }
  if (L.point || L.point_f64) {
    double p[3] = {0, 0, 0};
    if (valid) {  // T_live^-1 T_WS(T) T_SL [ray; 1] (:79-81)
      const auto rp = gmem(L.ray + 3 * (size_t)q);
      const double ray[3] = {rp[0], rp[1], rp[2]};
      double r[3], Cm[9], pS[3], pW[3];
      loadPose(L.T_SL + 7 * (size_t)i, r, Cm);
      mv3(Cm, ray, pS);
#pragma unroll
      for (int j = 0; j < 3; ++j) pS[j] += r[j];
      qrot(qnormalize(Q{pose[3], pose[4], pose[5], pose[6]}), Cm);
      mv3(Cm, pS, pW);
#pragma unroll
      for (int j = 0; j < 3; ++j) pW[j] += pose[j];
      loadPose(L.pose_live + 7 * (size_t)i, r, Cm);
#pragma unroll
      for (int j = 0; j < 3; ++j) pW[j] -= r[j];
      mtv3(Cm, pW, p);
    }
    if (L.point_f64) {
      const auto o = gmemw(L.point_f64 + 3 * (size_t)q);
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    }
    if (L.point) {
      const auto o = gmemw(L.point + 3 * (size_t)q);
      o[0] = (float)p[0]; o[1] = (float)p[1]; o[2] = (float)p[2];
    }
  }
}

void launch_lidar_chain(const LidarDeskewDev& L, hipStream_t s) {
  if (L.n_scans <= 0 || L.n_query <= 0) return;
  k_lidar_chain<<<(L.n_scans + 63) / 64, 64, 0, s>>>(L);
}
void launch_lidar_points(const LidarDeskewDev& L, hipStream_t s) {
  if (L.n_query <= 0) return;
  k_lidar_points<<<(L.n_query + kLidarPointsWG - 1) / kLidarPointsWG, kLidarPointsWG, 0, s>>>(L);
}

// ------------------------------------------------------------------ voxel downsampling
namespace {

constexpr int kVoxelWG = 256;

// The voxel of point i (VoxelGridFilter.hpp:54): per component the single-precision quotient
// p / float(voxel_size), correctly rounded, truncated toward zero. False for a non-finite component or
// a quotient outside int32 (undefined behaviour in the reference): such a point is never kept.
__device__ __forceinline__ bool voxelOf(const VoxelDev& V, int i, int& c, int* vx) {
  c = gmem(V.pt_cloud)[i];
  const float vs = gmem(V.vsize)[c];
  const auto p = gmem(V.point + 3 * (size_t)i);
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float qf = __fdiv_rn(p[j], vs);
    const bool in = qf >= -2147483648.0f && qf < 2147483648.0f;  // false for NaN
    ok = ok && in;
    vx[j] = in ? (int)qf : 0;
  }
  return ok;
}

__device__ __forceinline__ uint32_t voxelHash(int c, const int* vx) {
  uint32_t h = (uint32_t)c * 0x9E3779B1u;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    h ^= (uint32_t)vx[j];
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
  }
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}

}  // namespace

__global__ __launch_bounds__(kVoxelWG) void k_voxel_init(const VoxelDev V) {
  const int t = (int)(blockIdx.x * kVoxelWG + threadIdx.x);
  if (t < V.table_size) {
    gmemw(V.table)[t] = -1;
    gmemw(V.best)[t] = INT_MAX;
  }
  if (t < V.n_clouds) gmemw(V.n_kept)[t] = 0;
  if (t == 0) gmemw(V.err)[0] = 0;
}

__global__ __launch_bounds__(kVoxelWG) void k_voxel_insert(const VoxelDev V) {
  const int i = (int)(blockIdx.x * kVoxelWG + threadIdx.x);
  if (i >= V.n_points) return;
  int c, vx[3], found = -1;
  const bool used = (!V.use || gmem(V.use)[i]) && voxelOf(V, i, c, vx);
  if (used) {
    const uint32_t mask = (uint32_t)V.table_size - 1u;
    uint32_t s = voxelHash(c, vx) & mask;
    for (int probe = 0; probe < V.table_size; ++probe, s = (s + 1u) & mask) {
      int occ = atomicCAS(&V.table[s], -1, i);
      if (occ == -1) occ = i;  // claimed
      bool same = occ == i;
      if (!same) {  // the occupant's key, from the read-only input
        int oc, ov[3];
        voxelOf(V, occ, oc, ov);
        same = oc == c && ov[0] == vx[0] && ov[1] == vx[1] && ov[2] == vx[2];
      }
      if (same) {
        atomicMin(&V.best[s], i);
        found = (int)s;
        break;
      }
    }
    if (found < 0) atomicOr(V.err, 1);  // more keys than slots: cannot happen with table_size >= 2 n_points
  }
  gmemw(V.slot)[i] = found;
}

// 1,024 points per workgroup: the kept points of the workgroup's first cloud are counted in LDS and
// reach n_kept as one add, so that a large cloud does not send one add per wavefront to one address
constexpr int kVoxelKeepWG = 1024;

__global__ __launch_bounds__(kVoxelKeepWG) void k_voxel_keep(const VoxelDev V) {
  __shared__ int sCount, sCloud;
  const int i = (int)(blockIdx.x * kVoxelKeepWG + threadIdx.x);
  const bool in = i < V.n_points;
  if (threadIdx.x == 0) {  // (the first point of a launched workgroup exists)
    sCount = 0;
    sCloud = gmem(V.pt_cloud)[i];
  }
  __syncthreads();
  int c = -1;
  bool kept = false;
  if (in) {
    c = gmem(V.pt_cloud)[i];
    const int s = V.slot[i];
    kept = s >= 0 && V.best[s] == i;
    gmemw(V.keep)[i] = kept ? 1 : 0;
  }
  // n_kept: one integer add per (wavefront, cloud), into LDS for the workgroup's first cloud
  const int lane = (int)(threadIdx.x & 63);
  bool pending = in;
  while (true) {
    const unsigned long long act = __ballot(pending);
    if (!act) break;
    const int leader = __ffsll((long long)act) - 1;
    const int cl = __shfl(c, leader, 64);
    const bool mine = pending && c == cl;
    const unsigned long long m = __ballot(mine && kept);
    if (lane == leader && m) {
      if (cl == sCloud) atomicAdd(&sCount, __popcll(m));
      else atomicAdd(&V.n_kept[cl], __popcll(m));
    }
    if (mine) pending = false;
  }
  __syncthreads();
  if (threadIdx.x == 0 && sCount) atomicAdd(&V.n_kept[sCloud], sCount);
}

void launch_voxel_downsample(const VoxelDev& V, hipStream_t s) {
  if (V.n_points <= 0) return;
  const int n0 = V.table_size > V.n_clouds ? V.table_size : V.n_clouds;
  const int np = (V.n_points + kVoxelWG - 1) / kVoxelWG;
  k_voxel_init<<<(n0 + kVoxelWG - 1) / kVoxelWG, kVoxelWG, 0, s>>>(V);
  k_voxel_insert<<<np, kVoxelWG, 0, s>>>(V);
  k_voxel_keep<<<(V.n_points + kVoxelKeepWG - 1) / kVoxelKeepWG, kVoxelKeepWG, 0, s>>>(V);
}

}  // namespace okg
