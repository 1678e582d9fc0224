// kernels_imu_propagate.hip — ImuError::propagation (ImuError.cpp:537-759) for a batch of
// independent items on gfx950 (FP64): pose and speed of the next state from the previous estimate and
// the IMU samples between two stamps, with the optional 15x15 Jacobian and covariance.
//
//  k_imu_propagate_lane     one lane per item (64 per wavefront): the call without covariance and
//                           Jacobian (ViGraph::addStatesPropagate, ThreadedSlam::processFrame). Only
//                           Delta_q, acc_integral and acc_doubleintegral are carried; nothing of the
//                           bias Jacobians or the covariance is computed.
//  k_imu_propagate_group<COV>  one 16-lane group per item (four per wavefront), the layout of
//                           k_eval_imu: every lane of the group runs the scalar chain (:644-668), so
//                           the block-sparse F_delta (:672-682) is register resident; lane l < 15 owns
//                           column l of P_delta and P <- F P F^T + Q takes one LDS transpose per step.
//                           COV = false does no covariance work (Jacobian only).
//
// An item's arithmetic does not depend on the batch or on its position in it: loops run to the
// wavefront's longest item with the shorter ones predicated off, and no lane reads another item's
// data. An item whose samples do not reach t_end gets steps = -1 and nothing else is written
// (:552-553); an item with no integrated step keeps its pose and speed/bias bits (Jacobian = I,
// covariance = 0).
#include "imu_chain.hpp"
#include "launch.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

namespace {

struct PropItem {  // one item's record, loaded once
  int64_t t_start, t_end;
  int sbeg, N;
  bool covered;
};

__device__ __forceinline__ PropItem loadItem(const ImuPropagateDev& A, int i) {
  PropItem it;
  it.t_start = gmem(A.t_start)[i];
  it.t_end = gmem(A.t_end)[i];
  it.sbeg = gmem(A.sbegin)[i];
  it.N = gmem(A.sbegin)[i + 1] - it.sbeg;
  // imuMeasurements.back().timeStamp >= end (:552); the host has refused N == 0
  it.covered = it.N > 0 && gmem(A.ts)[it.sbeg + max(it.N - 1, 0)] >= it.t_end;
  return it;
}

// The outputs that need no Jacobian (:726-732), written by one lane: r_1, q_1 = normalize(q_0 Dq)
// (Transformation::set normalises) and v_1.
__device__ __forceinline__ void writeState(const ImuPropagateDev& A, int i, const Q& q0, const double* C0,
                                           const double* v0, const Q& Dq, const double* ai, const double* adi,
                                           double Dt) {
  const auto pose = gmemw(A.poses + 7 * (size_t)i);
  const auto sb = gmemw(A.sb + 9 * (size_t)i);
  const double gW[3] = {0.0, 0.0, A.par[6]};
  double Cadi[3], Cai[3];
  mv3(C0, adi, Cadi);
  mv3(C0, ai, Cai);
  double r1[3], v1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    r1[j] = pose[j] + v0[j] * Dt + Cadi[j] - 0.5 * gW[j] * Dt * Dt;
    v1[j] = v0[j] + (Cai[j] - gW[j] * Dt);
  }
  const Q q1 = qnormalize(qmul(q0, Dq));
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    pose[j] = r1[j];
    sb[j] = v1[j];
  }
  pose[3] = q1.x; pose[4] = q1.y; pose[5] = q1.z; pose[6] = q1.w;
}

}  // namespace

// ---- one lane per item: pose and speed only
__global__ __launch_bounds__(64) void k_imu_propagate_lane(const ImuPropagateDev A) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= A.n) return;
  const PropItem it = loadItem(A, i);
  if (!it.covered) {
    gmemw(A.steps)[i] = -1;
    return;
  }
  const auto sbp = gmem(A.sb + 9 * (size_t)i);
  const double v0[3] = {sbp[0], sbp[1], sbp[2]}, bg[3] = {sbp[3], sbp[4], sbp[5]}, ba[3] = {sbp[6], sbp[7], sbp[8]};
  Q Dq{0.0, 0.0, 0.0, 1.0};
  double C[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // R(Delta_q), carried (= qrot(Dq) of the previous step)
  double ai[3] = {0, 0, 0}, adi[3] = {0, 0, 0}, Dt = 0.0;
  int64_t time = it.t_start;
  int steps = 0;
  RawSample cur = loadRawSample(A.ts, A.ga, it.sbeg, it.N, 0), nxt = loadRawSample(A.ts, A.ga, it.sbeg, it.N, 1);
  for (int k = 0; k < it.N; ++k) {
    const RawSample ahead = loadRawSample(A.ts, A.ga, it.sbeg, it.N, k + 2);
    PropStep s;
    const bool ok = stepSample(A.par[0], A.par[1], it.N, it.t_end, k, cur, nxt, time, steps > 0, bg, ba, s);
    cur = nxt;
    nxt = ahead;
    if (!ok) continue;
    Dt += s.dt;
#include "imu_chain_lane_body.hpp"
    time = s.nexttime;
    ++steps;
    if (s.nexttime == it.t_end) break;
  }
  gmemw(A.steps)[i] = steps;
  if (steps == 0) return;
  const auto pose = gmem(A.poses + 7 * (size_t)i);
  const Q q0 = qnormalize(Q{pose[3], pose[4], pose[5], pose[6]});
  double C0[9];
  qrot(q0, C0);
  writeState(A, i, q0, C0, v0, Dq, ai, adi, Dt);
}

// ---- one 16-lane group per item: Jacobian, and with COV the covariance
constexpr int kPropGroup = 16;

template <bool COV>
__global__ __launch_bounds__(64) void k_imu_propagate_group(const ImuPropagateDev A) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int i = (int)blockIdx.x * kGroupsPerWave + g;
  __shared__ double sAll[kGroupsPerWave][15 * kColStride];  // per group: the P exchange, then the Jacobian
  double* const M = sAll[g];

  const bool inR = i < A.n;
  const int ic = inR ? i : 0;
  const PropItem it = loadItem(A, ic);
  const bool live = inR && it.covered;
  const auto sbp = gmem(A.sb + 9 * (size_t)ic);
  const double v0[3] = {sbp[0], sbp[1], sbp[2]}, bg[3] = {sbp[3], sbp[4], sbp[5]}, ba[3] = {sbp[6], sbp[7], sbp[8]};

  // the chain (:556-578), on every lane of the group
  Q Dq{0.0, 0.0, 0.0, 1.0};
  double C[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double Ci[9], Cdi[9], cross[9], dadbg[9], dvdbg[9], dpdbg[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) Ci[e] = Cdi[e] = cross[e] = dadbg[e] = dvdbg[e] = dpdbg[e] = 0.0;
  double ai[3] = {0, 0, 0}, adi[3] = {0, 0, 0}, Dt = 0.0;
  double Pc[15];  // column l of P_delta
#pragma unroll
  for (int e = 0; e < 15; ++e) Pc[e] = 0.0;

  int64_t time = it.t_start;
  int steps = 0;
  bool done = !live;
  // uniform trip count over the wavefront (the barriers of the P exchange); shorter items idle
  int Nmax = live ? it.N : 0;
  Nmax = max(Nmax, __shfl_xor(Nmax, 16, 64));
  Nmax = max(Nmax, __shfl_xor(Nmax, 32, 64));
  RawSample cur = loadRawSample(A.ts, A.ga, it.sbeg, it.N, 0), nxt = loadRawSample(A.ts, A.ga, it.sbeg, it.N, 1);
  for (int k = 0; k < Nmax; ++k) {
    const RawSample ahead = loadRawSample(A.ts, A.ga, it.sbeg, it.N, k + 2);
    PropStep s;
    const bool doStep =
        !done && k < it.N && stepSample(A.par[0], A.par[1], it.N, it.t_end, k, cur, nxt, time, steps > 0, bg, ba, s);  // uniform over the group
    cur = nxt;
    nxt = ahead;
    double F[kFdt + 1];
    if (doStep) {
      constexpr bool JR = false;
#include "imu_chain_group_body.hpp"
      time = s.nexttime;
      ++steps;
      if (s.nexttime == it.t_end) done = true;
    }
    if (COV) {
      // P <- F P F^T + Q (:684-707): M = F P (column l), exchange, P' = F M^T (column l)
      if (doStep && l < 15) {
        double Mc[15];
        applyF(F, Pc, Mc);
#pragma unroll
        for (int e = 0; e < 15; ++e) M[l * kColStride + e] = Mc[e];
      }
      __syncthreads();
      if (doStep && l < 15) {
        double Mr[15];
#pragma unroll
        for (int e = 0; e < 15; ++e) Mr[e] = M[e * kColStride + l];
        applyF(F, Mr, Pc);
        const double dt = s.dt;
        double sg = A.par[2], sa = A.par[3];
        if (s.gyr_sat) sg *= 100;
        if (s.acc_sat) sa *= 100;
        const double s2a = dt * sg * sg, s2v = dt * sa * A.par[3], s2p = 0.5 * dt * dt * s2v;
        const double s2bg = dt * A.par[4] * A.par[4], s2ba = dt * A.par[5] * A.par[5];
        const double q = l < 3 ? s2p : (l < 6 ? s2a : (l < 9 ? s2v : (l < 12 ? s2bg : s2ba)));
#pragma unroll
        for (int e = 0; e < 15; ++e) Pc[e] += (e == l) ? q : 0.0;
      }
      __syncthreads();
    }
  }

  if (live && l == 0) gmemw(A.steps)[i] = steps;
  if (inR && !live && l == 0) gmemw(A.steps)[i] = -1;
  const auto pose = gmem(A.poses + 7 * (size_t)ic);
  const Q q0 = qnormalize(Q{pose[3], pose[4], pose[5], pose[6]});
  double C0[9];
  qrot(q0, C0);

  // Jacobian (:735-746): lane 0 stages F row-major in the group's LDS, the group copies it out
  if (A.jac) {
    if (live && l == 0) {
#pragma unroll
      for (int e = 0; e < 225; ++e) M[e] = (e / 15 == e % 15) ? 1.0 : 0.0;
      double Cv[3], B[9];
      mv3(C0, adi, Cv);
      M[0 * 15 + 4] = Cv[2];  M[0 * 15 + 5] = -Cv[1];  // -[C_WS_0 acc_doubleintegral]x
      M[1 * 15 + 3] = -Cv[2]; M[1 * 15 + 5] = Cv[0];
      M[2 * 15 + 3] = Cv[1];  M[2 * 15 + 4] = -Cv[0];
      mv3(C0, ai, Cv);
      M[6 * 15 + 4] = Cv[2];  M[6 * 15 + 5] = -Cv[1];  // -[C_WS_0 acc_integral]x
      M[7 * 15 + 3] = -Cv[2]; M[7 * 15 + 5] = Cv[0];
      M[8 * 15 + 3] = Cv[1];  M[8 * 15 + 4] = -Cv[0];
#pragma unroll
      for (int r = 0; r < 3; ++r) M[r * 15 + 6 + r] = Dt;
      mm3(C0, dpdbg, B);
#pragma unroll
      for (int e = 0; e < 9; ++e) M[(e / 3) * 15 + 9 + e % 3] = B[e];
      mm3(C0, Cdi, B);
#pragma unroll
      for (int e = 0; e < 9; ++e) M[(e / 3) * 15 + 12 + e % 3] = -B[e];
      mm3(C0, dadbg, B);
#pragma unroll
      for (int e = 0; e < 9; ++e) M[(3 + e / 3) * 15 + 9 + e % 3] = -B[e];
      mm3(C0, dvdbg, B);
#pragma unroll
      for (int e = 0; e < 9; ++e) M[(6 + e / 3) * 15 + 9 + e % 3] = B[e];
      mm3(C0, Ci, B);
#pragma unroll
      for (int e = 0; e < 9; ++e) M[(6 + e / 3) * 15 + 12 + e % 3] = -B[e];
    }
    __syncthreads();
    if (live) {
      const auto J = gmemw(A.jac + 225 * (size_t)i);
      for (int e = l; e < 225; e += kPropGroup) J[e] = M[e];
    }
    __syncthreads();
  }

  // covariance (:749-757): P = T P_delta T^T, T = diag(C0, C0, C0, I, I). Column l of T P_delta,
  // exchange, then row l of P = T (row l of T P_delta)
  if (COV) {
    if (live && l < 15) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double o[3];
        mv3(C0, Pc + 3 * b, o);
        M[l * kColStride + 3 * b] = o[0]; M[l * kColStride + 3 * b + 1] = o[1]; M[l * kColStride + 3 * b + 2] = o[2];
      }
#pragma unroll
      for (int e = 9; e < 15; ++e) M[l * kColStride + e] = Pc[e];
    }
    __syncthreads();
    if (live && l < 15) {
      double Mr[15];
#pragma unroll
      for (int e = 0; e < 15; ++e) Mr[e] = M[e * kColStride + l];
      const auto Pout = gmemw(A.cov + 225 * (size_t)i + 15 * l);
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double o[3];
        mv3(C0, Mr + 3 * b, o);
        Pout[3 * b] = o[0]; Pout[3 * b + 1] = o[1]; Pout[3 * b + 2] = o[2];
      }
#pragma unroll
      for (int e = 9; e < 15; ++e) Pout[e] = Mr[e];
    }
  }

  if (live && l == 0 && steps > 0) writeState(A, i, q0, C0, v0, Dq, ai, adi, Dt);
}

void launch_imu_propagate(const ImuPropagateDev& A, hipStream_t s) {
  if (A.n <= 0) return;
  if (A.cov)
    k_imu_propagate_group<true><<<(A.n + kGroupsPerWave - 1) / kGroupsPerWave, 64, 0, s>>>(A);
  else if (A.jac)
    k_imu_propagate_group<false><<<(A.n + kGroupsPerWave - 1) / kGroupsPerWave, 64, 0, s>>>(A);
  else
    k_imu_propagate_lane<<<(A.n + 63) / 64, 64, 0, s>>>(A);
}

}  // namespace okg
