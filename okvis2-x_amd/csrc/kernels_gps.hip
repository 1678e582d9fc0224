// kernels_gps.hip — the GNSS factors of ViGraph::addGpsMeasurement (ViGraph.cpp:973-1006) for a batch
// of independent factors on gfx950 (FP64): GpsErrorAsynchronous::EvaluateWithMinimalJacobians
// (GpsErrorAsynchronous.cpp:98-300) with its own IMU pre-integration from the state's stamp t_k to the
// fix's stamp t_g (redoPreintegration, :303-507), and GpsErrorSynchronous (GpsErrorSynchronous.cpp:41-144).
//
//  k_gps_async<COV, NP>  one 16-lane group per factor (four per wavefront), the layout of
//                        k_imu_propagate_group: every lane of the group runs the scalar chain
//                        (:402-432), so the block-sparse F_delta (:437-452) is register resident; lane
//                        l < 15 owns column l of the covariance and P <- F P F^T + K takes one LDS
//                        transpose per step. The redo decision (:134-142) is made here; a factor that
//                        does not re-integrate loads its increments from `state` and is predicated off
//                        in the sample loop. The residual stage (:145-294) follows in the same group:
//                        it needs the leading 6x6 of P_delta only, which goes through LDS, never HBM.
//                        COV = use_imu_covariance. NP = 1 carries P = sum_j sigma_j^2 dPdsigma_j (the
//                        recursion and the symmetrisation are linear, and nothing else reads
//                        dPdsigma_); NP = 4 carries the reference's four matrices (the timing
//                        comparison of scripts/gps_timing.py).
//  k_gps_sync            one lane per factor: no chain, sqrt_info = LLT(information).L^T.
//
// A factor's arithmetic does not depend on the batch or on its position in it: loops run to the
// wavefront's longest re-integrating factor with the others predicated off, and no lane reads another
// factor's data. The host has refused every factor whose samples do not cover [t_k, t_g].
#include "imu_chain.hpp"
#include "launch.hpp"
#include "mat3_spd.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

namespace {

// C = A B for row-major A [R x K], B [K x N]
template <int R, int K, int N>
__device__ __forceinline__ void mmul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) s += A[r * K + k] * B[k * N + c];
      C[r * N + c] = s;
    }
}

// The diagonal entry l of K_j of one step (:455-463), j = 0..3 (sigma_g_c, sigma_a_c, sigma_gw_c,
// sigma_aw_c): the gyro factor enters once, the accelerometer factor cubed in the position block.
__device__ __forceinline__ double gpsNoise(int j, int l, const PropStep& s) {
  const double dt = s.dt, gm = s.gyr_sat ? 100.0 : 1.0, am = s.acc_sat ? 100.0 : 1.0;
  if (j == 0) return (l >= 3 && l < 6) ? gm * dt : 0.0;
  if (j == 1) return l < 3 ? 0.5 * dt * dt * dt * am * am * am : ((l >= 6 && l < 9) ? am * dt : 0.0);
  if (j == 2) return (l >= 9 && l < 12) ? dt : 0.0;
  return l >= 12 ? dt : 0.0;
}

// minimal [3 x 6] -> ambient [3 x 7]: J PoseManifold::minusJacobian(x) (PoseLocalParameterization.cpp:90-103),
// whose rotation block is 2 oplus(q^-1).topRows<3>() with the conjugate of x's quaternion as stored
__device__ __forceinline__ void liftRows(const double* J, const double* x, double* out) {
  double O[16];
  qoplusM(Q{-x[3], -x[4], -x[5], x[6]}, O);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[r * 7 + c] = J[r * 6 + c];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      out[r * 7 + 3 + c] = J[r * 6 + 3] * (2.0 * O[c]) + J[r * 6 + 4] * (2.0 * O[4 + c]) + J[r * 6 + 5] * (2.0 * O[8 + c]);
  }
}

template <int N>
__device__ __forceinline__ void storeRow(double* base, size_t i, const double* v) {
  if (!base) return;
  const auto o = gmemw(base + N * i);
#pragma unroll
  for (int e = 0; e < N; ++e) o[e] = v[e];
}

// What both functors do from the antenna position on (GpsErrorAsynchronous.cpp:200-294,
// GpsErrorSynchronous.cpp:80-140), written by one lane: error = z - (C_GW (r + a) + r_GW) with r the
// sensor position and a = C_WS r_SA at the fix's stamp, r = S error, and the Jacobians S Jmin with
// Jpose / Jsb the functor's minimal ones before the weighting (Jsb == nullptr: zeros) and J_T_GW =
// [-I, [C_GW (r + a)]x]. S is not differentiated.
__device__ __forceinline__ void gpsFinish(const GpsDev& A, int i, const double* pose, const double* G, const double* C_GW,
                                          const double* S, const double* rW, const double* aW, const double* Jpose,
                                          const double* Jsb) {
  const auto z = gmem(A.meas + 3 * (size_t)i);
  const double pW[3] = {rW[0] + aW[0], rW[1] + aW[1], rW[2] + aW[2]};
  double pG[3], err[3], r[3];
  mv3(C_GW, pW, pG);
#pragma unroll
  for (int j = 0; j < 3; ++j) err[j] = z[j] - (pG[j] + G[j]);
  mv3(S, err, r);
  storeRow<3>(A.r, i, r);
  storeRow<3>(A.error, i, err);
  storeRow<9>(A.sqrt_info, i, S);
  double J[27], Ja[21];
  if (A.J_pose || A.J_pose_amb) {
    mmul<3, 3, 6>(S, Jpose, J);
    storeRow<18>(A.J_pose, i, J);
    if (A.J_pose_amb) {
      liftRows(J, pose, Ja);
      storeRow<21>(A.J_pose_amb, i, Ja);
    }
  }
  if (A.J_sb) {
    if (Jsb) {
      mmul<3, 3, 9>(S, Jsb, J);
    } else {
#pragma unroll
      for (int e = 0; e < 27; ++e) J[e] = 0.0;
    }
    storeRow<27>(A.J_sb, i, J);
  }
  if (A.J_gw || A.J_gw_amb) {
    double X[9], J2[18];
    crossMx(pG, X);
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J2[rr * 6 + c] = rr == c ? -1.0 : 0.0;
        J2[rr * 6 + 3 + c] = X[rr * 3 + c];
      }
    mmul<3, 3, 6>(S, J2, J);
    storeRow<18>(A.J_gw, i, J);
    if (A.J_gw_amb) {
      liftRows(J, G, Ja);
      storeRow<21>(A.J_gw_amb, i, Ja);
    }
  }
}

// [-C_GW, C_GW [a]x + extra] (extra may be nullptr): the pose Jacobian before the weighting
__device__ __forceinline__ void poseJacobian(const double* C_GW, const double* aW, const double* extra, double* E,
                                             double* J) {
  double X[9];
  crossMx(aW, X);
  mm3(C_GW, X, E);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      J[r * 6 + c] = -C_GW[r * 3 + c];
      J[r * 6 + 3 + c] = extra ? extra[r * 3 + c] + E[r * 3 + c] : E[r * 3 + c];
    }
}

__device__ __forceinline__ const double* gwBlock(const GpsDev& A, int i) {
  return A.T_GW + 7 * (size_t)(A.gw_index ? gmem(A.gw_index)[i] : 0);
}

}  // namespace

// ---- GpsErrorSynchronous: one lane per factor
__global__ __launch_bounds__(64) void k_gps_sync(const GpsDev A) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= A.n) return;
  double pose[7], G[7], info[9], S[9];
  {
    const auto p = gmem(A.poses + 7 * (size_t)i);
    const auto g = gmem(gwBlock(A, i));
    const auto m = gmem(A.info + 9 * (size_t)i);
#pragma unroll
    for (int e = 0; e < 7; ++e) { pose[e] = p[e]; G[e] = g[e]; }
#pragma unroll
    for (int e = 0; e < 9; ++e) info[e] = m[e];
  }
  chol3U(info, S);
  double C_WS[9], C_GW[9], aW[3], E[9], Jp[18];
  qrot(Q{pose[3], pose[4], pose[5], pose[6]}, C_WS);  // (:67-68: the quaternions as stored)
  qrot(Q{G[3], G[4], G[5], G[6]}, C_GW);
  mv3(C_WS, A.r_SA, aW);
  poseJacobian(C_GW, aW, nullptr, E, Jp);
  gpsFinish(A, i, pose, G, C_GW, S, pose, aW, Jp, nullptr);
  if (A.steps) gmemw(A.steps)[i] = 0;
}

// ---- GpsErrorAsynchronous: one 16-lane group per factor
template <bool COV, int NP>
__global__ __launch_bounds__(64) void k_gps_async(const GpsDev A) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int i = (int)blockIdx.x * kGroupsPerWave + g;
  __shared__ double sAll[kGroupsPerWave][15 * kColStride];
  double* const M = sAll[g];

  const bool inR = i < A.n;
  const int ic = inR ? i : 0;
  const int64_t t_k = gmem(A.t_k)[ic], t_g = gmem(A.t_g)[ic];
  const int sbeg = gmem(A.sbegin)[ic], N = gmem(A.sbegin)[ic + 1] - sbeg;
  const auto sbp = gmem(A.sb + 9 * (size_t)ic);
  const double v0[3] = {sbp[0], sbp[1], sbp[2]}, bg[3] = {sbp[3], sbp[4], sbp[5]}, ba[3] = {sbp[6], sbp[7], sbp[8]};
  double* const st = A.state ? A.state + (size_t)kGpsState * ic : nullptr;

  // the redo decision (:134-142); without a state every factor is fresh
  double counter = 0.0, Db[6] = {0, 0, 0, 0, 0, 0};
  bool redo = false;
  if (st) {
    const auto s = gmem(st);
    counter = s[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Db[j] = bg[j] - s[60 + j];
      Db[3 + j] = ba[j] - s[63 + j];
    }
    redo = s[1] != 0.0 || sqrt(Db[0] * Db[0] + Db[1] * Db[1] + Db[2] * Db[2]) > 0.0003;
  }
  const bool doRedo = inR && (A.redo_always != 0 || (redo && N < 50) || counter == 0.0);

  // the increments: identity for a redo (:316-337), else the stored ones
  Q Dq{0.0, 0.0, 0.0, 1.0};
  double C[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  double Ci[9], Cdi[9], cross[9], dadbg[9], dvdbg[9], dpdbg[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) Ci[e] = Cdi[e] = cross[e] = dadbg[e] = dvdbg[e] = dpdbg[e] = 0.0;
  double ai[3] = {0, 0, 0}, adi[3] = {0, 0, 0};
  [[maybe_unused]] double Dt = 0.0;  // (the step body sums it; the residual stage takes t_g - t_k)
  double Pc[NP][15];  // column l of P (NP = 1) or of the four dPdsigma (NP = 4)
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int e = 0; e < 15; ++e) Pc[j][e] = 0.0;
  int steps = 0;
  if (doRedo) {
#pragma unroll
    for (int j = 0; j < 6; ++j) Db[j] = 0.0;
  } else if (inR) {  // (st is set: a factor without a state has counter 0)
    const auto s = gmem(st);
    Dq = Q{s[2], s[3], s[4], s[5]};
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      Ci[e] = s[6 + e];
      Cdi[e] = s[15 + e];
      dadbg[e] = s[30 + e];
      dvdbg[e] = s[39 + e];
      dpdbg[e] = s[48 + e];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ai[j] = s[24 + j];
      adi[j] = s[27 + j];
    }
    steps = (int)s[66];
    if (COV && l < 15) {
#pragma unroll
      for (int e = 0; e < 15; ++e) Pc[0][e] = s[67 + e * 15 + l];
    }
  }

  // ---- the chain (:339-485); uniform trip count over the wavefront (the barriers of the P exchange)
  int64_t time = t_k;
  bool done = !doRedo;
  int Nmax = doRedo ? N : 0;
  Nmax = max(Nmax, __shfl_xor(Nmax, 16, 64));
  Nmax = max(Nmax, __shfl_xor(Nmax, 32, 64));
  const int Nc = max(N, 1);
  RawSample cur = loadRawSample(A.ts, A.ga, sbeg, Nc, 0), nxt = loadRawSample(A.ts, A.ga, sbeg, Nc, 1);
  for (int k = 0; k < Nmax; ++k) {
    const RawSample ahead = loadRawSample(A.ts, A.ga, sbeg, Nc, k + 2);
    PropStep s;
    const bool doStep = !done && k < N && stepSample(A.par[0], A.par[1], N, t_g, k, cur, nxt, time, steps > 0, bg, ba, s);
    cur = nxt;
    nxt = ahead;
    double F[kFdt + 1];
    if (doStep) {
      constexpr bool JR = true;
#include "imu_chain_group_body.hpp"
      time = s.nexttime;
      ++steps;
      if (s.nexttime == t_g) done = true;
    }
    if (COV) {
      // P <- F P F^T + K (:464-467): M = F P (column l), exchange, P' = F M^T (column l)
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        if (doStep && l < 15) {
          double Mc[15];
          applyF(F, Pc[j], Mc);
#pragma unroll
          for (int e = 0; e < 15; ++e) M[l * kColStride + e] = Mc[e];
        }
        __syncthreads();
        if (doStep && l < 15) {
          double Mr[15];
#pragma unroll
          for (int e = 0; e < 15; ++e) Mr[e] = M[e * kColStride + l];
          applyF(F, Mr, Pc[j]);
          double q;
          if (NP == 1) {
            q = A.par[2] * A.par[2] * gpsNoise(0, l, s) + A.par[3] * A.par[3] * gpsNoise(1, l, s) +
                A.par[4] * A.par[4] * gpsNoise(2, l, s) + A.par[5] * A.par[5] * gpsNoise(3, l, s);
          } else {
            q = gpsNoise(j, l, s);
          }
#pragma unroll
          for (int e = 0; e < 15; ++e) Pc[j][e] += (e == l) ? q : 0.0;
        }
        __syncthreads();
      }
    }
  }

  // the symmetrisation and the sigma-weighted sum (:494-500) of a redo
  if (COV) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (doRedo && l < 15) {
#pragma unroll
        for (int e = 0; e < 15; ++e) M[l * kColStride + e] = Pc[j][e];
      }
      __syncthreads();
      if (doRedo && l < 15) {
#pragma unroll
        for (int e = 0; e < 15; ++e) Pc[j][e] = 0.5 * Pc[j][e] + 0.5 * M[e * kColStride + l];
      }
      __syncthreads();
    }
    if constexpr (NP == 4) {
      if (doRedo) {
#pragma unroll
        for (int e = 0; e < 15; ++e) {
          double p = Pc[0][e] * A.par[2] * A.par[2];
          p += Pc[1][e] * A.par[3] * A.par[3];
          p += Pc[2][e] * A.par[4] * A.par[4];
          p += Pc[3][e] * A.par[5] * A.par[5];
          Pc[0][e] = p;
        }
      }
    }
  }

  // ---- the state (a redo: everything; else the flag, :136)
  if (st && inR) {
    const auto s = gmemw(st);
    if (doRedo) {
      if (l == 0) {
        s[0] = counter + 1.0;
        s[1] = 0.0;
        s[2] = Dq.x; s[3] = Dq.y; s[4] = Dq.z; s[5] = Dq.w;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
          s[6 + e] = Ci[e];
          s[15 + e] = Cdi[e];
          s[30 + e] = dadbg[e];
          s[39 + e] = dvdbg[e];
          s[48 + e] = dpdbg[e];
          s[57 + e] = sbp[e];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          s[24 + j] = ai[j];
          s[27 + j] = adi[j];
        }
        s[66] = (double)steps;
      }
      if (l < 15) {  // (symmetric: column l is row l; without the covariance P_delta_ stays zero, :331)
#pragma unroll
        for (int e = 0; e < 15; ++e) s[67 + l * 15 + e] = Pc[0][e];
      }
    } else if (l == 0) {
      s[1] = redo ? 1.0 : 0.0;
    }
  }

  // ---- the residual stage (:145-294); the leading 6x6 of P_delta to every lane of the group
  double P6[36];
  if (COV) {
    if (l < 6) {
#pragma unroll
      for (int e = 0; e < 6; ++e) M[l * kColStride + e] = Pc[0][e];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) P6[r * 6 + c] = M[c * kColStride + r];
  }
  if (!(inR && l == 0)) return;  // (no barrier follows)

  double pose[7], G[7], info[9];
  {
    const auto p = gmem(A.poses + 7 * (size_t)i);
    const auto gw = gmem(gwBlock(A, i));
    const auto m = gmem(A.info + 9 * (size_t)i);
#pragma unroll
    for (int e = 0; e < 7; ++e) { pose[e] = p[e]; G[e] = gw[e]; }
#pragma unroll
    for (int e = 0; e < 9; ++e) info[e] = m[e];
  }
  const Q q0 = qnormalize(Q{pose[3], pose[4], pose[5], pose[6]});  // (Transformation's constructor normalises)
  double C0[9], C_GW[9];
  qrot(q0, C0);
  qrot(Q{G[3], G[4], G[5], G[6]}, C_GW);  // (:117-118: as stored)

  // T_WS at t_g with the first-order bias correction (:147-153)
  const double Dtg = durToSec(t_g - t_k);
  const double gW[3] = {0.0, 0.0, A.par[6]};
  double t0[3], t1[3], inc[3], Cinc[3], rtg[3];
  mv3(dpdbg, Db, t0);
  mv3(Cdi, Db + 3, t1);
#pragma unroll
  for (int j = 0; j < 3; ++j) inc[j] = adi[j] + t0[j] - t1[j];
  mv3(C0, inc, Cinc);
#pragma unroll
  for (int j = 0; j < 3; ++j) rtg[j] = pose[j] + v0[j] * Dtg - 0.5 * gW[j] * Dtg * Dtg + Cinc[j];
  mv3(dadbg, Db, t0);
  const Q qtg = qnormalize(qmul(qmul(q0, Dq), deltaQ(-t0[0], -t0[1], -t0[2])));
  double Ctg[9], aW[3];
  qrot(qtg, Ctg);
  mv3(Ctg, A.r_SA, aW);

  // sqrt_info (:170-194)
  double Ginv[9], W[9], S[9];
  inv3(info, Ginv);  // gpsCovariance_ (:87)
  if (COV) {
    // P.block<6,6>(0,0) of T P_delta T^T: C0 B C0^T per 3x3 block B of the leading 6x6
    double Pw[36];
#pragma unroll
    for (int br = 0; br < 2; ++br)
#pragma unroll
      for (int bc = 0; bc < 2; ++bc) {
        double B[9], CB[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) B[e] = P6[(3 * br + e / 3) * 6 + 3 * bc + e % 3];
        mm3(C0, B, CB);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            Pw[(3 * br + r) * 6 + 3 * bc + c] = CB[r * 3] * C0[c * 3] + CB[r * 3 + 1] * C0[c * 3 + 1] + CB[r * 3 + 2] * C0[c * 3 + 2];
      }
    double a0[3], X[9], E0[9], Jws[18], JP[18], cov[9];
    mv3(C0, A.r_SA, a0);
    crossMx(a0, X);
    mm3(C_GW, X, E0);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Jws[r * 6 + c] = C_GW[r * 3 + c];
        Jws[r * 6 + 3 + c] = -E0[r * 3 + c];
      }
    mmul<3, 6, 6>(Jws, Pw, JP);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += JP[r * 6 + k] * Jws[c * 6 + k];
        cov[r * 3 + c] = Ginv[r * 3 + c] + s;
      }
    inv3(cov, W);
  } else {
    inv3(Ginv, W);
  }
  chol3U(W, S);

  // the Jacobians before the weighting (:156-166, :213-269): Jprop's blocks applied to [-C_GW, E]
  double Cv[3], CX[9], extra[9], E[9], Jp[18], Jsb[27], B1[9], B2[9], B3[9], T1[9], T2[9];
  mv3(C0, adi, Cv);
  crossMx(Cv, CX);
  mm3(C_GW, CX, extra);  // (-C_GW) (-[C0 acc_doubleintegral]x)
  poseJacobian(C_GW, aW, extra, E, Jp);
  mm3(C0, dpdbg, B1);
  mm3(C0, dadbg, B2);
  mm3(C0, Cdi, B3);
  mm3(C_GW, B1, T1);
  mm3(E, B2, T2);
  mm3(C_GW, B3, B1);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Jsb[r * 9 + c] = -C_GW[r * 3 + c] * Dtg;
      Jsb[r * 9 + 3 + c] = -T1[r * 3 + c] - T2[r * 3 + c];
      Jsb[r * 9 + 6 + c] = B1[r * 3 + c];
    }
  gpsFinish(A, i, pose, G, C_GW, S, rtg, aW, Jp, Jsb);
  if (A.steps) gmemw(A.steps)[i] = steps;
}

void launch_gps_evaluate(const GpsDev& A, hipStream_t s) {
  if (A.n <= 0) return;
  if (A.kind == 1) {
    k_gps_sync<<<(A.n + 63) / 64, 64, 0, s>>>(A);
    return;
  }
  const int blocks = (A.n + kGroupsPerWave - 1) / kGroupsPerWave;
  if (!A.use_cov)
    k_gps_async<false, 1><<<blocks, 64, 0, s>>>(A);
  else if (A.four_p)
    k_gps_async<true, 4><<<blocks, 64, 0, s>>>(A);
  else
    k_gps_async<true, 1><<<blocks, 64, 0, s>>>(A);
}

}  // namespace okg
