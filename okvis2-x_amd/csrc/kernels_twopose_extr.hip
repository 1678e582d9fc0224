// kernels_twopose_extr.hip — TwoPoseExtrinsicsGraphError (okvis_ceres/src/TwoPoseExtrinsicsGraphError.cpp),
// the pose-graph edge marginalisation leaves with do_extrinsics: true: compute() (:73-330) and
// EvaluateWithMinimalJacobians (:393-610) for a batch of edges, one workgroup per edge. The edge
// couples the relative pose with the C extrinsics blocks: D = 6 + 6 C residuals, camera c in rows and
// columns 6 + 6 c .. 11 + 6 c (stayConst_ = true).
//
// k_twopose_extr_compute, 256 threads:
//   pass 1  landmarks dealt to the threads. A thread linearises its landmark's observations in S0
//           coordinates (|r| > 3 dropped, Cauchy corrector), does the 3x3 eigen-solve of
//           PseudoInverse::symmSqrt and leaves per kept observation J0, J2, r, A and per landmark V^+,
//           b1 and the keep flag in a scratch slab (written and read by this workgroup only).
//   pass 2  the relative system lives in LDS, compacted to the rows of the pose and of the cameras
//           the edge observes (an unobserved camera has no entry anywhere; its outputs stay the zeros
//           the runtime filled in). Per chunk of 16 landmarks the threads first form W = H01 and
//           W V^+ (D x 3 each), then every thread owns entries (a, b >= a) of the upper triangle plus
//           the right-hand side column and adds the chunk's landmarks in landmark order, the
//           observations of a landmark in observation order: sum H00_l in one matrix, sum W V^+ W^T in
//           the other, subtracted once at the end as the reference does. No atomics: an entry has one
//           owner and one order, whatever the batch.
//   eigen   cyclic Jacobi with round-robin pairing: floor(n/2) disjoint rotations per step (angles,
//           then columns of A and V, then rows of A), n - 1 steps per sweep, the convergence test and
//           the 32-sweep cap of jacobiEigenSym. Ascending rank sort, then J_ = D^(1/2) E^T (zero rows
//           first, for the dropped eigenvalues) and DeltaX_ = -E D^-1 E^T b0_.
// Every loop is bounded by the input sizes or by constants; workgroups do not communicate.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_problem.hpp"
#include "launch.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

namespace {

constexpr int kTpxThreads = 256;
constexpr int kTpxLd = kTwoPoseMaxD + 1;  // 43 doubles: odd row stride (a column walk of 32 lanes hits 32
                                          // distinct bank pairs); column n holds the right-hand side
constexpr int kTpxChunk = 16;             // landmarks staged per pass-2 step
constexpr int kTpxOtherBit = 1 << 8;      // "saw the other keyframe" in the camera mask

}  // namespace

__global__ __launch_bounds__(kTpxThreads) void k_twopose_extr_compute(TwoPoseExtrDev X) {
  const TwoPoseDev& T = X.in;
  const int e = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nc = T.n_cam, D = 6 + 6 * nc;

  __shared__ double sH[kTwoPoseMaxD * kTpxLd];
  __shared__ double sE[kTwoPoseMaxD * kTpxLd];
  __shared__ double sW[kTpxChunk * kTwoPoseMaxD * 3];
  __shared__ double sWV[kTpxChunk * kTwoPoseMaxD * 3];
  __shared__ double sB1[kTpxChunk * 3];
  __shared__ double sCS[kTwoPoseMaxD];
  __shared__ double sLam[kTwoPoseMaxD], sEtb[kTwoPoseMaxD];
  __shared__ int sKeep[kTpxChunk], sOb[kTpxChunk], sOe[kTpxChunk];
  __shared__ int sP[kTwoPoseMaxD / 2], sQ[kTwoPoseMaxD / 2];
  __shared__ int sAct[kTwoPoseMaxD], sInv[kTwoPoseMaxD];
  __shared__ int sMask[kTpxThreads / 64];
  __shared__ int sCont;

  const double* P0 = T.ref_pose + 7 * (size_t)e;
  const double* P1 = T.other_pose + 7 * (size_t)e;
  const Q q0 = qnormalize(Q{P0[3], P0[4], P0[5], P0[6]}), q1 = qnormalize(Q{P1[3], P1[4], P1[5], P1[6]});
  double C0[9];
  qrot(q0, C0);  // C_WS0 (C_S0W = C0^T)
  const double d01[3] = {P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2]};
  double rel[7];  // T_S0S1 = T_WS0^-1 T_WS1
  mtv3(C0, d01, rel);
  const Q qr = qnormalize(qmul(qinv(q0), q1));
  rel[3] = qr.x; rel[4] = qr.y; rel[5] = qr.z; rel[6] = qr.w;
  const double ident[7] = {0, 0, 0, 0, 0, 0, 1};
  double Crel[9];
  qrot(qnormalize(qr), Crel);  // as reprojectA forms C_WS from the pose it is given
  const double Cid[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

  // ---------------------------------------------------------------- pass 1: linearise, 3x3 solves
  const int lb = T.lm_begin[e], le = T.lm_begin[e + 1];
  int mask = 0;
  for (int l = lb + tid; l < le; l += kTpxThreads) {
    const double* hw = T.lm + 4 * (size_t)l;
    const double dw[3] = {hw[0] - P0[0] * hw[3], hw[1] - P0[1] * hw[3], hw[2] - P0[2] * hw[3]};
    double hp[4];
    mtv3(C0, dw, hp);  // hp_S0 = T_S0W hp_W
    hp[3] = hw[3];
    const double minDist = hp[2] / hp[3];
    double H11[6] = {0, 0, 0, 0, 0, 0}, b1[3] = {0, 0, 0};
    for (int o = T.obs_begin[l]; o < T.obs_begin[l + 1]; ++o) {
      const bool other = T.obs_other[o] != 0;
      const int ci = T.obs_cam[o];
      mask |= (1 << ci) | (other ? kTpxOtherBit : 0);  // before the outlier test (:194-197)
      const int flag = (other ? 2 : 0) | (ci << 2);
      const Cam cam = loadCam(T.cam + kCamDoubles * ci);
      const double* ex = T.extr + 7 * ci;
      double r[2], A[6], p[3];
      reprojectA(cam, other ? rel : ident, hp, ex, T.obs_L + 4 * (size_t)o, T.obs_kp + 2 * (size_t)o, r, A, p);
      if (sqrt(r[0] * r[0] + r[1] * r[1]) > 3.0) {  // obvious outliers (:211-213)
        X.obs_flag[o] = flag;
        continue;
      }
      if (T.obs_cauchy[o]) {  // Corrector, CauchyLoss (rho'' < 0): scale by sqrt(rho')
        const double s = sqrt(fmax(DBL_MIN, 1.0 / (1.0 + r[0] * r[0] + r[1] * r[1])));
        r[0] *= s; r[1] *= s;
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i] *= s;
      }
      double J0[12], Jl[6], J2[12];
      obsJacobians(A, p, hp[3], J0, Jl);  // J0 = [w A, -A [p]x], J1 = -A
      extrJacobian(A, other ? Crel : Cid, p, hp[3], ex, J2);
      double* R = X.obs_rec + (size_t)kTpxObsRec * o;
#pragma unroll
      for (int i = 0; i < 12; ++i) { R[i] = J0[i]; R[12 + i] = J2[i]; }
      R[24] = r[0]; R[25] = r[1];
#pragma unroll
      for (int i = 0; i < 6; ++i) R[26 + i] = A[i];
      X.obs_flag[o] = flag | 1;
      int k = 0;
      for (int a = 0; a < 3; ++a) {
        for (int b = a; b < 3; ++b) H11[k++] += A[a] * A[b] + A[3 + a] * A[3 + b];
        b1[a] += A[a] * r[0] + A[3 + a] * r[1];  // -J1^T r
      }
    }
    // V^+ with the symmSqrt clamp: eigenvalues <= tol map to 1/tol
    double V[9] = {H11[0], H11[1], H11[2], H11[1], H11[3], H11[4], H11[2], H11[4], H11[5]};
    double lam[3], Ev[9];
    jacobiEigenSym<3>(V, lam, Ev);
    const double tol = fmax(1.0e-7, 1.0e-7 * 3.0 * lam[2]);
    const int rank = (lam[0] > tol) + (lam[1] > tol) + (lam[2] > tol);
    double f[3];
    for (int i = 0; i < 3; ++i) {
      const double s = sqrt(lam[i] > tol ? 1.0 / lam[i] : 1.0 / tol);
      f[i] = s * s;
    }
    double* Lr = X.lm_rec + (size_t)kTpxLmRec * l;
    int k = 0;
    for (int a = 0; a < 3; ++a)
      for (int b = a; b < 3; ++b)
        Lr[k++] = Ev[a * 3 + 0] * f[0] * Ev[b * 3 + 0] + Ev[a * 3 + 1] * f[1] * Ev[b * 3 + 1] +
                  Ev[a * 3 + 2] * f[2] * Ev[b * 3 + 2];
    Lr[6] = b1[0]; Lr[7] = b1[1]; Lr[8] = b1[2];
    Lr[9] = (rank < 3 && minDist < 2.99) ? 0.0 : 1.0;  // :292-300
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) mask |= __shfl_xor(mask, sh, 64);
  if (lane == 0) sMask[wave] = mask;
  for (int i = tid; i < kTwoPoseMaxD * kTpxLd; i += kTpxThreads) { sH[i] = 0.0; sE[i] = 0.0; }
  __syncthreads();  // also makes pass 1's scratch records visible to the workgroup
  mask = sMask[0] | sMask[1] | sMask[2] | sMask[3];
  int na = 6;  // rows of the compacted system: the pose, then the observed cameras in order
  for (int c = 0; c < nc; ++c) na += ((mask >> c) & 1) ? 6 : 0;
  if (tid == 0) {
    int n = 0;
    for (int i = 0; i < 6; ++i) sAct[n++] = i;
    for (int c = 0; c < nc; ++c)
      if ((mask >> c) & 1)
        for (int i = 0; i < 6; ++i) sAct[n++] = 6 + 6 * c + i;
  }
  __syncthreads();

  // ---------------------------------------------------------------- pass 2: the D x D system
  const int nItems = na * (na + 1);
  for (int c0 = lb; c0 < le; c0 += kTpxChunk) {
    const int ng = min(kTpxChunk, le - c0);
    if (tid < ng) {
      const int l = c0 + tid;
      const double* Lr = X.lm_rec + (size_t)kTpxLmRec * l;
      sKeep[tid] = Lr[9] != 0.0;
      sOb[tid] = T.obs_begin[l];
      sOe[tid] = T.obs_begin[l + 1];
      sB1[3 * tid] = Lr[6]; sB1[3 * tid + 1] = Lr[7]; sB1[3 * tid + 2] = Lr[8];
    }
    for (int it = tid; it < ng * na; it += kTpxThreads) {  // W = H01 rows and W V^+
      const int g = it / na, a = it - g * na, l = c0 + g;
      const double* Lr = X.lm_rec + (size_t)kTpxLmRec * l;
      double w[3] = {0, 0, 0}, wv[3] = {0, 0, 0};
      if (Lr[9] != 0.0) {
        const int fa = sAct[a];
        const int ca = fa < 6 ? -1 : (fa - 6) / 6, ka = fa < 6 ? fa : 12 + (fa - 6) % 6;
        for (int o = T.obs_begin[l]; o < T.obs_begin[l + 1]; ++o) {
          const int fl = X.obs_flag[o];
          if (!(fl & 1)) continue;
          if (ca < 0 ? !(fl & 2) : (fl >> 2) != ca) continue;
          const double* R = X.obs_rec + (size_t)kTpxObsRec * o;
          const double j0 = R[ka], j1 = R[ka + 6];
          for (int j = 0; j < 3; ++j) w[j] -= j0 * R[26 + j] + j1 * R[29 + j];  // J^T J1, J1 = -A
        }
        const double Vp[9] = {Lr[0], Lr[1], Lr[2], Lr[1], Lr[3], Lr[4], Lr[2], Lr[4], Lr[5]};
        for (int j = 0; j < 3; ++j) wv[j] = w[0] * Vp[j] + w[1] * Vp[3 + j] + w[2] * Vp[6 + j];
      }
      const int at = (g * kTwoPoseMaxD + a) * 3;
      for (int j = 0; j < 3; ++j) { sW[at + j] = w[j]; sWV[at + j] = wv[j]; }
    }
    __syncthreads();
    for (int it = tid; it < nItems; it += kTpxThreads) {
      const int a = it / (na + 1), b = it - a * (na + 1);
      if (b < a) continue;
      const bool rhs = b == na;
      const int fa = sAct[a], fb = rhs ? 0 : sAct[b];
      const int ca = fa < 6 ? -1 : (fa - 6) / 6, ka = fa < 6 ? fa : 12 + (fa - 6) % 6;
      const int cb = fb < 6 ? -1 : (fb - 6) / 6, kb = fb < 6 ? fb : 12 + (fb - 6) % 6;
      // H00 has pose x pose, pose x camera and camera x same camera blocks only (:265-276)
      const bool direct = rhs || ca < 0 || ca == cb;
      double h = sH[a * kTpxLd + b], m = sE[a * kTpxLd + b];
      for (int g = 0; g < ng; ++g) {
        if (!sKeep[g]) continue;
        if (direct) {
          double hl = 0.0;
          for (int o = sOb[g]; o < sOe[g]; ++o) {
            const int fl = X.obs_flag[o];
            if (!(fl & 1)) continue;
            if (ca < 0 ? !(fl & 2) : (fl >> 2) != ca) continue;
            const double* R = X.obs_rec + (size_t)kTpxObsRec * o;
            if (rhs) {
              hl -= R[ka] * R[24] + R[ka + 6] * R[25];
            } else {
              if (cb >= 0 && (fl >> 2) != cb) continue;
              hl += R[ka] * R[kb] + R[ka + 6] * R[kb + 6];
            }
          }
          h += hl;
        }
        const double* wv = sWV + (g * kTwoPoseMaxD + a) * 3;
        const double* wb = rhs ? sB1 + 3 * g : sW + (g * kTwoPoseMaxD + b) * 3;
        m += wv[0] * wb[0] + wv[1] * wb[1] + wv[2] * wb[2];
      }
      sH[a * kTpxLd + b] = h;
      sE[a * kTpxLd + b] = m;
    }
    __syncthreads();
  }
  // H00_ -= mH, b0_ -= mb; both triangles; the results in the caller's (full) indices
  double* oH = X.H00 + (size_t)D * D * e;
  double* ob = X.b0 + (size_t)D * e;
  for (int it = tid; it < nItems; it += kTpxThreads) {
    const int a = it / (na + 1), b = it - a * (na + 1);
    if (b < a) continue;
    const double v = sH[a * kTpxLd + b] - sE[a * kTpxLd + b];
    sH[a * kTpxLd + b] = v;
    const int fa = sAct[a];
    if (b == na) {
      ob[fa] = v;
    } else {
      const int fb = sAct[b];
      sH[b * kTpxLd + a] = v;
      oH[fa * D + fb] = v;
      oH[fb * D + fa] = v;
    }
  }
  __syncthreads();
  for (int it = tid; it < na * na; it += kTpxThreads) {
    const int i = it / na, j = it - i * na;
    sE[i * kTpxLd + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();

  // ---------------------------------------------------------------- eigen-solve: A = sH, V = sE
  const int mEven = (na + 1) & ~1, half = mEven / 2;
  for (int sweep = 0; sweep < 32; ++sweep) {
    if (wave == 0) {
      double off = 0.0, dg = 0.0;
      for (int i = lane; i < na; i += 64) {
        dg += sH[i * kTpxLd + i] * sH[i * kTpxLd + i];
        for (int j = i + 1; j < na; ++j) off += sH[i * kTpxLd + j] * sH[i * kTpxLd + j];
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) {
        off += __shfl_xor(off, sh, 64);
        dg += __shfl_xor(dg, sh, 64);
      }
      if (lane == 0) sCont = !(off <= 1e-36 * dg || off == 0.0);
    }
    __syncthreads();
    if (!sCont) break;  // uniform over the workgroup
    for (int step = 0; step < mEven - 1; ++step) {
      if (tid < half) {  // round robin: player mEven-1 stays, the others rotate
        const int r = mEven - 1;
        const int u = tid == 0 ? r : (step + tid) % r, v = tid == 0 ? step : (step - tid + r) % r;
        const int p = min(u, v), q = max(u, v);
        double c = 1.0, s = 0.0;
        bool rot = false;
        if (q < na) {  // (an odd n plays against a dummy)
          const double apq = sH[p * kTpxLd + q];
          if (apq != 0.0) {
            const double theta = (sH[q * kTpxLd + q] - sH[p * kTpxLd + p]) / (2.0 * apq);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            rot = true;
          }
        }
        sP[tid] = p;
        sQ[tid] = rot ? q : -1;
        sCS[2 * tid] = c;
        sCS[2 * tid + 1] = s;
      }
      __syncthreads();
      for (int it = tid; it < na * half; it += kTpxThreads) {  // columns p, q of A and of V
        const int i = it / half, k = it - i * half;
        const int p = sP[k], q = sQ[k];
        if (q < 0) continue;
        const double c = sCS[2 * k], s = sCS[2 * k + 1];
        const double akp = sH[i * kTpxLd + p], akq = sH[i * kTpxLd + q];
        sH[i * kTpxLd + p] = c * akp - s * akq;
        sH[i * kTpxLd + q] = s * akp + c * akq;
        const double vkp = sE[i * kTpxLd + p], vkq = sE[i * kTpxLd + q];
        sE[i * kTpxLd + p] = c * vkp - s * vkq;
        sE[i * kTpxLd + q] = s * vkp + c * vkq;
      }
      __syncthreads();
      for (int it = tid; it < half * na; it += kTpxThreads) {  // rows p, q of A
        const int k = it / na, j = it - k * na;
        const int p = sP[k], q = sQ[k];
        if (q < 0) continue;
        const double c = sCS[2 * k], s = sCS[2 * k + 1];
        const double apk = sH[p * kTpxLd + j], aqk = sH[q * kTpxLd + j];
        sH[p * kTpxLd + j] = j == q ? 0.0 : c * apk - s * aqk;
        sH[q * kTpxLd + j] = j == p ? 0.0 : s * apk + c * aqk;
      }
      __syncthreads();
    }
  }

  // ---------------------------------------------------------------- sort ascending, outputs
  if (tid < na) sLam[tid] = sH[tid * kTpxLd + tid];
  __syncthreads();
  if (tid < na) {
    const double li = sLam[tid];
    int rank = 0;
    for (int j = 0; j < na; ++j) rank += (sLam[j] < li || (sLam[j] == li && j < tid)) ? 1 : 0;
    sInv[rank] = tid;
  }
  __syncthreads();
  const double tolD = 1.0e-8 * (double)D * sLam[sInv[na - 1]];  // H00_.cols() * largest eigenvalue (:309)
  if (tid < na) {
    double s = 0.0;
    for (int k = 0; k < na; ++k) s += sE[k * kTpxLd + tid] * sH[k * kTpxLd + na];
    sEtb[tid] = sLam[tid] > tolD ? s / sLam[tid] : 0.0;
  }
  __syncthreads();
  double* oJ = X.sqrt_info + (size_t)D * D * e;
  for (int it = tid; it < na * na; it += kTpxThreads) {
    const int r = it / na, k = it - r * na, i = sInv[r];
    // J_ row = sqrt(lambda_i) e_i^T; the dropped eigenvalues (and the unobserved cameras') rows come first
    if (sLam[i] > tolD) oJ[(size_t)(D - na + r) * D + sAct[k]] = sqrt(sLam[i]) * sE[k * kTpxLd + i];
  }
  if (tid < na) {
    double s = 0.0;
    for (int r = 0; r < na; ++r) s += sE[tid * kTpxLd + sInv[r]] * sEtb[sInv[r]];
    X.delta_x[(size_t)D * e + sAct[tid]] = 0.0 - s;  // DeltaX_ = -H^+ b0_
  }
  if (tid < 7) X.lin_point[7 * (size_t)e + tid] = (mask & kTpxOtherBit) ? rel[tid] : ident[tid];
  if (tid < nc) X.seen[(size_t)nc * e + tid] = (uint8_t)((mask >> tid) & 1);
}

// One wavefront per edge: error = DeltaX_ + (difference to the linearisation point), r = J_ error and
// the minimal Jacobians J_[:, block] Jerr of the two poses and the C extrinsics blocks.
__global__ __launch_bounds__(64) void k_twopose_extr_eval(TwoPoseExtrEvalDev T) {
  const int e = blockIdx.x, tid = threadIdx.x;
  const int nc = T.n_cam, D = 6 + 6 * nc;
  __shared__ double sErr[kTwoPoseMaxD];
  __shared__ double sC0[9], sB[9], sCX[9];
  __shared__ double sBex[kTwoPoseMaxCam * 9];
  const double* J = T.sqrt_info + (size_t)D * D * e;
  const double* dx = T.delta_x + (size_t)D * e;
  if (tid == 0) {
    const double* lp = T.lin_point + 7 * (size_t)e;
    const Q ql = qnormalize(Q{lp[3], lp[4], lp[5], lp[6]});
    const Q qlinv = qinv(ql);
    Q q0, q1, q0inv, qrel;
    double C0[9], d01[3], rS[3], B[9], CX[9];
    relPoseFrame(T.ref_pose + 7 * (size_t)e, T.other_pose + 7 * (size_t)e, q0, q1, C0, d01, rS, q0inv, qrel);
    const Q dq = qmul(qrel, qlinv);
    sErr[0] = dx[0] + rS[0] - lp[0]; sErr[1] = dx[1] + rS[1] - lp[1]; sErr[2] = dx[2] + rS[2] - lp[2];
    sErr[3] = dx[3] + 2.0 * dq.x; sErr[4] = dx[4] + 2.0 * dq.y; sErr[5] = dx[5] + 2.0 * dq.z;
    plusOplus3(q0inv, qmul(q1, qlinv), B);  // Jerr = [C_S0W 0; 0 B] (:492-497)
    ctCrossMx(C0, d01, CX);                 // JerrRef = [-C_S0W, C_S0W [r_WS - r_WS0]x; 0, -B] (:501-506)
    for (int i = 0; i < 9; ++i) { sC0[i] = C0[i]; sB[i] = B[i]; sCX[i] = CX[i]; }
  } else if (tid <= nc) {
    const int c = tid - 1;
    double* er = sErr + 6 + 6 * c;
    double* Bx = sBex + 9 * c;
    for (int i = 0; i < 6; ++i) er[i] = dx[6 + 6 * c + i];
    for (int i = 0; i < 9; ++i) Bx[i] = 0.0;
    if (T.seen[(size_t)nc * e + c]) {  // linearisationPoints_T_SC_[c] is set (:439-448, :572-578)
      const double* x = T.extr + 7 * c;
      const double* xl = T.lin_extr + 7 * ((size_t)nc * e + c);
      const Q dq = qmul(qnormalize(Q{x[3], x[4], x[5], x[6]}), qinv(qnormalize(Q{xl[3], xl[4], xl[5], xl[6]})));
      er[0] += x[0] - xl[0]; er[1] += x[1] - xl[1]; er[2] += x[2] - xl[2];
      er[3] += 2.0 * dq.x; er[4] += 2.0 * dq.y; er[5] += 2.0 * dq.z;
      double Om[16];
      qoplusM(dq, Om);
      for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) Bx[r * 3 + q] = Om[r * 4 + q];
    }
  }
  __syncthreads();
  if (T.r && tid < D) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += J[tid * D + k] * sErr[k];
    T.r[(size_t)D * e + tid] = s;
  }
  for (int it = tid; it < D * 3; it += 64) {
    const int i = it / 3, q = it - 3 * i;
    const double* Jr = J + i * D;
    const double jt = Jr[0] * sC0[q * 3 + 0] + Jr[1] * sC0[q * 3 + 1] + Jr[2] * sC0[q * 3 + 2];  // (J C0^T)_q
    const double jb = Jr[3] * sB[0 * 3 + q] + Jr[4] * sB[1 * 3 + q] + Jr[5] * sB[2 * 3 + q];
    const double jx = Jr[0] * sCX[0 * 3 + q] + Jr[1] * sCX[1 * 3 + q] + Jr[2] * sCX[2 * 3 + q];
    if (T.J_ref) {
      double* o = T.J_ref + ((size_t)D * e + i) * 6;
      o[q] = -jt;
      o[3 + q] = jx - jb;
    }
    if (T.J_other) {
      double* o = T.J_other + ((size_t)D * e + i) * 6;
      o[q] = jt;
      o[3 + q] = jb;
    }
  }
  if (T.J_extr)
    for (int it = tid; it < nc * D * 3; it += 64) {
      const int c = it / (D * 3), rem = it - c * D * 3, i = rem / 3, q = rem - 3 * i;
      double* o = T.J_extr + (((size_t)nc * e + c) * D + i) * 6;
      if (T.seen[(size_t)nc * e + c]) {  // Jerrex = [I 0; 0 oplus(q_SC q_lin^-1)_3x3]
        const double* Jr = J + i * D + 6 + 6 * c;
        const double* Bx = sBex + 9 * c;
        o[q] = Jr[q];
        o[3 + q] = Jr[3] * Bx[0 * 3 + q] + Jr[4] * Bx[1 * 3 + q] + Jr[5] * Bx[2 * 3 + q];
      } else {
        o[q] = 0.0;
        o[3 + q] = 0.0;
      }
    }
}

void launch_twopose_extr_compute(const TwoPoseExtrDev& T, hipStream_t s) {
  if (T.in.n_edges > 0) hipLaunchKernelGGL(k_twopose_extr_compute, dim3(T.in.n_edges), dim3(kTpxThreads), 0, s, T);
}

void launch_twopose_extr_eval(const TwoPoseExtrEvalDev& T, hipStream_t s) {
  if (T.n_edges > 0) hipLaunchKernelGGL(k_twopose_extr_eval, dim3(T.n_edges), dim3(64), 0, s, T);
}

}  // namespace okg
