// kernels_place.hip — the two device-side parts of Frontend::verifyRecognisedPlace (Frontend.cpp:258-602)
// on gfx950, for a batch of candidates:
//
//  k_place_match   :316-345, one wavefront per (landmark, camera). The lanes take the image's keypoints
//                  64 per round, a lane holding its keypoint's descriptor in 12 registers; the landmark's
//                  descriptors are the same for every lane (wave-uniform loads) and are walked in order
//                  inside the round. A lane keeps the first (descriptor, k) attaining its minimum; one
//                  ordered minimum across the lanes at the end (distance, then descriptor, then k) gives
//                  the serial walk's match: the first (descriptor, keypoint) attaining the minimum below
//                  distMin's start, the truncated threshold. Every (landmark, camera) element of both outputs is written.
//  k_place_refine  :434-598, one workgroup per job runs the whole solve: ::ceres::Solve with
//                  TRUST_REGION / LEVENBERG_MARQUARDT on one 6-dimensional pose block, then the outlier
//                  count and H at the result. Lanes take the observations strided; per linearisation the
//                  21 + 6 + 1 sums (J^T J, J^T r, cost) go through blockSumN's fixed-order tree; lane 0
//                  forms the Jacobi scaling, solves the damped 6x6 normal equations by a Cholesky
//                  factorisation, takes every decision of TrustRegionMinimizer and publishes the next
//                  point and what to do there through LDS. No host round trip, no atomics.
//
// Both: a job's result depends on its own rows only and every reduction has a fixed shape, so the bits are
// the same in every batch and on every run. Loop bounds are counts; nothing is read or written past them.
#include "block_reduce.hpp"
#include "launch.hpp"
#include "loss.hpp"
#include "match_geometry.hpp"

namespace okg {

namespace {

__global__ __launch_bounds__(64) void k_place_match(const PlaceMatchDev M) {
  const int item = blockIdx.x;  // (landmark, camera); the grid is n_lm * n_cam
  const int lane = threadIdx.x;
  const int l = item / M.n_cam, im = item - l * M.n_cam;
  const int j = gmem(M.lm_job)[l];
  const int img = gmem(M.job_image)[(size_t)j * M.n_cam + im];
  int kb = 0, K = 0;
  if (img >= 0) {
    kb = gmem(M.kp_begin)[img];
    K = gmem(M.kp_begin)[img + 1] - kb;
  }
  const int db = gmem(M.desc_begin)[l];
  const int nd = gmem(M.desc_begin)[l + 1] - db;
  // the lane's best: the first (descriptor, k) attaining its minimum, k ascending over the rounds
  int best = M.best_init, bestD = 0x7fffffff, bestK = 0x7fffffff;
  for (int base = 0; base < K; base += 64) {
    const int k = base + lane;
    if (k < K) {
      gptr<uint32_t> kd = gmem(M.desc) + 12 * ((size_t)kb + k);
      uint32_t mine[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) mine[i] = kd[i];
      int rb = 0x7fffffff, rd = 0;  // this round's first descriptor at the lane's minimum
      for (int d = 0; d < nd; ++d) {
        const int dist = hamming48(mine, gmem(M.old_desc) + 12 * ((size_t)db + d));
        if (dist < rb) { rb = dist; rd = d; }
      }
      // an earlier round's k is smaller: it keeps a tie on (distance, descriptor)
      if (rb < best || (rb == best && rb < M.best_init && rd < bestD)) { best = rb; bestD = rd; bestK = k; }
    }
  }
  const bool has = best < M.best_init;
  const int dmin = waveMinInt(has ? best : kNoDist);
  if (dmin >= M.best_init) {  // nothing replaced distMin (also: no image, K = 0, no descriptors)
    // :338 compares distMin itself: where its start is below the threshold, the untouched (kMin = 0,
    // distMin) of a pair that was walked is a match, as in the reference
    const bool start = M.start_matches && K > 0 && nd > 0;
    if (lane == 0) {
      gmemw(M.out_kp)[item] = start ? 0 : -1;
      gmemw(M.out_dist)[item] = start ? M.best_init : -1;
    }
    return;
  }
  const int dsc = waveMinInt(has && best == dmin ? bestD : 0x7fffffff);
  const int kmin = waveMinInt(has && best == dmin && bestD == dsc ? bestK : 0x7fffffff);
  if (lane == 0) {
    gmemw(M.out_kp)[item] = kmin;
    gmemw(M.out_dist)[item] = dmin;
  }
}

// ------------------------------------------------------------------------------------------ refine
constexpr int kRB = 128;  // a candidate has tens to a few hundred observations
constexpr int kSums = 28; // J^T J (21, upper triangle row by row) | J^T r (6) | cost
enum PlaceOp { kOpStop = 0, kOpLinearise = 1, kOpCandidate = 2 };

// Ceres' Corrector on one 2-row block with a 2x6 Jacobian (corrector.cc): r and J corrected in place,
// returns the cost rho(|r|^2) / 2. J may be nullptr.
__device__ __forceinline__ double placeCorrect(const PlaceRefineDev& R, double r[2], double* J) {
  const double sq = r[0] * r[0] + r[1] * r[1];
  if (R.loss_kind == OKVISGPU_LOSS_NONE) return 0.5 * sq;
  double rho[3];
  lossRho(okvisgpu_loss{R.loss_kind, 0, R.loss_a, R.loss_b}, sq, rho);
  const double sqrtRho1 = sqrt(rho[1]);
  double scale = sqrtRho1, alphaSq = 0.0;
  if (sq != 0.0 && rho[2] > 0.0) {  // the second-order correction
    const double D = 1.0 + 2.0 * sq * rho[2] / rho[1];
    const double alpha = 1.0 - sqrt(D);
    scale = sqrtRho1 / (1.0 - alpha);
    alphaSq = alpha / sq;
  }
  if (J) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      if (alphaSq == 0.0) {
        J[c] *= sqrtRho1;
        J[6 + c] *= sqrtRho1;
      } else {
        const double rtj = J[c] * r[0] + J[6 + c] * r[1];
        J[c] = sqrtRho1 * (J[c] - alphaSq * r[0] * rtj);
        J[6 + c] = sqrtRho1 * (J[6 + c] - alphaSq * r[1] * rtj);
      }
    }
  }
  r[0] *= scale;
  r[1] *= scale;
  return 0.5 * rho[0];
}

// observation o at `pose`: the weighted residual without the loss and its minimal pose Jacobian
__device__ __forceinline__ void placeObs(const PlaceRefineDev& R, int o, const double pose[7], double r[2],
                                         double Jp[12]) {
  const int c = gmem(R.obs_cam)[o];
  double crow[kCamDoubles], ex[7], L[4], m[2], hp[4];
#pragma unroll
  for (int i = 0; i < kCamDoubles; ++i) crow[i] = gmem(R.cam)[(size_t)kCamDoubles * c + i];
#pragma unroll
  for (int i = 0; i < 7; ++i) ex[i] = gmem(R.extr)[7 * (size_t)c + i];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    L[i] = gmem(R.obs_L)[4 * (size_t)o + i];
    hp[i] = gmem(R.obs_pt)[4 * (size_t)o + i];
  }
  m[0] = gmem(R.obs_kp)[2 * (size_t)o];
  m[1] = gmem(R.obs_kp)[2 * (size_t)o + 1];
  double A[6], p[3], Jl[6];
  reprojectA(loadCam(crow), pose, hp, ex, L, m, r, A, p);
  obsJacobians(A, p, hp[3], Jp, Jl);
}

// PoseManifold::Plus (PoseLocalParameterization.cpp:29-50)
__device__ __forceinline__ void placePosePlus(const double x[7], const double d[6], double out[7]) {
  const Q dq = deltaQ(d[3], d[4], d[5]);
  const Q q = qnormalize(qmul(dq, qnormalize(Q{x[3], x[4], x[5], x[6]})));
  out[0] = x[0] + d[0];
  out[1] = x[1] + d[1];
  out[2] = x[2] + d[2];
  out[3] = q.x; out[4] = q.y; out[5] = q.z; out[6] = q.w;
}

__device__ __forceinline__ int tri(int i, int j) {  // (i <= j) in the upper triangle stored row by row
  return i * 6 - i * (i - 1) / 2 + (j - i);
}

// (A + diag(d2)) y = g by a lower Cholesky factorisation, A [21] upper triangle; false if not positive
// definite or the solution is not finite
__device__ __forceinline__ bool placeSolve(const double A[21], const double d2[6], const double g[6], double y[6]) {
  double Lm[36];
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k <= i; ++k) {
      double s = A[tri(k, i)] + (i == k ? d2[i] : 0.0);
      for (int q = 0; q < k; ++q) s -= Lm[i * 6 + q] * Lm[k * 6 + q];
      if (i == k) {
        if (!(s > 0.0) || !isfinite(s)) return false;
        Lm[i * 6 + i] = sqrt(s);
      } else {
        Lm[i * 6 + k] = s / Lm[k * 6 + k];
      }
    }
  double z[6];
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
    for (int q = 0; q < i; ++q) s -= Lm[i * 6 + q] * z[q];
    z[i] = s / Lm[i * 6 + i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = z[i];
    for (int q = i + 1; q < 6; ++q) s -= Lm[q * 6 + i] * y[q];
    y[i] = s / Lm[i * 6 + i];
  }
  bool ok = true;
  for (int i = 0; i < 6; ++i) ok = ok && isfinite(y[i]);
  return ok;
}

// lane 0's state of TrustRegionMinimizer + LevenbergMarquardtStrategy (Solver::Options defaults)
struct PlaceState {
  double x[7], cand[7], best[7];
  double jscale[6], H[21], g[6], diag[6];  // H, g of the Jacobi-scaled Jacobian
  double x_cost, cand_cost, min_cost, x_norm, gmax, mcc, rel;
  double radius, decrease;
  int iteration, succ, unsucc, invalid, termination;
  bool reuse, step_successful;
};

// FinalizeIterationAndCheckIfMinimizerCanContinue, then steps until one is valid: the next operation
__device__ int placeNextStep(const PlaceRefineDev& R, PlaceState& S) {
  for (;;) {
    if (S.step_successful) {
      ++S.succ;
      if (S.x_cost < S.min_cost) {
        S.min_cost = S.x_cost;
        for (int i = 0; i < 7; ++i) S.best[i] = S.x[i];
      }
    } else {
      ++S.unsucc;
    }
    if (S.iteration >= R.max_iter) { S.termination = OKVISGPU_NO_CONVERGENCE; return kOpStop; }
    if (S.gmax <= 1e-10) { S.termination = OKVISGPU_CONVERGENCE; return kOpStop; }
    if (S.radius <= 1e-32) { S.termination = OKVISGPU_CONVERGENCE; return kOpStop; }
    ++S.iteration;
    S.step_successful = false;
    // LevenbergMarquardtStrategy::ComputeStep
    if (!S.reuse)
      for (int i = 0; i < 6; ++i) S.diag[i] = fmin(fmax(S.H[tri(i, i)], 1e-6), 1e32);
    S.reuse = true;
    double d2[6], y[6], step[6];
    for (int i = 0; i < 6; ++i) d2[i] = S.diag[i] / S.radius;
    bool valid = placeSolve(S.H, d2, S.g, y);
    if (valid) {
      // model_cost_change = -(J step) . (r + J step / 2) = -(step . g + step^T H step / 2)
      double sg = 0.0, shs = 0.0;
      for (int i = 0; i < 6; ++i) {
        step[i] = -y[i];
        sg += step[i] * S.g[i];
      }
      for (int i = 0; i < 6; ++i) {
        double row = 0.0;
        for (int k = 0; k < 6; ++k) row += S.H[i <= k ? tri(i, k) : tri(k, i)] * step[k];
        shs += step[i] * row;
      }
      S.mcc = -(sg + 0.5 * shs);
      valid = S.mcc > 0.0;
    }
    if (!valid) {  // HandleInvalidStep; StepIsInvalid = StepRejected(0)
      if (++S.invalid >= 5) {
        S.termination = OKVISGPU_FAILURE;
        --S.iteration;
        return kOpStop;
      }
      S.radius /= S.decrease;
      S.decrease *= 2.0;
      S.reuse = true;
      continue;
    }
    S.invalid = 0;
    double delta[6];
    for (int i = 0; i < 6; ++i) delta[i] = step[i] * S.jscale[i];
    placePosePlus(S.x, delta, S.cand);
    return kOpCandidate;
  }
}

__global__ __launch_bounds__(kRB) void k_place_refine(const PlaceRefineDev R) {
  __shared__ double sh[kSums * kRB];
  __shared__ double c_pose[7];  // the point the workgroup evaluates next ...
  __shared__ int c_op;          // ... and what it evaluates there (PlaceOp)
  const int j = blockIdx.x, t = threadIdx.x;
  const int b = gmem(R.obs_begin)[j], e = gmem(R.obs_begin)[j + 1];
  gwptr<double> outR = gmemw(R.out_real) + (size_t)kPlaceReal * j;
  gwptr<int32_t> outI = gmemw(R.out_int) + (size_t)kPlaceInt * j;
  if (b == e) {  // no residuals: cost 0, gradient 0, converged at iteration 0
    if (t < kPlaceReal) outR[t] = 0.0;
    if (t == 0) {
      outI[0] = 0; outI[1] = 1; outI[2] = 0; outI[3] = OKVISGPU_CONVERGENCE; outI[4] = 0;
    }
    return;
  }
  PlaceState S;  // lane 0's
  bool first = true;
  double initial_cost = 0.0;
  if (t == 0) {
    for (int i = 0; i < 7; ++i) S.x[i] = c_pose[i] = gmem(R.pose)[7 * (size_t)j + i];
    c_op = kOpLinearise;
    S.min_cost = DBL_MAX;
    S.radius = 1e4;
    S.decrease = 2.0;
    S.iteration = S.succ = S.unsucc = S.invalid = 0;
    S.termination = OKVISGPU_NO_CONVERGENCE;
    S.reuse = false;
    S.step_successful = true;
    S.x_cost = 0.0;
  }
  ldsBarrier();
  for (;;) {
    const int op = c_op;
    double pose[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) pose[i] = c_pose[i];
    ldsBarrier();  // (every lane has read the control block before lane 0 rewrites it)
    if (op == kOpStop) break;
    if (op == kOpLinearise) {
      double v[kSums];
#pragma unroll
      for (int i = 0; i < kSums; ++i) v[i] = 0.0;
      for (int o = b + t; o < e; o += kRB) {
        double r[2], J[12];
        placeObs(R, o, pose, r, J);
        v[27] += placeCorrect(R, r, J);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int k = i; k < 6; ++k) v[i * 6 - i * (i - 1) / 2 + (k - i)] += J[i] * J[k] + J[6 + i] * J[6 + k];
          v[21 + i] += J[i] * r[0] + J[6 + i] * r[1];
        }
      }
      blockSumN<kRB, kSums>(v, sh);
      if (t == 0) {  // EvaluateGradientAndJacobian's remainder at x = pose
        S.x_cost = v[27];
        bool finite = true;
        for (int i = 0; i < kSums; ++i) finite = finite && isfinite(v[i]);
        if (first) {
          initial_cost = S.x_cost;
          for (int i = 0; i < 6; ++i) S.jscale[i] = 1.0 / (1.0 + sqrt(v[tri(i, i)]));
        }
        if (first && !finite) {  // the initial evaluation failed: the solve ends there
          S.termination = OKVISGPU_FAILURE;
          S.succ = 1;
          c_op = kOpStop;
        } else {
          if (!first) {  // HandleSuccessfulStep: LevenbergMarquardtStrategy::StepAccepted(rel)
            const double q = 2.0 * S.rel - 1.0;
            S.radius = fmin(1e16, S.radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
            S.decrease = 2.0;
            S.reuse = false;
            S.step_successful = true;
          }
          double ng[6], proj[7];
          for (int i = 0; i < 6; ++i) {
            ng[i] = -v[21 + i];
            S.g[i] = v[21 + i] * S.jscale[i];
            for (int k = i; k < 6; ++k) S.H[tri(i, k)] = v[tri(i, k)] * S.jscale[i] * S.jscale[k];
          }
          placePosePlus(S.x, ng, proj);  // |x - Plus(x, -g)|_max
          double gm = 0.0, xn = 0.0;
          for (int i = 0; i < 7; ++i) {
            gm = fmax(gm, fabs(S.x[i] - proj[i]));
            xn += S.x[i] * S.x[i];
          }
          S.gmax = gm;
          S.x_norm = sqrt(xn);
          c_op = placeNextStep(R, S);
        }
        first = false;
      }
    } else {  // the candidate's cost
      double cost = 0.0;
      for (int o = b + t; o < e; o += kRB) {
        double r[2], J[12];
        placeObs(R, o, pose, r, J);
        cost += placeCorrect(R, r, nullptr);
      }
      cost = blockSum<kRB>(cost, sh);
      if (t == 0) {
        S.cand_cost = cost;
        double sn = 0.0;
        for (int i = 0; i < 7; ++i) sn += (S.x[i] - S.cand[i]) * (S.x[i] - S.cand[i]);
        sn = sqrt(sn);
        const double cost_change = S.x_cost - S.cand_cost;
        // (Ceres returns from both tolerance tests before the iteration is recorded: not counted)
        if (sn <= 1e-8 * (S.x_norm + 1e-8)) {
          S.termination = OKVISGPU_CONVERGENCE;
          --S.iteration;
          c_op = kOpStop;
        } else if (fabs(cost_change) <= 1e-6 * S.x_cost) {
          S.termination = OKVISGPU_CONVERGENCE;
          --S.iteration;
          c_op = kOpStop;
        } else {
          S.rel = S.cand_cost >= DBL_MAX ? -DBL_MAX : cost_change / S.mcc;
          if (S.rel > 1e-3) {  // the linearisation at the new point completes HandleSuccessfulStep
            for (int i = 0; i < 7; ++i) S.x[i] = S.cand[i];
            c_op = kOpLinearise;
          } else {  // HandleUnsuccessfulStep: StepRejected
            S.radius /= S.decrease;
            S.decrease *= 2.0;
            S.reuse = true;
            c_op = placeNextStep(R, S);
          }
        }
      }
    }
    if (t == 0) {
      if (c_op == kOpStop) {  // the solve's result: the lowest-cost accepted point
        const bool have = S.min_cost < DBL_MAX;
        for (int i = 0; i < 7; ++i) c_pose[i] = have ? S.best[i] : S.x[i];
      } else {
        for (int i = 0; i < 7; ++i) c_pose[i] = c_op == kOpCandidate ? S.cand[i] : S.x[i];
      }
    }
    ldsBarrier();
  }
  // :565-598 at the refined pose (c_pose): outliers |r| > 3 counted, inliers add J^T J to H
  double pose[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) pose[i] = c_pose[i];
  double h[22];
#pragma unroll
  for (int i = 0; i < 22; ++i) h[i] = 0.0;
  for (int o = b + t; o < e; o += kRB) {
    double r[2], J[12];
    placeObs(R, o, pose, r, J);
    if (sqrt(r[0] * r[0] + r[1] * r[1]) > 3.0) {
      h[21] += 1.0;
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = i; k < 6; ++k) h[i * 6 - i * (i - 1) / 2 + (k - i)] += J[i] * J[k] + J[6 + i] * J[6 + k];
    }
  }
  blockSumN<kRB, 22>(h, sh);
  if (t == 0) {
    const bool failed = S.termination == OKVISGPU_FAILURE && S.iteration == 0 && S.min_cost >= DBL_MAX;
    outR[0] = initial_cost;
    outR[1] = failed ? initial_cost : fmin(S.min_cost, S.x_cost);
    for (int i = 0; i < 6; ++i)
      for (int k = 0; k < 6; ++k) outR[2 + i * 6 + k] = h[i <= k ? tri(i, k) : tri(k, i)];
    outI[0] = S.iteration;
    outI[1] = S.succ;
    outI[2] = S.unsucc;
    outI[3] = S.termination;
    outI[4] = (int32_t)h[21];
    for (int i = 0; i < 7; ++i) gmemw(R.pose)[7 * (size_t)j + i] = pose[i];
  }
}

}  // namespace

void launch_place_match(const PlaceMatchDev& M, hipStream_t s) {
  const int64_t n = (int64_t)M.n_lm * M.n_cam;
  if (n <= 0) return;
  k_place_match<<<(unsigned)n, 64, 0, s>>>(M);
}

void launch_place_refine(const PlaceRefineDev& R, hipStream_t s) {
  if (R.n_jobs <= 0) return;
  k_place_refine<<<R.n_jobs, kRB, 0, s>>>(R);
}

}  // namespace okg
