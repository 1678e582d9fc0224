// kernels_landmarks.hip — the post-solve landmark pass: ViGraph::updateLandmarks
// (okvis_ceres/src/ViGraph.cpp:1762-1841) and ViGraph::areLandmarksInFrontOfCameras (:1621-1642)
// for every landmark of the batch in one launch.
//
// One lane per landmark. The observations of a landmark are contiguous and sorted by (pose,
// camera) on the device (the reference's KeypointIdentifier map order), so the lane walks its run
// [visit_obs_begin[lm_visit_begin[l]], visit_obs_begin[lm_visit_begin[l + 1]]) once: per observation
// the landmark in the camera frame, the unit ray dir_W, the behind flag, the in-front test and the
// norm of the weighted reprojection residual without loss (obsCore, the code k_eval_obs runs); kept
// rays (norm <= 2.5) are stored and summed. A second walk over the stored rays takes the deviations
// from the mean (two passes: the one-pass sum of squares cancels on far landmarks). No lane reads
// what another writes: the result does not depend on the schedule, there are no atomics, and the
// per-window counts are taken on the host from the flags.
#include <hip/hip_runtime.h>

#include "device_problem.hpp"
#include "launch.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

__global__ __launch_bounds__(64) void k_update_landmarks(const DevProblem* __restrict__ Pp, double* quality,
                                                         uint8_t* flags, double* obs_err, double* dirs) {
  const DevProblem& P = *Pp;
  const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (l >= P.n_lm) return;
  const int vb = min(max(gmem(P.lm_visit_begin)[l], 0), P.n_visit);
  const int ve = min(max(gmem(P.lm_visit_begin)[l + 1], vb), P.n_visit);
  const int ob = min(max(gmem(P.visit_obs_begin)[vb], 0), P.n_obs);
  const int oe = min(max(gmem(P.visit_obs_begin)[ve], ob), P.n_obs);
  double hp[4];
  {
    const auto hpp = gmem(P.lm[0] + 4 * (size_t)l);
    for (int k = 0; k < 4; ++k) hp[k] = hpp[k];
  }
  bool behind = false, notInFront = false, haveBest = false;
  double bestErr = 1.0e12, best[3] = {0.0, 0.0, 0.0};
  double sum[3] = {0.0, 0.0, 0.0};
  int kept = 0;
  for (int o = ob; o < oe; ++o) {
    const int op = gmem(P.obs_pose)[o], ci = gmem(P.obs_cam)[o];
    double err = 0.0;
    bool ok = op >= 0 && op < P.n_pose && ci >= 0 && ci < P.n_cam;
    int cpose = 0;
    if (ok) {
      cpose = gmem(P.cam_pose)[ci];
      ok = cpose >= 0 && cpose < P.n_pose;
    }
    if (!ok) {  // (never with a batch analyse() built; an observation that cannot be read is skipped)
      obs_err[o] = HUGE_VAL;
      continue;
    }
    double pose[7], ex[7], L[4], m[2];
    {
      const auto pp = gmem(P.pose[0] + 7 * (size_t)op);
      const auto ep = gmem(P.pose[0] + 7 * (size_t)cpose);  // T_SC: the camera's pose-kind block
      for (int k = 0; k < 7; ++k) {
        pose[k] = pp[k];
        ex[k] = ep[k];
      }
      const auto Lp = gmem(P.obs_L + 4 * (size_t)o);
      for (int k = 0; k < 4; ++k) L[k] = Lp[k];
      const auto mp = gmem(P.obs_kp + 2 * (size_t)o);
      m[0] = mp[0];
      m[1] = mp[1];
    }
    double C_WS[9], C_SC[9], C_WC[9];
    qrot(qnormalize(Q{pose[3], pose[4], pose[5], pose[6]}), C_WS);
    qrot(qnormalize(Q{ex[3], ex[4], ex[5], ex[6]}), C_SC);
    mm3(C_WS, C_SC, C_WC);
    // T_WC = T_WS T_SC; pos_C = T_WC^-1 hp_W = [C_CW hp.xyz - (C_CW r_WC) w, w]
    double r_WC[3], t[3], pos[3];
    mv3(C_WS, ex, r_WC);
    for (int k = 0; k < 3; ++k) r_WC[k] += pose[k];
    mtv3(C_WC, r_WC, t);
    mtv3(C_WC, hp, pos);
    double w = hp[3];
    for (int k = 0; k < 3; ++k) pos[k] -= t[k] * w;
    // areLandmarksInFrontOfCameras, on the undivided point
    if (pos[2] * w < 0.0) notInFront = true;
    if (fabs(w) > 1.0e-16 && pos[2] / w < 0.05) notInFront = true;
    if (fabs(w) > 1.0e-12) {
      for (int k = 0; k < 3; ++k) pos[k] /= w;
      w = 1.0;
    }
    double d[3];
    mv3(C_WC, pos, d);
    const double n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (n2 > 0.0) {  // (Eigen's normalized() leaves a zero vector as it is)
      const double n = sqrt(n2);
      for (int k = 0; k < 3; ++k) d[k] /= n;
    }
    if (pos[2] < 0.1) behind = true;
    if (pos[2] < 0.0)
      for (int k = 0; k < 3; ++k) d[k] = -d[k];

    {
      const auto cp = gmem(P.cam + kCamDoubles * (size_t)ci);
      const Cam cam = Cam{(int)cp[0], cp[1], cp[2], cp[3], cp[4], cp[5], cp[6], cp[7], cp[8], cp[9], cp[10], cp[11], cp[12]};
      double r[2], A[6], cost;
      obsCore(cam, L, m, pose, C_WS, hp, ex, false, false, r, A, cost);
      err = sqrt(r[0] * r[0] + r[1] * r[1]);
    }
    obs_err[o] = err;
    if (err > 2.5) continue;

    // the reference's norm of the 4-vector, w included ([x y z 1] after the division)
    const double n4 = sqrt(pos[0] * pos[0] + pos[1] * pos[1] + pos[2] * pos[2] + w * w);
    if (err < bestErr && n4 > 1.0e-4) {
      const double dist = fmax(0.1, n4);
      for (int k = 0; k < 3; ++k) best[k] = r_WC[k] + dist * d[k];
      bestErr = err;
      haveBest = true;
    }
    double* dk = dirs + 3 * (size_t)(ob + kept);  // kept rays, packed at the front of the landmark's run
    for (int k = 0; k < 3; ++k) {
      dk[k] = d[k];
      sum[k] += d[k];
    }
    ++kept;
  }

  double q = 0.0;
  if (kept > 0) {
    const double mean[3] = {sum[0] / kept, sum[1] / kept, sum[2] / kept};
    double dev[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < kept; ++i) {
      const double* dk = dirs + 3 * (size_t)(ob + i);
      for (int k = 0; k < 3; ++k) {
        const double e = dk[k] - mean[k];
        dev[k] += e * e;
      }
    }
    const double s0 = sqrt(dev[0]), s1 = sqrt(dev[1]), s2 = sqrt(dev[2]);
    q = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
  }
  uint8_t f = notInFront ? kLmNotInFront : 0;
  if (q > 0.04) {
    f |= kLmInitialised;
  } else if (kept > 0 && behind && haveBest) {
    f |= kLmReset;
    for (int x = 0; x < 2; ++x) {
      double* dst = P.lm[x] + 4 * (size_t)l;
      dst[0] = best[0];
      dst[1] = best[1];
      dst[2] = best[2];
      dst[3] = 1.0;
    }
  }
  quality[l] = q;
  flags[l] = f;
}

void launch_update_landmarks(const DevProblem& P, double* quality, uint8_t* flags, double* obs_err, double* dirs,
                             hipStream_t s) {
  if (P.n_lm > 0)
    hipLaunchKernelGGL(k_update_landmarks, dim3((P.n_lm + 63) / 64), dim3(64), 0, s, P.self, quality, flags, obs_err,
                       dirs);
}

}  // namespace okg
