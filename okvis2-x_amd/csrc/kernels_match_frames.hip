// kernels_match_frames.hip — the keypoint-against-keypoint BRISK matching of Frontend::matchMotionStereo's
// worker loop (Frontend.cpp:2057-2149, mode 0) and Frontend::matchStereo's inner loop (:2259-2316, mode 1)
// on gfx950: every side-0 keypoint of a job against every side-1 keypoint of the job.
//
//  k_match_frames_prepare  one lane per keypoint of either side: e_W = normalised(C_WC ray); side 0's lanes
//                          write the no-match value of every output, side 1's the flag use1 && ray_valid1.
//                          One lane per job: C_WC0, r_WC0, C_WC1, r_WC1 and the mean focal lengths, so the
//                          match kernel composes no transform.
//  k_match_frames<MODE>    one wavefront per participating side-0 keypoint (use0 && ray_valid0; the list is
//                          the runtime's), the descriptor in 12 registers, lanes over the side-1 keypoints
//                          in ascending order, 64 per round.
//
// The reference walks the side-1 keypoints serially and tests a candidate when its distance is below the
// best so far; whether a candidate is admissible (ray validity, the two angle tests, triangulateFast, the
// two depths) does not depend on that best. So the match is the first admissible side-1 keypoint attaining
// the minimum admissible distance below the threshold, and point, flag and quality are that candidate's.
// A round forms the 64 distances; the lanes below the best at the round's start evaluate the geometry (a
// superset of the candidates the serial walk would evaluate, with the same outcomes); the wave minimum over
// the admissible distances, first lane on a tie, replaces the best if it is strictly smaller. Mode 0's
// quality and projection check run once, on the winner; a winner failing the check leaves no match.
//
// In mode 1 a side-0 keypoint without a valid ray can have no admissible candidate, so it is left out of
// the list like one with use0 = 0. best's start is an integer: d < threshold iff d < ceil(threshold) (mode
// 1), d < (uint32_t)threshold (mode 0), both formed once by the runtime.
//
// No atomics, no communication between wavefronts; loop bounds are counts. A job's result depends on its
// own keypoints only and the reduction has a fixed shape: the same bits in every batch and on every run.
#include "launch.hpp"
#include "match_geometry.hpp"

namespace okg {

namespace {

__global__ __launch_bounds__(64) void k_match_frames_prepare(const FrameMatchDev F) {
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int64_t nk = (int64_t)F.n_kp0 + F.n_kp1;
  if (idx >= nk + F.n_jobs) return;
  if (idx >= nk) {  // a job's transforms
    const int j = (int)(idx - nk);
    gwptr<double> g = gmemw(F.job_geo) + (size_t)kFrameGeoDoubles * j;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      gptr<double> ps = gmem(side ? F.job_pose1 : F.job_pose0) + 7 * (size_t)j;
      gptr<double> es = gmem(side ? F.job_ext1 : F.job_ext0) + 7 * (size_t)j;
      double pose[7], ext[7], C[9], r[3];
#pragma unroll
      for (int i = 0; i < 7; ++i) { pose[i] = ps[i]; ext[i] = es[i]; }
      composeWC(pose, ext, C, r);
#pragma unroll
      for (int i = 0; i < 9; ++i) g[12 * side + i] = C[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) g[12 * side + 9 + i] = r[i];
      gptr<double> cr = gmem(F.cam) + (size_t)kMatchCamDoubles * gmem(side ? F.job_cam1 : F.job_cam0)[j];
      g[24 + side] = 0.5 * (cr[1] + cr[2]);
    }
    return;
  }
  const int side = idx >= F.n_kp0;
  const int k = (int)(side ? idx - F.n_kp0 : idx);
  const int j = gmem(side ? F.kp1_job : F.kp0_job)[k];
  gptr<double> ps = gmem(side ? F.job_pose1 : F.job_pose0) + 7 * (size_t)j;
  gptr<double> es = gmem(side ? F.job_ext1 : F.job_ext0) + 7 * (size_t)j;
  gptr<double> rs = gmem(side ? F.ray1 : F.ray0) + 3 * (size_t)k;
  double pose[7], ext[7], C[9], r[3];
#pragma unroll
  for (int i = 0; i < 7; ++i) { pose[i] = ps[i]; ext[i] = es[i]; }
  composeWC(pose, ext, C, r);
  const double ray[3] = {rs[0], rs[1], rs[2]};
  double cr[3], e[3];
  mv3(C, ray, cr);
  normalised3(cr, e);
  gwptr<double> eo = gmemw(side ? F.e1 : F.e0) + 3 * (size_t)k;
  eo[0] = e[0]; eo[1] = e[1]; eo[2] = e[2];
  if (side) {
    const bool use = F.use1 ? gmem(F.use1)[k] != 0 : true;
    gmemw(F.flag1)[k] = (uint8_t)(use && gmem(F.valid1)[k] != 0);
  } else {
    gmemw(F.out_match)[k] = -1;
    gmemw(F.out_dist)[k] = -1;
    gwptr<double> p = gmemw(F.out_point) + 4 * (size_t)k;
    p[0] = 0.0; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0;
    gmemw(F.out_quality)[k] = 0.0;
    gmemw(F.out_init)[k] = 0;
  }
}

template <int MODE>
__global__ __launch_bounds__(64) void k_match_frames(const FrameMatchDev F, int first, int count) {
  if ((int)blockIdx.x >= count) return;
  const int k0 = gmem(F.kp_list)[first + blockIdx.x];
  const int lane = threadIdx.x;
  const int j = gmem(F.kp0_job)[k0];
  const int b1 = gmem(F.kp1_begin)[j];
  const int n1 = gmem(F.kp1_begin)[j + 1] - b1;
  gptr<double> g = gmem(F.job_geo) + (size_t)kFrameGeoDoubles * j;
  // the third columns of C_WC0 and C_WC1 (the depths), the camera centres, the focal lengths
  const double z0[3] = {g[2], g[5], g[8]}, r0[3] = {g[9], g[10], g[11]};
  const double z1[3] = {g[14], g[17], g[20]}, r1[3] = {g[21], g[22], g[23]};
  const double f0 = g[24], f1 = g[25];
  uint32_t desc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) desc[i] = gmem(F.desc0)[12 * (size_t)k0 + i];
  const double e0[3] = {gmem(F.e0)[3 * (size_t)k0], gmem(F.e0)[3 * (size_t)k0 + 1], gmem(F.e0)[3 * (size_t)k0 + 2]};
  const double s0 = gmem(F.size0)[k0] / f0;
  const double minDepth = MODE == 0 ? 0.2 : 0.1;

  int best = F.best_init[MODE], match = -1;
  double point[3] = {0.0, 0.0, 0.0};
  int parallel = 0;
  for (int base = 0; base < n1; base += 64) {
    const int l = base + lane;
    const size_t k1 = (size_t)b1 + (l < n1 ? l : 0);  // a lane past the end reads the job's first row, unused
    bool live = l < n1 && gmem(F.flag1)[k1] != 0;
    const int ds = hamming48(desc, gmem(F.desc1) + 12 * k1);
    live = live && ds < best;
    if (!__any(live)) continue;
    int d = kNoDist;
    double pt[3] = {0.0, 0.0, 0.0};
    bool par = false;
    if (live) {
      const double e1[3] = {gmem(F.e1)[3 * k1], gmem(F.e1)[3 * k1 + 1], gmem(F.e1)[3 * k1 + 2]};
      const double c = dot3(e0, e1);
      if (MODE == 1 || !(c < 0.5)) {
        double sigma = s0 * 0.125;
        if (MODE == 1) {
          const double s1 = gmem(F.size1)[k1] / f1;
          sigma = (s0 < s1 ? s1 : s0) * 0.125;  // std::max
        }
        bool valid;
        triangulateFast(r0, e0, r1, e1, sigma, pt, valid, par);
        const double a[3] = {pt[0] - r0[0], pt[1] - r0[1], pt[2] - r0[2]};
        const double b[3] = {pt[0] - r1[0], pt[1] - r1[1], pt[2] - r1[2]};
        const double depth0 = z0[0] * a[0] + z0[1] * a[1] + z0[2] * a[2];
        const double depth1 = z1[0] * b[0] + z1[1] * b[1] + z1[2] * b[2];
        if (valid && !(c < 0.8) && !(depth0 < minDepth) && !(depth1 < minDepth)) d = ds;
      }
    }
    const int total = waveMinInt(d);
    if (total < best) {  // the first lane attaining the round's minimum
      const int src = __builtin_ctzll(__ballot(d == total));
      best = total;
      match = base + src;
      point[0] = __shfl(pt[0], src, 64);
      point[1] = __shfl(pt[1], src, 64);
      point[2] = __shfl(pt[2], src, 64);
      parallel = __shfl((int)par, src, 64);
    }
  }
  if (match < 0) return;  // the prepare kernel wrote the no-match values
  double quality = 0.0;
  if (MODE == 0) {
    const double a[3] = {point[0] - r0[0], point[1] - r0[1], point[2] - r0[2]};
    const double b[3] = {point[0] - r1[0], point[1] - r1[1], point[2] - r1[2]};
    double an[3], bn[3];
    normalised3(a, an);
    normalised3(b, bn);
    quality = acos(dot3(an, bn));
    // projectHomogeneous(camera1, T_WC1^-1 [p, 1]) Successful and within 4 px of keypoint1 (:2140-2147)
    double C1[9], pc[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) C1[i] = g[12 + i];
    mtv3(C1, b, pc);
    gptr<double> cr = gmem(F.cam) + (size_t)kMatchCamDoubles * gmem(F.job_cam1)[j];
    double crow[kCamDoubles];
#pragma unroll
    for (int i = 0; i < kCamDoubles; ++i) crow[i] = cr[i];
    const Cam cam = loadCam(crow);
    const double width = cr[13], height = cr[14];
    if (fabs(pc[2]) < 1.0e-12) return;  // Invalid
    const double rz = 1.0 / pc[2];
    const double u0 = pc[0] * rz, u1 = pc[1] * rz;
    if (cam.dist == 3 && u0 * u0 + u1 * u1 > 9.0) return;  // Invalid (RadialTangentialDistortion8.hpp:98)
    double d0, d1, Jd[4];
    distort(cam, u0, u1, d0, d1, Jd, false);
    const double px = cam.fu * d0 + cam.cu, py = cam.fv * d1 + cam.cv;
    const bool inImage = !(px < 0.0 || py < 0.0) && !(px >= width || py >= height);
    if (!inImage || !(pc[2] > 0.0)) return;  // OutsideImage, Behind
    const size_t km = (size_t)b1 + match;
    const double dx = gmem(F.xy1)[2 * km] - px, dy = gmem(F.xy1)[2 * km + 1] - py;
    if (!(sqrt(dx * dx + dy * dy) < 4.0)) return;
  }
  if (lane == 0) {
    gmemw(F.out_match)[k0] = match;
    gmemw(F.out_dist)[k0] = best;
    gwptr<double> p = gmemw(F.out_point) + 4 * (size_t)k0;
    p[0] = point[0]; p[1] = point[1]; p[2] = point[2]; p[3] = 1.0;
    gmemw(F.out_quality)[k0] = quality;
    gmemw(F.out_init)[k0] = (uint8_t)(parallel ? 0 : 1);
  }
}

}  // namespace

void launch_match_frames_prepare(const FrameMatchDev& F, hipStream_t s) {
  const int64_t n = (int64_t)F.n_kp0 + F.n_kp1 + F.n_jobs;
  if (n <= 0) return;
  k_match_frames_prepare<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(F);
}

void launch_match_frames(const FrameMatchDev& F, hipStream_t s) {
  // kp_list holds the participating side-0 keypoints of the mode-0 jobs first, then the mode-1 jobs'
  if (F.n_list0 > 0) k_match_frames<0><<<F.n_list0, 64, 0, s>>>(F, 0, F.n_list0);
  if (F.n_list1 > 0) k_match_frames<1><<<F.n_list1, 64, 0, s>>>(F, F.n_list0, F.n_list1);
}

}  // namespace okg
