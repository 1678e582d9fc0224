// kernels_match.hip — Frontend::matchToMap (Frontend.cpp:1299-1956) on gfx950: BRISK matching of the
// keypoints of a new frame against up to three descriptors of every landmark of the window.
//
//  k_match_prepare   one lane per (job, landmark): the candidate preparation of :1335-1508. FoV check
//                    with projectHomogeneous and its status logic, the 3D test, and the three best-scored
//                    observations (newest first) with their descriptor, ray e0_W and camera centre r0_W.
//  k_match<PASS>     one wavefront per keypoint, lanes over the landmarks in ascending order, 64 per
//                    round. PASS 0 is matchToMapByThread (:1745-1827, 3D candidates, projection gate
//                    before any popcount), PASS 1 matchToMapByThreadUnitialised (:1831-1956, the other
//                    candidates, epipolar test and triangulateFast, stereo_triangulation.cpp:30-112).
//
// The reference walks the candidates of a keypoint serially and records a candidate when its distance
// is below the best so far; whether a candidate is admissible (gate, epipolar test, triangulation)
// does not depend on that best. So the records are the strict prefix minima of the admissible
// distances in (landmark, slot) order, and the match is the first candidate attaining the minimum. A
// round computes the admissible distances of 64 landmarks, an exclusive prefix minimum over the lanes
// gives every lane the best before its landmark, and the lane walks its own slots from there: record
// count, reprojection sum and pass 1's last non-parallel point come out as in the serial walk.
// Geometry is evaluated for the slots below the best at the round's start: a superset of the slots the
// serial walk would evaluate, and their outcome is the same.
//
// A job's result depends on its own keypoints and the shared map only; the reductions have a fixed
// shape, so a result is the same bits in every batch and on every run.
#include "launch.hpp"
#include "match_geometry.hpp"

namespace okg {

namespace {

// reprThreshold = 3 + f (imu ? 0.06 : 0.34), f the mean focal length (:1340-1342)
__device__ __forceinline__ double reprThreshold(const Cam& c, int imu_use) {
  const double f = 0.5 * (c.fu + c.fv);
  return imu_use ? 3.0 + f * 0.06 : 3.0 + f * 0.34;
}
__global__ __launch_bounds__(64) void k_match_prepare(const MatchDev M) {
  const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (int64_t)M.n_jobs * M.n_lm) return;
  const int j = (int)(idx / M.n_lm), l = (int)(idx % M.n_lm);
  int n = -1, is3d = 0;
  int slotObs[3] = {-1, -1, -1};
  double proj[2] = {0.0, 0.0};
  auto finish = [&]() {
    gmemw(M.cand_n)[idx] = n;
    gmemw(M.cand_is3d)[idx] = (uint8_t)(n > 0 ? is3d : 0);
    gmemw(M.cand_obs)[3 * idx + 0] = n > 0 ? slotObs[0] : -1;
    gmemw(M.cand_obs)[3 * idx + 1] = n > 0 ? slotObs[1] : -1;
    gmemw(M.cand_obs)[3 * idx + 2] = n > 0 ? slotObs[2] : -1;
    gmemw(M.cand_proj)[2 * idx + 0] = n > 0 ? proj[0] : 0.0;
    gmemw(M.cand_proj)[2 * idx + 1] = n > 0 ? proj[1] : 0.0;
  };
  if (M.lm_use && !gmem(M.lm_use)[l]) return finish();

  const int camIdx = gmem(M.job_cam)[j];
  gptr<double> cr = gmem(M.cam) + (size_t)kMatchCamDoubles * camIdx;
  double crow[kCamDoubles];
#pragma unroll
  for (int i = 0; i < kCamDoubles; ++i) crow[i] = cr[i];
  const Cam cam = loadCam(crow);
  const double width = cr[13], height = cr[14];
  const double thr = reprThreshold(cam, M.imu_use);
  const double focalLength = cam.fu + cam.fv;  // the sum (:1359-1361)

  double pose[7], ext[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    pose[i] = gmem(M.job_pose_prepare)[7 * (size_t)j + i];
    ext[i] = gmem(M.extr)[7 * (size_t)camIdx + i];
  }
  double C1[9], r1[3];
  composeWC(pose, ext, C1, r1);
  const double hp[4] = {gmem(M.lm)[4 * (size_t)l], gmem(M.lm)[4 * (size_t)l + 1], gmem(M.lm)[4 * (size_t)l + 2],
                        gmem(M.lm)[4 * (size_t)l + 3]};
  const double p_W[3] = {hp[0] / hp[3], hp[1] / hp[3], hp[2] / hp[3]};
  const double r_W[3] = {p_W[0] - r1[0], p_W[1] - r1[1], p_W[2] - r1[2]};
  double e_W[3];
  normalised3(r_W, e_W);
  const double r = fmax(0.01, sqrt(dot3(r_W, r_W)));

  // hp_C = T_CW1 hp_W; projectHomogeneous and project's status (PinholeCamera.hpp:249-284, 485-494)
  {
    const double d[3] = {hp[0] - r1[0] * hp[3], hp[1] - r1[1] * hp[3], hp[2] - r1[2] * hp[3]};
    double pc[3];
    mtv3(C1, d, pc);
    if (hp[3] < 0) { pc[0] = -pc[0]; pc[1] = -pc[1]; pc[2] = -pc[2]; }
    if (fabs(pc[2]) < 1.0e-12) return finish();  // Invalid
    const double rz = 1.0 / pc[2];
    const double u0 = pc[0] * rz, u1 = pc[1] * rz;
    if (cam.dist == 3 && u0 * u0 + u1 * u1 > 9.0) return finish();  // Invalid (RadialTangentialDistortion8.hpp:98)
    double d0, d1, Jd[4];
    distort(cam, u0, u1, d0, d1, Jd, false);
    proj[0] = cam.fu * d0 + cam.cu;
    proj[1] = cam.fv * d1 + cam.cv;
    const bool inImage = !(proj[0] < 0.0 || proj[1] < 0.0) && !(proj[0] >= width || proj[1] >= height);
    if (inImage && !(pc[2] > 0.0)) return finish();  // Behind
    if (proj[0] < -thr || proj[1] < -thr || proj[0] > width + thr || proj[1] > height + thr) return finish();
  }

  const double quality = gmem(M.lm_quality)[l];
  const double cos10 = cos(10.0 / focalLength), cos06 = cos(0.6);
  const double closeScale = 0.2 / focalLength / quality;
  double rWn[3];
  normalised3(r_W, rWn);
  double best[3] = {1.0, 1.0, 1.0};
  int used = 0;
  const int o0 = gmem(M.obs_begin)[l], o1 = gmem(M.obs_begin)[l + 1];
  for (int o = o1 - 1; o >= o0; --o) {  // rbegin() .. rend()
    const int op = gmem(M.obs_pose)[o], oc = gmem(M.obs_cam)[o];
    double po[7], eo[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      po[i] = gmem(M.poses)[7 * (size_t)op + i];
      eo[i] = gmem(M.extr)[7 * (size_t)oc + i];
    }
    double Co[9], ro[3];
    composeWC(po, eo, Co, ro);
    const double r_old[3] = {p_W[0] - ro[0], p_W[1] - ro[1], p_W[2] - ro[2]};
    if (!is3d) {
      const double rc[3] = {r_W[0] - closeScale * r_old[0], r_W[1] - closeScale * r_old[1],
                            r_W[2] - closeScale * r_old[2]};
      double rcn[3];
      normalised3(rc, rcn);
      if (dot3(rWn, rcn) > cos10) is3d = 1;
    }
    double ron[3];
    normalised3(r_old, ron);
    const double cosV = dot3(e_W, ron);
    if (cosV < cos06 && !M.loop_closure) continue;
    const double scaleChange = fabs(r - sqrt(dot3(r_old, r_old))) / r;
    if (scaleChange > 0.5 && !M.loop_closure) continue;
    const double score = 0.5 * (acos(cosV) / 0.6 + scaleChange / 0.5);
    double worst = 0.0;
    int wi = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s)
      if (best[s] > worst) { worst = best[s]; wi = s; }
    const double cur = wi == 0 ? best[0] : wi == 1 ? best[1] : best[2];
    if (score < cur) {
      if (wi == 0) { best[0] = score; slotObs[0] = o; }
      else if (wi == 1) { best[1] = score; slotObs[1] = o; }
      else { best[2] = score; slotObs[2] = o; }
      used = max(used, wi + 1);
      double en[3], e0[3];
      const double ray[3] = {gmem(M.obs_ray)[3 * (size_t)o], gmem(M.obs_ray)[3 * (size_t)o + 1],
                             gmem(M.obs_ray)[3 * (size_t)o + 2]};
      normalised3(ray, en);
      mv3(Co, en, e0);
      gwptr<double> g = gmemw(M.cand_geo) + 6 * (3 * (size_t)idx + wi);
      g[0] = e0[0]; g[1] = e0[1]; g[2] = e0[2];
      g[3] = ro[0]; g[4] = ro[1]; g[5] = ro[2];
      gptr<uint32_t> src = gmem(M.obs_desc) + 12 * (size_t)o;
      gwptr<uint32_t> dst = gmemw(M.cand_desc) + 12 * (3 * (size_t)idx + wi);
#pragma unroll
      for (int i = 0; i < 12; ++i) dst[i] = src[i];
    }
  }
  n = used > 0 ? used : -1;  // no kept observation: left out (the reference keeps one row of pool memory)
  finish();
}

// exclusive prefix minimum over the wavefront's lanes (kNoDist for lane 0); *total = the minimum of all
__device__ __forceinline__ int exclusiveMin(int v, int lane, int* total) {
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl = min(incl, t);
  }
  *total = __shfl(incl, 63, 64);
  const int e = __shfl_up(incl, 1, 64);
  return lane == 0 ? kNoDist : e;
}
__device__ __forceinline__ int waveSumInt(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double waveSumDouble(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// pass 1's tests of one slot (:1903-1939): true when the candidate is admissible
__device__ __forceinline__ bool admissible1(const double e0[3], const double r0[3], const double r1[3],
                                            const double e1[3], double sigma, double cos6, double pt[3],
                                            bool& parallel) {
  if (dot3(e0, e1) < cos6) {
    const double t[3] = {r1[0] - r0[0], r1[1] - r0[1], r1[2] - r0[2]};
    double et[3], c0[3], c1[3], n0[3], n1[3];
    normalised3(t, et);
    cross3(e0, et, c0);
    cross3(e1, et, c1);
    normalised3(c0, n0);
    normalised3(c1, n1);
    if (dot3(n0, n1) < cos6) return false;  // not in the epipolar plane
    const double nn[3] = {n0[0] + n0[0], n0[1] + n0[1], n0[2] + n0[2]};  // n0 twice, as written (:1914)
    double nnn[3], c01[3];
    normalised3(nn, nnn);
    cross3(e0, e1, c01);
    if (dot3(c01, nnn) > 0.0) return false;  // divergent rays
  }
  bool valid;
  triangulateFast(r0, e0, r1, e1, sigma, pt, valid, parallel);
  if (!valid) return false;
  const double a[3] = {pt[0] - r0[0], pt[1] - r0[1], pt[2] - r0[2]};
  const double b[3] = {pt[0] - r1[0], pt[1] - r1[1], pt[2] - r1[2]};
  if (sqrt(dot3(a, a)) < 0.2 || sqrt(dot3(b, b)) < 0.2) return false;  // out of focus
  return true;
}

template <int PASS>
__global__ __launch_bounds__(64) void k_match(const MatchDev M, int first, int count) {
  if ((int)blockIdx.x >= count) return;
  const int k = gmem(M.kp_list)[first + blockIdx.x];
  const int lane = threadIdx.x;
  const int j = gmem(M.kp_job)[k];
  const int carried = gmem(M.kp_lm)[k];
  bool use = !(carried >= 0 && !M.loop_closure);
  if (PASS == 1) use = use && gmem(M.kp_ray_valid)[k] != 0;
  int best = kNoDist, match = -1, records = 0;
  double sum = 0.0, point[3] = {0.0, 0.0, 0.0};
  bool havePoint = false;
  if (use) {
    const int camIdx = gmem(M.job_cam)[j];
    gptr<double> cr = gmem(M.cam) + (size_t)kMatchCamDoubles * camIdx;
    const double f = 0.5 * (cr[1] + cr[2]);
    const double thr = M.imu_use ? 3.0 + f * 0.06 : 3.0 + f * 0.34;
    const double thr2 = thr * thr;
    const double kx = gmem(M.kp_xy)[2 * (size_t)k], ky = gmem(M.kp_xy)[2 * (size_t)k + 1];
    uint32_t desc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) desc[i] = gmem(M.kp_desc)[12 * (size_t)k + i];
    // pass 1: T_WC1 at pose_match, the keypoint's ray in W, sigma = 1 / f (:1842-1874)
    double r1[3] = {0, 0, 0}, e1[3] = {0, 0, 0}, sigma = 0.0, cos6 = 0.0;
    if (PASS == 1) {
      double pose[7], ext[7], C1[9], en[3];
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        pose[i] = gmem(M.job_pose_match)[7 * (size_t)j + i];
        ext[i] = gmem(M.extr)[7 * (size_t)camIdx + i];
      }
      composeWC(pose, ext, C1, r1);
      const double ray[3] = {gmem(M.kp_ray)[3 * (size_t)k], gmem(M.kp_ray)[3 * (size_t)k + 1],
                             gmem(M.kp_ray)[3 * (size_t)k + 2]};
      normalised3(ray, en);
      mv3(C1, en, e1);
      sigma = 1.0 / f;
      cos6 = cos(6.0 * sigma);
    }
    const size_t jl = (size_t)j * M.n_lm;
    for (int base = 0; base < M.n_lm; base += 64) {
      const int l = base + lane;
      // the landmark's table row, loaded whole (every row is written, zero for a non-candidate): the
      // three loads are independent, so a round waits for memory once
      int n = -1;
      bool is3d = false;
      double px = 0.0, py = 0.0;
      if (l < M.n_lm) {
        n = gmem(M.cand_n)[jl + l];
        is3d = gmem(M.cand_is3d)[jl + l] != 0;
        if (PASS == 0) {
          px = gmem(M.cand_proj)[2 * (jl + l)];
          py = gmem(M.cand_proj)[2 * (jl + l) + 1];
        }
      }
      bool act = n > 0 && is3d == (PASS == 0);
      double rd2 = 0.0;
      if (PASS == 0) {  // the projection gate, before any popcount (:1807-1810)
        const double dx = px - kx, dy = py - ky;
        rd2 = dx * dx + dy * dy;
        act = act && !(rd2 > thr2);
      }
      if (!__any(act)) continue;
      // admissible distances of the lane's slots (kNoDist: none); dist < best as doubles, best
      // starting at the matching threshold
      int d[3] = {kNoDist, kNoDist, kNoDist};
      bool par[3] = {false, false, false};
      double pt[9];
      if (act) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          if (s >= n) continue;
          const int ds = hamming48(desc, gmem(M.cand_desc) + 12 * (3 * (jl + l) + s));
          if (!((double)ds < M.threshold) || !(ds < best)) continue;
          if (PASS == 1) {
            gptr<double> g = gmem(M.cand_geo) + 6 * (3 * (jl + l) + s);
            const double e0[3] = {g[0], g[1], g[2]}, r0[3] = {g[3], g[4], g[5]};
            if (!admissible1(e0, r0, r1, e1, sigma, cos6, &pt[3 * s], par[s])) continue;
          }
          d[s] = ds;
        }
      }
      const bool isCarried = PASS == 1 && act && l == carried;
      const int laneMin = isCarried ? kNoDist : min(d[0], min(d[1], d[2]));
      int total;
      int b = min(best, exclusiveMin(laneMin, lane, &total));
      int rec = 0;
      bool lanePoint = false;
      double lp[3] = {0.0, 0.0, 0.0};
      if (isCarried) {
        // the landmark the keypoint already carries: counts once, changes nothing (:1941-1944)
        rec = (d[0] < b || d[1] < b || d[2] < b) ? 1 : 0;
      } else {
#pragma unroll
        for (int s = 0; s < 3; ++s)
          if (d[s] < b) {
            b = d[s];
            ++rec;
            if (PASS == 1 && !par[s]) {
              lanePoint = true;
              lp[0] = pt[3 * s]; lp[1] = pt[3 * s + 1]; lp[2] = pt[3 * s + 2];
            }
          }
      }
      records += waveSumInt(rec);
      if (PASS == 0) sum += waveSumDouble(rec ? (double)rec * sqrt(rd2) : 0.0);
      if (PASS == 1) {
        const unsigned long long pm = __ballot(lanePoint);
        if (pm) {  // the last non-parallel record in order
          const int src = 63 - __builtin_clzll(pm);
          point[0] = __shfl(lp[0], src, 64);
          point[1] = __shfl(lp[1], src, 64);
          point[2] = __shfl(lp[2], src, 64);
          havePoint = true;
        }
      }
      if (total < best) {  // the first lane attaining the round's minimum
        const unsigned long long mm = __ballot(laneMin == total);
        match = base + __builtin_ctzll(mm);
        best = total;
      }
    }
  }
  if (lane == 0) {
    gmemw(M.out_match)[k] = match;
    gmemw(M.out_dist)[k] = match >= 0 ? best : -1;
    gmemw(M.out_records)[k] = records;
    gmemw(M.out_sum)[k] = PASS == 0 ? sum : 0.0;
    gwptr<double> p = gmemw(M.out_point) + 4 * (size_t)k;
    p[0] = point[0]; p[1] = point[1]; p[2] = point[2];
    p[3] = havePoint ? 1.0 : 0.0;
  }
}

}  // namespace

void launch_match_prepare(const MatchDev& M, hipStream_t s) {
  const int64_t n = (int64_t)M.n_jobs * M.n_lm;
  if (n <= 0) return;
  k_match_prepare<<<(unsigned)((n + 63) / 64), 64, 0, s>>>(M);
}

void launch_match(const MatchDev& M, hipStream_t s) {
  // kp_list holds the keypoints of the pass-0 jobs first, then those of the pass-1 jobs
  if (M.n_kp0 > 0) k_match<0><<<M.n_kp0, 64, 0, s>>>(M, 0, M.n_kp0);
  if (M.n_kp1 > 0) k_match<1><<<M.n_kp1, 64, 0, s>>>(M, M.n_kp0, M.n_kp1);
}

}  // namespace okg
