// batch_calls.cpp — the call-scoped batch entry points of the okvisgpu C ABI: each takes a batch of
// independent items in the caller's arrays, runs a few kernels over it and returns the results;
// nothing of the resident problem (okvisgpu_set_problems) is read or written.
//
// Every call has the same shape: validate, declare each array once in a BatchLayout
// (batch_stage.hpp) against the field of the kernels' descriptor that points to it,
// c->beginBatch (sizes the context's pinned stage and batchScratch, patches the descriptor, stages
// the inputs), fill what the host computes itself through S.host(), c->uploadBatch (one copy up),
// launch, c->finishBatch (one copy down, the synchronise, outputs to the caller's arrays).
// batchScratch is shared by all of them and by the two batch-wide calls of resident_calls.cpp, so
// an array holds stale bytes of other calls until a kernel writes it: no kernel may read a scratch
// or output array it has not written.
#include "runtime.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "launch.hpp"
#include "loss.hpp"
#include "mat3_spd.hpp"

using namespace okg;

namespace {

// A CSR begin array of n items: begin[0] == 0 and begin[i + 1] >= begin[i]. `who` is the call's
// prefix; with an item noun the message names the first offending item.
void checkCsr(const int32_t* begin, size_t n, const char* name, const char* item, const std::string& who) {
  if (begin[0] != 0) throw ArgError{who + name + " must start at 0"};
  for (size_t i = 0; i < n; ++i)
    if (begin[i + 1] < begin[i])
      throw ArgError{who + name + " not monotone" + (item ? " at " + std::string(item) + " " + std::to_string(i) : "")};
}

// Item i's IMU samples cover its interval: there are some, the first is not after t_begin and, with
// t_end given, the last is not before it (the assertions of ImuError.cpp:550, ViGraph.cpp:976-982
// with GpsErrorAsynchronous.cpp:311-313, and LidarMotionUndistortion.cpp:34). `who` and `item` as
// for checkCsr; nameBegin / nameEnd are the call's names of the two stamps.
void checkCovered(const int32_t* begin, const int64_t* ts, size_t i, const char* nameBegin, int64_t t_begin,
                  const char* nameEnd, const int64_t* t_end, const char* item, const std::string& who) {
  const std::string it = who + item + " " + std::to_string(i);
  const int32_t s0 = begin[i], s1 = begin[i + 1];
  if (s1 == s0) throw ArgError{it + " has no samples"};
  if (ts[s0] > t_begin)
    throw ArgError{it + ": first sample " + std::to_string(ts[s0]) + " !<= " + nameBegin + " " + std::to_string(t_begin)};
  if (t_end && ts[s1 - 1] < *t_end)
    throw ArgError{it + ": last sample " + std::to_string(ts[s1 - 1]) + " !>= " + nameEnd + " " + std::to_string(*t_end)};
}

// The caller's cameras as rows of `doubles` values: kCamDoubles (distortion model, fu, fv, cu, cv,
// eight coefficients) or kMatchCamDoubles (the same, then width and height).
std::vector<double> packCameras(const okvisgpu_camera* cams, size_t n, int doubles, const std::string& who,
                                bool nameCamera = true) {
  std::vector<double> cam((size_t)doubles * n);
  for (size_t k = 0; k < n; ++k) {
    const okvisgpu_camera& q = cams[k];
    if (q.distortion < 0 || q.distortion > 3)
      throw ArgError{who + "unknown distortion model" + (nameCamera ? " of camera " + std::to_string(k) : "")};
    const double cv[kMatchCamDoubles] = {(double)q.distortion, q.fu, q.fv, q.cu, q.cv, q.dist[0], q.dist[1], q.dist[2],
                                         q.dist[3], q.dist[4], q.dist[5], q.dist[6], q.dist[7], (double)q.width,
                                         (double)q.height};
    std::memcpy(&cam[(size_t)doubles * k], cv, sizeof(double) * (size_t)doubles);
  }
  return cam;
}

void imuParams(const okvisgpu_imu_params& ip, double* par) {
  const double v[7] = {ip.a_max, ip.g_max, ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c, ip.g};
  std::memcpy(par, v, sizeof(v));
}

// the begin array of a CSR without items: its one element
const int32_t kEmptyCsr[1] = {0};

// The inputs of an okvisgpu_twopose_edges batch (okvisgpu_twopose_compute and
// okvisgpu_twopose_extrinsics_compute), checked and declared into S against T's fields; the caller
// declares its outputs after them. What is packed here lives in I until the batch has begun.
// Throws ArgError with `who` in front.
struct TwoPoseInputs {
  std::vector<double> cam;
  std::vector<uint8_t> cauchy;
  size_t nl = 0, no = 0;
};
void declareTwoPose(const okvisgpu_twopose_edges* E, const std::string& who, BatchLayout& S, TwoPoseDev& T,
                    TwoPoseInputs& I) {
  const size_t ne = (size_t)E->n_edges, nc = (size_t)std::max(0, E->n_cameras);
  checkCsr(E->landmark_begin, ne, "landmark_begin", nullptr, who);
  const size_t nl = (size_t)E->landmark_begin[ne];
  if (nl) checkCsr(E->obs_begin, nl, "obs_begin", nullptr, who);
  const size_t no = nl ? (size_t)E->obs_begin[nl] : 0;
  if (no && (!E->landmarks || !E->obs_other || !E->obs_camera || !E->obs_keypoint || !E->obs_sqrt_info ||
             !E->cameras || !E->extrinsics))
    throw ArgError{who + "observation arrays missing"};
  for (size_t o = 0; o < no; ++o)
    if (E->obs_camera[o] < 0 || E->obs_camera[o] >= E->n_cameras) throw ArgError{who + "obs_camera out of range"};
  I.cam = packCameras(E->cameras, E->cameras ? nc : 0, kCamDoubles, who, false);
  I.cauchy.assign(no, 1);
  if (E->obs_cauchy) for (size_t o = 0; o < no; ++o) I.cauchy[o] = E->obs_cauchy[o] ? 1 : 0;
  I.nl = nl;
  I.no = no;
  T.n_edges = E->n_edges;
  T.n_cam = E->n_cameras;
  S.in(T.ref_pose, E->ref_pose, 7 * ne);
  S.in(T.other_pose, E->other_pose, 7 * ne);
  S.in(T.cam, I.cam.data(), I.cam.size());
  S.in(T.extr, E->extrinsics, 7 * nc);
  S.in(T.lm_begin, E->landmark_begin, ne + 1);
  S.in(T.lm, E->landmarks, 4 * nl);
  S.in(T.obs_begin, nl ? E->obs_begin : kEmptyCsr, nl + 1);
  S.in(T.obs_other, E->obs_other, no);
  S.in(T.obs_cam, E->obs_camera, no);
  S.in(T.obs_kp, E->obs_keypoint, 2 * no);
  S.in(T.obs_L, E->obs_sqrt_info, 4 * no);
  S.in(T.obs_cauchy, I.cauchy.data(), no);
}

}  // namespace

extern "C" {

int okvisgpu_imu_append(okvisgpu_ctx* c, const okvisgpu_imu_append_batch* A, int32_t* steps) {
  if (!c || !A || A->n < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "imu_append: bad arguments");
  if (A->n == 0) return OKVISGPU_OK;
  if (!A->state || !A->t1_old_ns || !A->t1_new_ns || !A->speed_biases || !A->sample_begin)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "imu_append: missing arrays");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)A->n;
    checkCsr(A->sample_begin, n, "sample_begin", nullptr, "imu_append: ");
    const size_t ns = (size_t)A->sample_begin[n];
    if (ns && (!A->sample_t_ns || !A->sample_gyr_acc)) throw ArgError{"imu_append: sample arrays missing"};
    std::vector<int32_t> blk(4 * n);
    for (size_t i = 0; i < n; ++i) { blk[4 * i] = 0; blk[4 * i + 1] = (int32_t)i; blk[4 * i + 2] = 0; blk[4 * i + 3] = (int32_t)i; }
    double par[7];
    imuParams(A->imu_params, par);
    // a descriptor holding only what the append mode of k_eval_imu reads
    DevProblem D{};
    D.n_imu = A->n;
    D.n_fac = A->n;
    BatchLayout S;
    S.in(D.imu_blocks, blk.data(), 4 * n);
    S.in(D.imu_t0, A->t1_old_ns, n);
    S.in(D.imu_t1, A->t1_new_ns, n);
    S.in(D.imu_sbegin, A->sample_begin, n + 1);
    S.in(D.imu_ts, A->sample_t_ns, ns);
    S.in(D.imu_ga, A->sample_gyr_acc, 6 * ns);
    S.in(D.imu_par, par, 7);
    S.in(D.sb[0], A->speed_biases, 9 * n);
    const auto self = S.in(D.self, nullptr, 1);  // the descriptor itself, staged once its pointers are known
    S.inout(D.imu_state, A->state, A->state, (size_t)kImuState * n);
    c->beginBatch(S);
    D.sb[1] = D.sb[0];
    *S.host(self) = D;
    c->uploadBatch(S);
    launch_imu_append(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    if (steps)
      for (size_t i = 0; i < n; ++i) {
        const int s0 = A->sample_begin[i], s1 = A->sample_begin[i + 1];
        const bool covered = s1 > s0 && A->sample_t_ns[s1 - 1] >= A->t1_new_ns[i];
        steps[i] = covered ? (int32_t)A->state[i * kImuState + 291] : -1;
      }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_imu_propagate(okvisgpu_ctx* c, const okvisgpu_imu_propagate_batch* A, int32_t* steps) {
  if (!c || !A || A->n < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "imu_propagate: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "imu_propagate: call after solve_end");
  if (A->n == 0) return OKVISGPU_OK;
  if (!A->poses || !A->speed_biases || !A->t_start_ns || !A->t_end_ns || !A->sample_begin || !A->sample_t_ns ||
      !A->sample_gyr_acc)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "imu_propagate: missing arrays");
  return guarded(c, [&]() {
    const size_t n = (size_t)A->n;
    checkCsr(A->sample_begin, n, "sample_begin", nullptr, "imu_propagate: ");
    for (size_t i = 0; i < n; ++i)  // (an item that ends before t_end gets steps = -1 on the device)
      checkCovered(A->sample_begin, A->sample_t_ns, i, "t_start", A->t_start_ns[i], nullptr, nullptr, "item",
                   "imu_propagate: ");
    HIPCHK(hipSetDevice(c->device));
    const size_t ns = (size_t)A->sample_begin[n];
    ImuPropagateDev D{};
    D.n = A->n;
    imuParams(A->imu_params, D.par);
    BatchLayout S;
    S.in(D.t_start, A->t_start_ns, n);
    S.in(D.t_end, A->t_end_ns, n);
    S.in(D.sbegin, A->sample_begin, n + 1);
    S.in(D.ts, A->sample_t_ns, ns);
    S.in(D.ga, A->sample_gyr_acc, 6 * ns);
    // an uncovered item's rows stay the caller's: poses and speed/biases come back as they went up; the
    // covariance and Jacobian rows of such an item were never written on the device and are skipped below
    S.inout(D.poses, A->poses, A->poses, 7 * n);
    S.inout(D.sb, A->speed_biases, A->speed_biases, 9 * n);
    const auto st = S.out(D.steps, steps, n);
    BatchSlot<double> cov{-1}, jac{-1};
    if (A->covariance) cov = S.out(D.cov, nullptr, 225 * n);
    if (A->jacobian) jac = S.out(D.jac, nullptr, 225 * n);
    c->beginBatch(S);
    c->uploadBatch(S);
    launch_imu_propagate(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    for (size_t i = 0; i < n; ++i) {
      if (S.host(st)[i] < 0) continue;
      if (A->covariance) std::memcpy(A->covariance + 225 * i, S.host(cov) + 225 * i, 1800);
      if (A->jacobian) std::memcpy(A->jacobian + 225 * i, S.host(jac) + 225 * i, 1800);
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_gps_evaluate(okvisgpu_ctx* c, const okvisgpu_gps_batch* A, okvisgpu_gps_result* R) {
  static_assert(kGpsState == OKVISGPU_GPS_STATE_DOUBLES, "device layout and header layout differ");
  if (!c || !A || !R || A->n < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "gps_evaluate: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "gps_evaluate: call after solve_end");
  if (A->kind != 0 && A->kind != 1)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "gps_evaluate: unknown kind " + std::to_string(A->kind));
  if (A->n == 0) return OKVISGPU_OK;
  const bool async = A->kind == 0;
  if (!A->poses || !A->T_GW || A->n_gw < 1 || !A->measurement || !A->information ||
      (async && (!A->speed_biases || !A->t_k_ns || !A->t_g_ns || !A->sample_begin)))
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "gps_evaluate: missing arrays");
  return guarded(c, [&]() {
    const std::string who = "gps_evaluate: ";
    const size_t n = (size_t)A->n;
    size_t ns = 0;
    if (async) {
      checkCsr(A->sample_begin, n, "sample_begin", "factor", who);
      ns = (size_t)A->sample_begin[n];
      if (ns && (!A->sample_t_ns || !A->sample_gyr_acc)) throw ArgError{who + "sample arrays missing"};
    }
    for (size_t i = 0; i < n; ++i) {
      const std::string fac = who + "factor " + std::to_string(i);
      if (A->gw_index && (A->gw_index[i] < 0 || A->gw_index[i] >= A->n_gw))
        throw ArgError{fac + ": gw_index " + std::to_string(A->gw_index[i]) + " outside [0, n_gw)"};
      const double* G = A->information + 9 * i;
      double top = 0.0, U[9];
      bool finite = true;
      for (int e = 0; e < 9; ++e) {
        finite = finite && std::isfinite(G[e]);
        top = std::max(top, std::fabs(G[e]));
      }
      if (!finite) throw ArgError{fac + ": information is not finite"};
      if (std::fabs(G[1] - G[3]) > 1e-12 * top || std::fabs(G[2] - G[6]) > 1e-12 * top || std::fabs(G[5] - G[7]) > 1e-12 * top)
        throw ArgError{fac + ": information is not symmetric"};
      if (!chol3U(G, U)) throw ArgError{fac + ": information is not positive definite"};
      if (!async) continue;
      if (A->t_g_ns[i] < A->t_k_ns[i])  // (ViGraph.cpp:976-982)
        throw ArgError{fac + ": t_g " + std::to_string(A->t_g_ns[i]) + " < t_k " + std::to_string(A->t_k_ns[i])};
      checkCovered(A->sample_begin, A->sample_t_ns, i, "t_k", A->t_k_ns[i], "t_g", &A->t_g_ns[i], "factor", who);
    }
    HIPCHK(hipSetDevice(c->device));
    GpsDev D{};
    D.n = A->n;
    D.kind = A->kind;
    D.use_cov = A->use_imu_covariance ? 1 : 0;
    D.redo_always = A->redo_propagation_always ? 1 : 0;
    {  // (development: the four-matrix recursion, for the comparison of scripts/gps_timing.py)
      const char* e = std::getenv("OKVISGPU_GPS_FOUR_P");
      D.four_p = e && e[0] == '1';
    }
    imuParams(A->imu_params, D.par);
    std::memcpy(D.r_SA, A->r_SA, sizeof(D.r_SA));
    BatchLayout S;
    S.in(D.poses, A->poses, 7 * n);
    S.in(D.T_GW, A->T_GW, 7 * (size_t)A->n_gw);
    if (A->gw_index) S.in(D.gw_index, A->gw_index, n);
    S.in(D.meas, A->measurement, 3 * n);
    S.in(D.info, A->information, 9 * n);
    if (async) {
      S.in(D.sb, A->speed_biases, 9 * n);
      S.in(D.t_k, A->t_k_ns, n);
      S.in(D.t_g, A->t_g_ns, n);
      S.in(D.sbegin, A->sample_begin, n + 1);
      S.in(D.ts, A->sample_t_ns, ns);
      S.in(D.ga, A->sample_gyr_acc, 6 * ns);
      if (A->state) S.inout(D.state, A->state, A->state, (size_t)kGpsState * n);
    }
    if (R->r) S.out(D.r, R->r, 3 * n);
    if (R->error) S.out(D.error, R->error, 3 * n);
    if (R->sqrt_info) S.out(D.sqrt_info, R->sqrt_info, 9 * n);
    if (R->J_pose) S.out(D.J_pose, R->J_pose, 18 * n);
    if (R->J_speed_bias) S.out(D.J_sb, R->J_speed_bias, 27 * n);
    if (R->J_T_GW) S.out(D.J_gw, R->J_T_GW, 18 * n);
    if (R->J_pose_ambient) S.out(D.J_pose_amb, R->J_pose_ambient, 21 * n);
    if (R->J_T_GW_ambient) S.out(D.J_gw_amb, R->J_T_GW_ambient, 21 * n);
    if (R->steps) S.out(D.steps, R->steps, n);
    c->beginBatch(S);
    c->uploadBatch(S);
    launch_gps_evaluate(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_lidar_deskew(okvisgpu_ctx* c, const okvisgpu_lidar_deskew_batch* A, okvisgpu_lidar_deskew_result* R) {
  if (!c || !A || !R || A->n_scans < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "lidar_deskew: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "lidar_deskew: call after solve_end");
  if (!std::isfinite(A->g)) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "lidar_deskew: g is not finite");
  if (A->n_scans == 0) return OKVISGPU_OK;
  if (!A->pose0 || !A->speed_bias0 || !A->t_start_ns || !A->sample_begin || !A->query_begin)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "lidar_deskew: missing arrays");
  return guarded(c, [&]() {
    const std::string who = "lidar_deskew: ";
    const size_t n = (size_t)A->n_scans;
    checkCsr(A->sample_begin, n, "sample_begin", "scan", who);
    checkCsr(A->query_begin, n, "query_begin", "scan", who);
    const size_t ns = (size_t)A->sample_begin[n], nq = (size_t)A->query_begin[n];
    const bool points = R->point || R->point_f64;
    if (ns && (!A->sample_t_ns || !A->sample_gyr_acc)) throw ArgError{who + "sample arrays missing"};
    if (nq && !A->query_t_ns) throw ArgError{who + "query_t_ns missing"};
    if (nq && points && (!A->ray || !A->pose_live || !A->T_SL))
      throw ArgError{who + "ray, pose_live and T_SL are needed for the point outputs"};
    std::vector<int32_t> before(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const int32_t s0 = A->sample_begin[i], s1 = A->sample_begin[i + 1];
      const int32_t q0 = A->query_begin[i], q1 = A->query_begin[i + 1];
      const std::string scan = who + "scan " + std::to_string(i);
      if (q1 > q0 && s1 - s0 < 2) throw ArgError{scan + " has queries but fewer than two samples"};
      if (s1 > s0)  // (a scan without queries may come without samples)
        checkCovered(A->sample_begin, A->sample_t_ns, i, "t_start", A->t_start_ns[i], nullptr, nullptr, "scan", who);
      for (int32_t s = s0 + 1; s < s1; ++s)
        if (A->sample_t_ns[s] < A->sample_t_ns[s - 1])
          throw ArgError{scan + ": sample stamps decrease at sample " + std::to_string(s - s0)};
      for (int32_t q = q0; q < q1; ++q) {
        if (q > q0 && A->query_t_ns[q] < A->query_t_ns[q - 1])
          throw ArgError{scan + ": query stamps decrease at query " + std::to_string(q - q0)};
        before[i] += A->query_t_ns[q] < A->t_start_ns[i];
      }
    }
    if (!nq) {  // nothing to propagate
      if (R->n_before) std::fill(R->n_before, R->n_before + n, 0);
      return (int)OKVISGPU_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    LidarDeskewDev D{};
    D.n_scans = A->n_scans;
    D.n_query = (int32_t)nq;
    D.g = A->g;
    BatchLayout S;
    S.in(D.pose0, A->pose0, 7 * n);
    S.in(D.sb0, A->speed_bias0, 9 * n);
    S.in(D.t_start, A->t_start_ns, n);
    S.in(D.sbegin, A->sample_begin, n + 1);
    S.in(D.ts, A->sample_t_ns, ns);
    S.in(D.ga, A->sample_gyr_acc, 6 * ns);
    S.in(D.qbegin, A->query_begin, n + 1);
    const auto qScan = S.in(D.q_scan, nullptr, nq);
    S.in(D.qt, A->query_t_ns, nq);
    if (points) {
      S.in(D.ray, A->ray, 3 * nq);
      S.in(D.pose_live, A->pose_live, 7 * n);
      S.in(D.T_SL, A->T_SL, 7 * n);
    }
    if (R->valid) S.out(D.valid, R->valid, nq);
    if (R->point) S.out(D.point, R->point, 3 * nq);
    if (R->point_f64) S.out(D.point_f64, R->point_f64, 3 * nq);
    if (R->pose) S.out(D.pose, R->pose, 7 * nq);
    if (R->speed) S.out(D.speed, R->speed, 3 * nq);
    if (R->omega_S) S.out(D.omega, R->omega_S, 3 * nq);
    S.scratch(D.table, (size_t)kLidarRow * ns);  // written by the chain kernel, read by the point kernel
    c->beginBatch(S);
    for (size_t i = 0; i < n; ++i)  // the scan of every query
      for (int32_t q = A->query_begin[i]; q < A->query_begin[i + 1]; ++q) S.host(qScan)[q] = (int32_t)i;
    c->uploadBatch(S);
    launch_lidar_chain(D, c->stream);
    HIPCHK(hipGetLastError());
    launch_lidar_points(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    if (R->n_before) std::copy(before.begin(), before.end(), R->n_before);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_voxel_downsample(okvisgpu_ctx* c, const okvisgpu_voxel_downsample_batch* A,
                              okvisgpu_voxel_downsample_result* R) {
  if (!c || !A || !R || A->n_clouds < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "voxel_downsample: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "voxel_downsample: call after solve_end");
  if (A->n_clouds == 0) return OKVISGPU_OK;
  if (!A->cloud_begin || !A->voxel_size)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "voxel_downsample: missing arrays");
  return guarded(c, [&]() {
    const std::string who = "voxel_downsample: ";
    const size_t n = (size_t)A->n_clouds;
    checkCsr(A->cloud_begin, n, "cloud_begin", "cloud", who);
    const size_t np = (size_t)A->cloud_begin[n];
    if (np && !A->point) throw ArgError{who + "point missing"};
    if (np > ((size_t)1 << 29)) throw ArgError{who + "more than 2^29 points"};
    std::vector<float> vsize(n);
    for (size_t i = 0; i < n; ++i) {
      if (!(std::isfinite(A->voxel_size[i]) && A->voxel_size[i] > 0.0))
        throw ArgError{who + "voxel_size of cloud " + std::to_string(i) + " is not finite and positive"};
      vsize[i] = (float)A->voxel_size[i];  // Eigen promotes the divisor to the expression's scalar
    }
    if (!np) {
      if (R->n_kept) std::fill(R->n_kept, R->n_kept + n, 0);
      return (int)OKVISGPU_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    VoxelDev D{};
    D.n_points = (int32_t)np;
    D.n_clouds = A->n_clouds;
    D.table_size = 64;
    while ((size_t)D.table_size < 2 * np) D.table_size *= 2;
    BatchLayout S;
    const auto ptCloud = S.in(D.pt_cloud, nullptr, np);
    S.in(D.point, A->point, 3 * np);
    S.in(D.vsize, vsize.data(), n);
    if (A->use) S.in(D.use, A->use, np);
    // delivered below, once the error word is known to be clear
    const auto keep = S.out(D.keep, nullptr, np);
    const auto kept = S.out(D.n_kept, nullptr, n);
    const auto err = S.out(D.err, nullptr, 1);
    S.scratch(D.table, (size_t)D.table_size);
    S.scratch(D.best, (size_t)D.table_size);
    S.scratch(D.slot, np);
    c->beginBatch(S);
    for (size_t i = 0; i < n; ++i)  // the cloud of every point
      for (int32_t p = A->cloud_begin[i]; p < A->cloud_begin[i + 1]; ++p) S.host(ptCloud)[p] = (int32_t)i;
    c->uploadBatch(S);
    launch_voxel_downsample(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    if (*S.host(err)) throw std::runtime_error("voxel_downsample: hash table exhausted");
    if (R->keep) std::memcpy(R->keep, S.host(keep), np);
    if (R->n_kept) std::memcpy(R->n_kept, S.host(kept), sizeof(int32_t) * n);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_frame_overlap(okvisgpu_ctx* c, const okvisgpu_frame_overlap_batch* A, okvisgpu_frame_overlap_result* R) {
  if (!c || !A || !R) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "frame_overlap: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "frame_overlap: call after solve_end");
  if (A->n_frames < 0 || A->n_jobs < 0 || A->n_groups < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "frame_overlap: negative count");
  return guarded(c, [&]() {
    const std::string who = "frame_overlap: ";
    const size_t nf = (size_t)A->n_frames, nj = (size_t)A->n_jobs, ng = (size_t)A->n_groups;
    if (nf && !A->image_begin) throw ArgError{who + "image_begin missing"};
    if (nf) checkCsr(A->image_begin, nf, "image_begin", "frame", who);
    const size_t ni = nf ? (size_t)A->image_begin[nf] : 0;
    if (ni && (!A->rows || !A->cols || !A->kp_begin)) throw ArgError{who + "image arrays missing"};
    if (ni) checkCsr(A->kp_begin, ni, "kp_begin", "image", who);
    const size_t nk = ni ? (size_t)A->kp_begin[ni] : 0;
    if (nk && (!A->keypoint || !A->landmark)) throw ArgError{who + "keypoint arrays missing"};
    if (nj && (!A->job_kind || !A->job_frame_a || !A->job_radius_factor)) throw ArgError{who + "job arrays missing"};
    if (ng && !A->group_begin) throw ArgError{who + "group_begin missing"};
    if (ng) checkCsr(A->group_begin, ng, "group_begin", "group", who);
    if (ng && (size_t)A->group_begin[ng] > nj) throw ArgError{who + "group_begin exceeds n_jobs"};
    // the grid of every image
    std::vector<int32_t> gr(ni), gc(ni), imgFrame(ni);
    std::vector<uint8_t> imgLive(ni);
    for (size_t f = 0; f < nf; ++f)
      for (int32_t im = A->image_begin[f]; im < A->image_begin[f + 1]; ++im) imgFrame[(size_t)im] = (int32_t)f;
    for (size_t im = 0; im < ni; ++im) {
      if (A->rows[im] < 0 || A->cols[im] < 0) throw ArgError{who + "negative rows or cols of image " + std::to_string(im)};
      gr[im] = A->rows[im] / 10;
      gc[im] = A->cols[im] / 10;
      imgLive[im] = A->rows[im] > 0 && A->cols[im] > 0;
      if ((size_t)gr[im] * (size_t)((gc[im] + 31) / 32) > (size_t)OKVISGPU_OVERLAP_MASK_WORDS)
        throw ArgError{who + "image " + std::to_string(im) + ": a " + std::to_string(gr[im]) + " x " + std::to_string(gc[im]) +
                       " grid needs more than OKVISGPU_OVERLAP_MASK_WORDS words per mask"};
    }
    // the items, and one half-width table per distinct radius
    std::vector<OverlapItem> items;
    std::vector<int32_t> hw, hwOff((size_t)OKVISGPU_OVERLAP_MAX_RADIUS + 1, -1);
    auto tableOf = [&](int32_t Rad) {
      if (hwOff[(size_t)Rad] < 0) {
        hwOff[(size_t)Rad] = (int32_t)hw.size();
        hw.resize(hw.size() + (size_t)Rad + 1, 0);
        int32_t* h = hw.data() + hwOff[(size_t)Rad];
        int err = 0, dx = Rad, dy = 0, plus = 1, minus = 2 * Rad - 1;
        while (dx >= dy) {  // the midpoint recurrence of OpenCV's Circle()
          h[dy] = std::max(h[dy], dx);
          h[dx] = std::max(h[dx], dy);
          ++dy;
          err += plus;
          plus += 2;
          if (err > 0) {
            err -= minus;
            --dx;
            minus -= 2;
          }
        }
      }
      return hwOff[(size_t)Rad];
    };
    int32_t maxWords = 1;
    std::vector<int32_t> nKeypoints(nj, 0);
    for (size_t j = 0; j < nj; ++j) {
      const std::string job = who + "job " + std::to_string(j);
      const int32_t kind = A->job_kind[j], fa = A->job_frame_a[j];
      if (kind < 0 || kind > 3) throw ArgError{job + ": unknown kind " + std::to_string(kind)};
      if (fa < 0 || fa >= A->n_frames) throw ArgError{job + ": frame_a " + std::to_string(fa) + " out of range"};
      int32_t fb = -1;
      if (kind <= 1) {
        if (!A->job_frame_b) throw ArgError{who + "job_frame_b missing"};
        fb = A->job_frame_b[j];
        if (fb < 0 || fb >= A->n_frames) throw ArgError{job + ": frame_b " + std::to_string(fb) + " out of range"};
      }
      if (kind == 0 && A->image_begin[fa + 1] - A->image_begin[fa] != A->image_begin[fb + 1] - A->image_begin[fb])
        throw ArgError{job + ": frames " + std::to_string(fa) + " and " + std::to_string(fb) + " differ in image count"};
      if (kind == 3 && !A->flag) throw ArgError{job + ": kind 3 needs flag"};
      const double factor = A->job_radius_factor[j];
      if (!(std::isfinite(factor) && factor >= 0.0)) throw ArgError{job + ": radius factor is not finite and >= 0"};
      nKeypoints[j] = ni ? A->kp_begin[A->image_begin[fa + 1]] - A->kp_begin[A->image_begin[fa]] : 0;
      for (int side = (kind == 1 ? 1 : 0); side <= (kind <= 1 ? 1 : 0); ++side) {
        const int32_t f = side ? fb : fa;
        for (int32_t im = A->image_begin[f]; im < A->image_begin[f + 1]; ++im) {
          if (kind == 0 && !imgLive[(size_t)im]) continue;  // (:2922)
          const double radius = (double)std::min(gr[(size_t)im], gc[(size_t)im]) * factor;
          if (!(radius < (double)OKVISGPU_OVERLAP_MAX_RADIUS + 1.0))
            throw ArgError{job + ": radius above OKVISGPU_OVERLAP_MAX_RADIUS on image " + std::to_string(im)};
          const int32_t Rad = (int32_t)radius;
          const double area = radius * radius * 3.14159265358979323846;  // M_PI; < 2^22
          const int32_t other = kind == 0 ? (side ? fa : fb) : (kind == 1 ? fa : -1);
          items.push_back({(int32_t)j, side, im, other, kind, Rad, tableOf(Rad), (int32_t)area});
          maxWords = std::max(maxWords, gr[(size_t)im] * ((gc[(size_t)im] + 31) / 32));
        }
      }
    }
    if (!nj) {  // nothing to paint: every group is empty
      if (R->group_best) std::fill(R->group_best, R->group_best + ng, -1);
      if (R->group_max) std::fill(R->group_max, R->group_max + ng, 0.0);
      return (int)OKVISGPU_OK;
    }
    // one id table per frame: the smallest power of two >= two slots per keypoint
    std::vector<int32_t> tabBegin(nf + 1, 0);
    for (size_t f = 0; f < nf; ++f) {
      const size_t kf = ni ? (size_t)(A->kp_begin[A->image_begin[f + 1]] - A->kp_begin[A->image_begin[f]]) : 0;
      size_t size = 2;
      while (size < 2 * kf) size *= 2;
      if ((size_t)tabBegin[f] + size > (size_t)0x7fffffff) throw ArgError{who + "too many keypoints"};
      tabBegin[f + 1] = tabBegin[f] + (int32_t)size;
    }
    HIPCHK(hipSetDevice(c->device));
    OverlapDev D{};
    D.n_kp = (int32_t)nk;
    D.n_items = (int32_t)items.size();
    D.n_jobs = A->n_jobs;
    D.n_groups = A->n_groups;
    D.table_total = tabBegin[nf];
    D.max_words = maxWords;
    BatchLayout S;
    S.in(D.kp_begin, ni ? A->kp_begin : kEmptyCsr, ni + 1);
    const auto kpImage = S.in(D.kp_image, nullptr, nk);
    S.in(D.kp, A->keypoint, 2 * nk);
    S.in(D.lm, A->landmark, nk);
    if (A->flag) S.in(D.flag, A->flag, nk);
    S.in(D.img_frame, imgFrame.data(), ni);
    S.in(D.img_gr, gr.data(), ni);
    S.in(D.img_gc, gc.data(), ni);
    S.in(D.img_live, imgLive.data(), ni);
    S.in(D.tab_begin, tabBegin.data(), nf + 1);
    S.in(D.items, items.data(), items.size());
    S.in(D.hw, hw.data(), hw.size());
    S.in(D.job_kind, A->job_kind, nj);
    if (ng) S.in(D.group_begin, A->group_begin, ng + 1);
    // delivered below, once the error word is known to be clear
    const auto overlap = S.out(D.overlap, nullptr, nj);
    const auto count = S.out(D.count, nullptr, 4 * nj);
    const auto matched = S.out(D.n_matched, nullptr, 2 * nj);
    const auto best = S.out(D.group_best, nullptr, ng);
    const auto gmax = S.out(D.group_max, nullptr, ng);
    const auto err = S.out(D.err, nullptr, 1);
    S.scratch(D.table, (size_t)D.table_total);
    S.scratch(D.live, (size_t)D.table_total);
    c->beginBatch(S);
    for (size_t im = 0; im < ni; ++im)  // the image of every keypoint
      for (int32_t k = A->kp_begin[im]; k < A->kp_begin[im + 1]; ++k) S.host(kpImage)[k] = (int32_t)im;
    c->uploadBatch(S);
    launch_frame_overlap(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    if (*S.host(err)) throw std::runtime_error("frame_overlap: id table exhausted");
    if (R->overlap) std::memcpy(R->overlap, S.host(overlap), sizeof(double) * nj);
    if (R->count) std::memcpy(R->count, S.host(count), sizeof(int32_t) * 4 * nj);
    if (R->n_matched) std::memcpy(R->n_matched, S.host(matched), sizeof(int32_t) * 2 * nj);
    if (R->n_keypoints) std::copy(nKeypoints.begin(), nKeypoints.end(), R->n_keypoints);
    if (R->group_best && ng) std::memcpy(R->group_best, S.host(best), sizeof(int32_t) * ng);
    if (R->group_max && ng) std::memcpy(R->group_max, S.host(gmax), sizeof(double) * ng);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_match_to_map(okvisgpu_ctx* c, const okvisgpu_match_batch* A, okvisgpu_match_result* R) {
  if (!c || !A || !R) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "match_to_map: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "match_to_map: call after solve_end");
  if (A->n_jobs < 0 || A->n_landmarks < 0 || A->n_poses < 0 || A->n_cameras < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "match_to_map: negative count");
  if (A->n_jobs == 0) return OKVISGPU_OK;
  return guarded(c, [&]() {
    const std::string who = "match_to_map: ";
    const size_t nj = (size_t)A->n_jobs, nl = (size_t)A->n_landmarks, nc = (size_t)A->n_cameras;
    if (!A->job_camera || !A->job_pass || !A->job_pose_prepare || !A->job_pose_match || !A->kp_begin)
      throw ArgError{who + "job arrays missing"};
    if (!nc || !A->cameras || !A->extrinsics) throw ArgError{who + "cameras missing"};
    checkCsr(A->kp_begin, nj, "kp_begin", "job", who);
    const size_t nk = (size_t)A->kp_begin[nj];
    if (nk && (!A->keypoint || !A->descriptor || !A->ray || !A->ray_valid || !A->landmark))
      throw ArgError{who + "keypoint arrays missing"};
    if (nl && (!A->landmarks || !A->landmark_quality || !A->obs_begin)) throw ArgError{who + "landmark arrays missing"};
    if (nl) checkCsr(A->obs_begin, nl, "obs_begin", "landmark", who);
    const size_t no = nl ? (size_t)A->obs_begin[nl] : 0;
    if (no && (!A->obs_pose || !A->obs_camera || !A->obs_descriptor || !A->obs_ray || !A->poses))
      throw ArgError{who + "observation arrays missing"};
    for (size_t o = 0; o < no; ++o) {
      if (A->obs_pose[o] < 0 || A->obs_pose[o] >= A->n_poses)
        throw ArgError{who + "obs_pose out of range at observation " + std::to_string(o)};
      if (A->obs_camera[o] < 0 || A->obs_camera[o] >= A->n_cameras)
        throw ArgError{who + "obs_camera out of range at observation " + std::to_string(o)};
    }
    size_t nk0 = 0;
    for (size_t j = 0; j < nj; ++j) {
      if (A->job_camera[j] < 0 || A->job_camera[j] >= A->n_cameras)
        throw ArgError{who + "job_camera out of range at job " + std::to_string(j)};
      if (A->job_pass[j] != 0 && A->job_pass[j] != 1) throw ArgError{who + "job_pass not 0 / 1 at job " + std::to_string(j)};
      if (A->job_pass[j] == 0) nk0 += (size_t)(A->kp_begin[j + 1] - A->kp_begin[j]);
    }
    for (size_t k = 0; k < nk; ++k)
      if (A->landmark[k] < -1 || A->landmark[k] >= A->n_landmarks)
        throw ArgError{who + "carried landmark out of range at keypoint " + std::to_string(k)};
    const std::vector<double> cam = packCameras(A->cameras, nc, kMatchCamDoubles, who);
    HIPCHK(hipSetDevice(c->device));
    const size_t njl = nj * nl;
    MatchDev D{};
    D.n_jobs = A->n_jobs;
    D.n_lm = A->n_landmarks;
    D.n_kp0 = (int32_t)nk0;
    D.n_kp1 = (int32_t)(nk - nk0);
    D.imu_use = A->imu_use ? 1 : 0;
    D.loop_closure = A->loop_closure ? 1 : 0;
    D.threshold = A->matching_threshold;
    BatchLayout S;
    S.in(D.poses, A->poses, 7 * (size_t)A->n_poses);
    S.in(D.cam, cam.data(), cam.size());
    S.in(D.extr, A->extrinsics, 7 * nc);
    S.in(D.lm, A->landmarks, 4 * nl);
    S.in(D.lm_quality, A->landmark_quality, nl);
    if (A->landmark_use) S.in(D.lm_use, A->landmark_use, nl);
    S.in(D.obs_begin, nl ? A->obs_begin : nullptr, nl + 1);
    S.in(D.obs_pose, A->obs_pose, no);
    S.in(D.obs_cam, A->obs_camera, no);
    S.in(D.obs_desc, A->obs_descriptor, 12 * no);
    S.in(D.obs_ray, A->obs_ray, 3 * no);
    S.in(D.job_cam, A->job_camera, nj);
    S.in(D.job_pose_prepare, A->job_pose_prepare, 7 * nj);
    S.in(D.job_pose_match, A->job_pose_match, 7 * nj);
    const auto kpList = S.in(D.kp_list, nullptr, nk);
    const auto kpJob = S.in(D.kp_job, nullptr, nk);
    S.in(D.kp_xy, A->keypoint, 2 * nk);
    S.in(D.kp_desc, A->descriptor, 12 * nk);
    S.in(D.kp_ray, A->ray, 3 * nk);
    S.in(D.kp_ray_valid, A->ray_valid, nk);
    S.in(D.kp_lm, A->landmark, nk);
    S.out(D.cand_n, R->cand_n, njl);
    S.out(D.cand_is3d, R->cand_is3d, njl);
    S.out(D.cand_obs, R->cand_obs, 3 * njl);
    S.out(D.cand_proj, R->cand_projection, 2 * njl);
    S.out(D.out_match, R->match_landmark, nk);
    S.out(D.out_dist, R->match_distance, nk);
    S.out(D.out_records, R->n_records, nk);
    S.out(D.out_sum, R->record_repr_sum, nk);
    S.out(D.out_point, R->point, 4 * nk);
    S.scratch(D.cand_geo, 18 * njl);
    S.scratch(D.cand_desc, 36 * njl);
    c->beginBatch(S);
    {  // the keypoints of the pass-0 jobs, then those of the pass-1 jobs; the job of every keypoint
      int32_t *list = S.host(kpList), *job = S.host(kpJob);
      size_t at0 = 0, at1 = nk0;
      for (size_t j = 0; j < nj; ++j)
        for (int32_t k = A->kp_begin[j]; k < A->kp_begin[j + 1]; ++k) {
          job[k] = (int32_t)j;
          list[A->job_pass[j] == 0 ? at0++ : at1++] = k;
        }
    }
    c->uploadBatch(S);
    launch_match_prepare(D, c->stream);
    HIPCHK(hipGetLastError());
    launch_match(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_match_frames(okvisgpu_ctx* c, const okvisgpu_frame_match_batch* A, okvisgpu_frame_match_result* R) {
  if (!c || !A || !R) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "match_frames: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "match_frames: call after solve_end");
  if (A->n_jobs < 0 || A->n_cameras < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "match_frames: negative count");
  if (A->n_jobs == 0) return OKVISGPU_OK;
  return guarded(c, [&]() {
    const std::string who = "match_frames: ";
    const size_t nj = (size_t)A->n_jobs, nc = (size_t)A->n_cameras;
    if (!A->job_mode || !A->job_camera0 || !A->job_camera1 || !A->job_pose0 || !A->job_pose1 || !A->job_extrinsics0 ||
        !A->job_extrinsics1 || !A->kp0_begin || !A->kp1_begin)
      throw ArgError{who + "job arrays missing"};
    if (!nc || !A->cameras) throw ArgError{who + "cameras missing"};
    checkCsr(A->kp0_begin, nj, "kp0_begin", "job", who);
    checkCsr(A->kp1_begin, nj, "kp1_begin", "job", who);
    const size_t n0 = (size_t)A->kp0_begin[nj], n1 = (size_t)A->kp1_begin[nj];
    if (n0 && (!A->size0 || !A->descriptor0 || !A->ray0 || !A->ray_valid0)) throw ArgError{who + "side-0 keypoint arrays missing"};
    if (n1 && (!A->keypoint1 || !A->size1 || !A->descriptor1 || !A->ray1 || !A->ray_valid1))
      throw ArgError{who + "side-1 keypoint arrays missing"};
    for (size_t j = 0; j < nj; ++j) {
      if (A->job_mode[j] != 0 && A->job_mode[j] != 1) throw ArgError{who + "job_mode not 0 / 1 at job " + std::to_string(j)};
      if (A->job_camera0[j] < 0 || A->job_camera0[j] >= A->n_cameras)
        throw ArgError{who + "job_camera0 out of range at job " + std::to_string(j)};
      if (A->job_camera1[j] < 0 || A->job_camera1[j] >= A->n_cameras)
        throw ArgError{who + "job_camera1 out of range at job " + std::to_string(j)};
    }
    const std::vector<double> cam = packCameras(A->cameras, nc, kMatchCamDoubles, who);
    // the side-0 keypoints that take part (use0 and ray_valid0: in mode 1 a keypoint without a valid ray
    // has no admissible candidate), per mode
    size_t nl[2] = {0, 0};
    for (size_t j = 0; j < nj; ++j)
      for (int32_t k = A->kp0_begin[j]; k < A->kp0_begin[j + 1]; ++k)
        if ((!A->use0 || A->use0[k]) && A->ray_valid0[k]) ++nl[A->job_mode[j]];
    HIPCHK(hipSetDevice(c->device));
    FrameMatchDev D{};
    D.n_jobs = A->n_jobs;
    D.n_kp0 = (int32_t)n0;
    D.n_kp1 = (int32_t)n1;
    D.n_list0 = (int32_t)nl[0];
    D.n_list1 = (int32_t)nl[1];
    {  // d < best as the reference starts it: uint32_t(threshold) in mode 0, the double itself in mode 1
      const double t = A->matching_threshold;
      const double lim = 385.0;  // above every distance of 384 bits
      D.best_init[0] = !(t > 0.0) ? 0 : (int32_t)std::floor(std::min(t, lim));
      D.best_init[1] = !(t > 0.0) ? 0 : (int32_t)std::ceil(std::min(t, lim));
    }
    BatchLayout S;
    S.in(D.cam, cam.data(), cam.size());
    S.in(D.job_cam0, A->job_camera0, nj);
    S.in(D.job_cam1, A->job_camera1, nj);
    S.in(D.job_pose0, A->job_pose0, 7 * nj);
    S.in(D.job_pose1, A->job_pose1, 7 * nj);
    S.in(D.job_ext0, A->job_extrinsics0, 7 * nj);
    S.in(D.job_ext1, A->job_extrinsics1, 7 * nj);
    S.in(D.kp1_begin, A->kp1_begin, nj + 1);
    const auto job0 = S.in(D.kp0_job, nullptr, n0);
    const auto job1 = S.in(D.kp1_job, nullptr, n1);
    const auto kpList = S.in(D.kp_list, nullptr, nl[0] + nl[1]);
    S.in(D.size0, A->size0, n0);
    S.in(D.desc0, A->descriptor0, 12 * n0);
    S.in(D.ray0, A->ray0, 3 * n0);
    S.in(D.xy1, A->keypoint1, 2 * n1);
    S.in(D.size1, A->size1, n1);
    S.in(D.desc1, A->descriptor1, 12 * n1);
    S.in(D.ray1, A->ray1, 3 * n1);
    S.in(D.valid1, A->ray_valid1, n1);
    if (A->use1) S.in(D.use1, A->use1, n1);
    S.out(D.out_match, R->match, n0);
    S.out(D.out_dist, R->distance, n0);
    S.out(D.out_point, R->point, 4 * n0);
    S.out(D.out_quality, R->quality, n0);
    S.out(D.out_init, R->initialisable, n0);
    // written by the prepare kernel, read by the match kernels
    S.scratch(D.job_geo, (size_t)kFrameGeoDoubles * nj);
    S.scratch(D.e0, 3 * n0);
    S.scratch(D.e1, 3 * n1);
    S.scratch(D.flag1, n1);
    c->beginBatch(S);
    {  // the job of every keypoint; the participating side-0 keypoints of the mode-0 jobs, then the mode-1 jobs'
      int32_t *j0 = S.host(job0), *j1 = S.host(job1), *list = S.host(kpList);
      size_t at[2] = {0, nl[0]};
      for (size_t j = 0; j < nj; ++j) {
        for (int32_t k = A->kp0_begin[j]; k < A->kp0_begin[j + 1]; ++k) {
          j0[k] = (int32_t)j;
          if ((!A->use0 || A->use0[k]) && A->ray_valid0[k]) list[at[A->job_mode[j]]++] = k;
        }
        for (int32_t k = A->kp1_begin[j]; k < A->kp1_begin[j + 1]; ++k) j1[k] = (int32_t)j;
      }
    }
    c->uploadBatch(S);
    launch_match_frames_prepare(D, c->stream);
    HIPCHK(hipGetLastError());
    launch_match_frames(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_place_match(okvisgpu_ctx* c, const okvisgpu_place_match_batch* A, okvisgpu_place_match_result* R) {
  if (!c || !A || !R) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_match: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_match: call after solve_end");
  if (A->n_jobs < 0 || A->n_cameras < 0 || A->n_images < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_match: negative count");
  if (A->n_jobs == 0) return OKVISGPU_OK;
  return guarded(c, [&]() {
    const std::string who = "place_match: ";
    const size_t nj = (size_t)A->n_jobs, nc = (size_t)A->n_cameras, ni = (size_t)A->n_images;
    if (!A->lm_begin || (nc && !A->job_image)) throw ArgError{who + "job arrays missing"};
    if (ni && !A->kp_begin) throw ArgError{who + "kp_begin missing"};
    if (ni) checkCsr(A->kp_begin, ni, "kp_begin", "image", who);
    const size_t nk = ni ? (size_t)A->kp_begin[ni] : 0;
    if (nk && !A->descriptor) throw ArgError{who + "descriptor missing"};
    checkCsr(A->lm_begin, nj, "lm_begin", "job", who);
    const size_t nl = (size_t)A->lm_begin[nj];
    if (nl && !A->desc_begin) throw ArgError{who + "desc_begin missing"};
    if (nl) checkCsr(A->desc_begin, nl, "desc_begin", "landmark", who);
    const size_t nd = nl ? (size_t)A->desc_begin[nl] : 0;
    if (nd && !A->old_descriptor) throw ArgError{who + "old_descriptor missing"};
    for (size_t i = 0; i < nj * nc; ++i)
      if (A->job_image[i] < -1 || A->job_image[i] >= A->n_images)
        throw ArgError{who + "job_image out of range at job " + std::to_string(i / nc)};
    if (nl * nc > (size_t)0x7fffffff) throw ArgError{who + "too many (landmark, camera) pairs"};
    const size_t no = nl * nc;
    if (!no) {  // nothing to match: every job has ctr = 0
      if (R->job_matches) std::fill(R->job_matches, R->job_matches + nj, 0);
      return (int)OKVISGPU_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    PlaceMatchDev D{};
    D.n_lm = (int32_t)nl;
    D.n_cam = (int32_t)nc;
    {  // distMin's start: uint32_t(threshold), above no distance of 384 bits when clamped to 385
      const double t = A->matching_threshold;
      D.best_init = !(t > 0.0) ? 0 : (int32_t)std::floor(std::min(t, 385.0));
      D.start_matches = (double)D.best_init < t && t <= 385.0;  // (:338 on a distMin nothing replaced)
    }
    BatchLayout S;
    S.in(D.kp_begin, ni ? A->kp_begin : kEmptyCsr, ni + 1);
    S.in(D.desc, A->descriptor, 12 * nk);
    S.in(D.job_image, A->job_image, nj * nc);
    const auto lmJob = S.in(D.lm_job, nullptr, nl);
    S.in(D.desc_begin, A->desc_begin, nl + 1);
    S.in(D.old_desc, A->old_descriptor, 12 * nd);
    const auto kp = S.out(D.out_kp, R->match_keypoint, no);
    S.out(D.out_dist, R->match_distance, no);
    c->beginBatch(S);
    for (size_t j = 0; j < nj; ++j)  // the job of every landmark
      for (int32_t l = A->lm_begin[j]; l < A->lm_begin[j + 1]; ++l) S.host(lmJob)[l] = (int32_t)j;
    c->uploadBatch(S);
    launch_place_match(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    if (R->job_matches) {  // ctr: the job's (landmark, camera) pairs with a match
      const int32_t* mk = S.host(kp);
      for (size_t j = 0; j < nj; ++j) {
        int32_t ctr = 0;
        for (size_t i = (size_t)A->lm_begin[j] * nc; i < (size_t)A->lm_begin[j + 1] * nc; ++i) ctr += mk[i] >= 0;
        R->job_matches[j] = ctr;
      }
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_place_refine(okvisgpu_ctx* c, const okvisgpu_place_refine_batch* A, okvisgpu_place_refine_result* R) {
  if (!c || !A || !R) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_refine: bad arguments");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_refine: call after solve_end");
  if (A->n_jobs < 0 || A->n_cameras < 0 || A->max_num_iterations < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_refine: negative count");
  if (A->loss.kind < OKVISGPU_LOSS_NONE || A->loss.kind > OKVISGPU_LOSS_TOLERANT)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_refine: unknown loss kind " + std::to_string(A->loss.kind));
  if (!lossValid(A->loss)) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "place_refine: non-positive loss scale");
  if (A->n_jobs == 0) return OKVISGPU_OK;
  return guarded(c, [&]() {
    const std::string who = "place_refine: ";
    const size_t nj = (size_t)A->n_jobs, nc = (size_t)A->n_cameras;
    if (!A->pose || !A->obs_begin) throw ArgError{who + "job arrays missing"};
    checkCsr(A->obs_begin, nj, "obs_begin", "job", who);
    const size_t no = (size_t)A->obs_begin[nj];
    if (no && (!A->obs_camera || !A->obs_keypoint || !A->obs_sqrt_info || !A->obs_point))
      throw ArgError{who + "observation arrays missing"};
    if (no && (!nc || !A->cameras || !A->extrinsics)) throw ArgError{who + "cameras missing"};
    for (size_t o = 0; o < no; ++o)
      if (A->obs_camera[o] < 0 || A->obs_camera[o] >= A->n_cameras)
        throw ArgError{who + "obs_camera out of range at observation " + std::to_string(o)};
    const std::vector<double> cam = packCameras(A->cameras, A->cameras ? nc : 0, kCamDoubles, who);
    HIPCHK(hipSetDevice(c->device));
    PlaceRefineDev D{};
    D.n_jobs = A->n_jobs;
    D.max_iter = A->max_num_iterations;
    D.loss_kind = A->loss.kind;
    D.loss_a = A->loss.a;
    D.loss_b = A->loss.b;
    BatchLayout S;
    S.in(D.cam, cam.data(), cam.size());
    S.in(D.extr, A->extrinsics, 7 * nc);
    S.in(D.obs_begin, A->obs_begin, nj + 1);
    S.in(D.obs_cam, A->obs_camera, no);
    S.in(D.obs_kp, A->obs_keypoint, 2 * no);
    S.in(D.obs_L, A->obs_sqrt_info, 4 * no);
    S.in(D.obs_pt, A->obs_point, 4 * no);
    const auto pose = S.inout(D.pose, A->pose, nullptr, 7 * nj);  // (written back per job, below)
    const auto real = S.out(D.out_real, nullptr, (size_t)kPlaceReal * nj);
    const auto ints = S.out(D.out_int, nullptr, (size_t)kPlaceInt * nj);
    c->beginBatch(S);
    c->uploadBatch(S);
    launch_place_refine(D, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    for (size_t j = 0; j < nj; ++j) {
      if (A->obs_begin[j + 1] > A->obs_begin[j]) std::memcpy(A->pose + 7 * j, S.host(pose) + 7 * j, 56);
      const double* r = S.host(real) + kPlaceReal * j;
      const int32_t* q = S.host(ints) + kPlaceInt * j;
      if (R->initial_cost) R->initial_cost[j] = r[0];
      if (R->final_cost) R->final_cost[j] = r[1];
      if (R->H) std::memcpy(R->H + 36 * j, r + 2, 36 * sizeof(double));
      if (R->num_iterations) R->num_iterations[j] = q[0];
      if (R->num_successful_steps) R->num_successful_steps[j] = q[1];
      if (R->num_unsuccessful_steps) R->num_unsuccessful_steps[j] = q[2];
      if (R->termination_type) R->termination_type[j] = q[3];
      if (R->n_outliers) R->n_outliers[j] = q[4];
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_twopose_compute(okvisgpu_ctx* c, const okvisgpu_twopose_edges* E, double* delta_x, double* sqrt_info,
                             double* lin_point, double* H00, double* b0) {
  if (!c || !E || E->n_edges < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "twopose_compute: bad arguments");
  if (E->n_edges == 0) return OKVISGPU_OK;
  if (!E->ref_pose || !E->other_pose || !E->landmark_begin || !E->obs_begin || !delta_x || !sqrt_info || !lin_point)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "twopose_compute: missing arrays");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    const size_t ne = (size_t)E->n_edges;
    TwoPoseDev T{};
    TwoPoseInputs I;
    BatchLayout S;
    declareTwoPose(E, "twopose_compute: ", S, T, I);
    const auto out = S.out(T.out, nullptr, (size_t)kTwoPoseOut * ne);
    c->beginBatch(S);
    c->uploadBatch(S);
    launch_twopose_compute(T, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    for (size_t e = 0; e < ne; ++e) {
      const double* r = S.host(out) + (size_t)kTwoPoseOut * e;
      std::memcpy(&delta_x[6 * e], r, 6 * 8);
      std::memcpy(&sqrt_info[36 * e], r + 6, 36 * 8);
      std::memcpy(&lin_point[7 * e], r + 42, 7 * 8);
      if (H00) std::memcpy(&H00[36 * e], r + 49, 36 * 8);
      if (b0) std::memcpy(&b0[6 * e], r + 85, 6 * 8);
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_twopose_extrinsics_compute(okvisgpu_ctx* c, const okvisgpu_twopose_edges* E, double* delta_x,
                                        double* sqrt_info, double* lin_point, uint8_t* camera_seen, double* H00,
                                        double* b0) {
  if (!c || !E || E->n_edges < 0 || E->n_cameras < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "twopose_extrinsics_compute: bad arguments");
  static_assert(kTwoPoseMaxCam == OKVISGPU_TWOPOSE_MAX_CAMERAS, "device bound and header bound differ");
  if (E->n_cameras > OKVISGPU_TWOPOSE_MAX_CAMERAS)
    return fail(c, OKVISGPU_ERR_UNSUPPORTED, "twopose_extrinsics_compute: more than OKVISGPU_TWOPOSE_MAX_CAMERAS cameras");
  if (E->n_edges == 0) return OKVISGPU_OK;
  if (!E->ref_pose || !E->other_pose || !E->landmark_begin || !E->obs_begin || !delta_x || !sqrt_info || !lin_point ||
      (E->n_cameras && !camera_seen))
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "twopose_extrinsics_compute: missing arrays");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    const size_t ne = (size_t)E->n_edges, nc = (size_t)E->n_cameras, D = 6 + 6 * nc;
    TwoPoseExtrDev X{};
    TwoPoseInputs I;
    BatchLayout S;
    declareTwoPose(E, "twopose_extrinsics_compute: ", S, X.in, I);
    S.scratch(X.obs_rec, (size_t)kTpxObsRec * I.no);
    S.scratch(X.obs_flag, I.no);
    S.scratch(X.lm_rec, (size_t)kTpxLmRec * I.nl);
    S.out(X.delta_x, delta_x, D * ne);
    S.out(X.sqrt_info, sqrt_info, D * D * ne);
    S.out(X.lin_point, lin_point, 7 * ne);
    S.out(X.H00, H00, D * D * ne);
    S.out(X.b0, b0, D * ne);
    S.out(X.seen, camera_seen, nc * ne);
    c->beginBatch(S);
    c->uploadBatch(S);
    // the outputs (all that is read back) zero-filled: the kernel writes the observed rows only
    HIPCHK(hipMemsetAsync(S.devBase() + S.downBegin(), 0, S.downEnd() - S.downBegin(), c->stream));
    launch_twopose_extr_compute(X, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_twopose_extrinsics_evaluate(okvisgpu_ctx* c, const okvisgpu_twopose_extrinsics_eval* V, double* r,
                                         double* J_ref, double* J_other, double* J_extrinsics) {
  if (!c || !V || V->n_edges < 0 || V->n_cameras < 0)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "twopose_extrinsics_evaluate: bad arguments");
  if (V->n_cameras > OKVISGPU_TWOPOSE_MAX_CAMERAS)
    return fail(c, OKVISGPU_ERR_UNSUPPORTED, "twopose_extrinsics_evaluate: more than OKVISGPU_TWOPOSE_MAX_CAMERAS cameras");
  if (V->n_edges == 0) return OKVISGPU_OK;
  if (!V->ref_pose || !V->other_pose || !V->delta_x || !V->sqrt_info || !V->lin_point ||
      (V->n_cameras && (!V->extrinsics || !V->lin_extrinsics || !V->camera_seen)))
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "twopose_extrinsics_evaluate: missing arrays");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    const size_t ne = (size_t)V->n_edges, nc = (size_t)V->n_cameras, D = 6 + 6 * nc;
    TwoPoseExtrEvalDev T{};
    T.n_edges = V->n_edges;
    T.n_cam = V->n_cameras;
    BatchLayout S;
    S.in(T.ref_pose, V->ref_pose, 7 * ne);
    S.in(T.other_pose, V->other_pose, 7 * ne);
    S.in(T.extr, V->extrinsics, 7 * nc);
    S.in(T.delta_x, V->delta_x, D * ne);
    S.in(T.sqrt_info, V->sqrt_info, D * D * ne);
    S.in(T.lin_point, V->lin_point, 7 * ne);
    S.in(T.lin_extr, V->lin_extrinsics, 7 * nc * ne);
    S.in(T.seen, V->camera_seen, nc * ne);
    if (r) S.out(T.r, r, D * ne);
    if (J_ref) S.out(T.J_ref, J_ref, 6 * D * ne);
    if (J_other) S.out(T.J_other, J_other, 6 * D * ne);
    if (J_extrinsics) S.out(T.J_extr, J_extrinsics, 6 * D * nc * ne);
    c->beginBatch(S);
    c->uploadBatch(S);
    launch_twopose_extr_eval(T, c->stream);
    HIPCHK(hipGetLastError());
    c->finishBatch(S);
    return (int)OKVISGPU_OK;
  });
}

}  // extern "C"
