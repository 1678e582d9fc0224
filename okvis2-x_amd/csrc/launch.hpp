// launch.hpp — host-side launchers of the gfx950 kernels (one stream, graph-capturable: no
// allocation, no synchronisation, no host reads inside any launcher). A launcher only launches:
// grids come from the descriptor's counts, and where the batch size picks a kernel form it reads
// the regime the runtime decided (DevProblem few / many / lin_prep / chol_schedule; launchRegime,
// plan.hpp). The order of an iteration's launches is the runtime's step table.
#pragma once

#include <hip/hip_runtime.h>

#include "device_problem.hpp"

namespace okg {

// evaluation (kernels_eval.hip); mode 0 current, 1 candidate, 2 initial, 3 initial without loss
void launch_eval(const DevProblem& P, int mode, hipStream_t s);      // few: launch_eval_few, else obs + imu
void launch_eval_few(const DevProblem& P, int mode, hipStream_t s);  // observations, IMU, priors, edges as one launch
void launch_eval_obs(const DevProblem& P, int mode, hipStream_t s);
void launch_eval_imu(const DevProblem& P, int mode, hipStream_t s);
void launch_eval_imu_as_solved(const DevProblem& P, int mode, hipStream_t s);  // (okvisgpu_time_kernel)
// ImuError::append for a batch (P: n_imu, imu_blocks {0, f, 0, f}, imu_t0 = old t1, imu_t1 = new t1,
// imu_sbegin / imu_ts / imu_ga = appended samples, imu_par (one row), imu_state, sb[0] = biases)
void launch_imu_append(const DevProblem& P, hipStream_t s);
// ImuError::propagation for a batch of independent items (kernels_imu_propagate.hip;
// okvisgpu_imu_propagate). Device arrays in the layout of okvisgpu_imu_propagate_batch; poses and sb
// are updated in place, steps [n] is always written (-1: samples do not reach t_end, nothing else
// of the item is written), cov / jac [n][225] row-major or nullptr. Neither: one lane per item;
// otherwise one 16-lane group per item, the covariance recursion only with cov.
struct ImuPropagateDev {
  int32_t n;
  double par[7];  // a_max, g_max, sigma_g_c, sigma_a_c, sigma_gw_c, sigma_aw_c, g
  double* poses;
  double* sb;
  const int64_t* t_start;
  const int64_t* t_end;
  const int32_t* sbegin;
  const int64_t* ts;
  const double* ga;
  double* cov;
  double* jac;
  int32_t* steps;
};
void launch_imu_propagate(const ImuPropagateDev& A, hipStream_t s);
// GpsErrorAsynchronous / GpsErrorSynchronous for a batch of factors (kernels_gps.hip;
// okvisgpu_gps_evaluate). Device arrays in the layout of okvisgpu_gps_batch / _result. kind 1 reads
// none of sb, t_k, t_g, the samples and state. gw_index and state may be nullptr (block 0; every
// factor fresh), and so may every output; an output that is set is written for every factor. Of
// state, a factor that re-integrates gets all kGpsState entries written, one that does not only its
// redo flag [1]. four_p: the covariance recursion on the reference's four dPdsigma matrices instead
// of their sigma-weighted sum (scripts/gps_timing.py's comparison; the entry point never sets it).
constexpr int kGpsState = 292;
struct GpsDev {
  int32_t n, kind, use_cov, redo_always, four_p;
  double par[7];  // a_max, g_max, sigma_g_c, sigma_a_c, sigma_gw_c, sigma_aw_c, g
  double r_SA[3];
  const double* poses;
  const double* sb;
  const double* T_GW;
  const int32_t* gw_index;
  const double* meas;
  const double* info;
  const int64_t* t_k;
  const int64_t* t_g;
  const int32_t* sbegin;
  const int64_t* ts;
  const double* ga;
  double* state;
  double* r;
  double* error;
  double* sqrt_info;
  double* J_pose;
  double* J_sb;
  double* J_gw;
  double* J_pose_amb;
  double* J_gw_amb;
  int32_t* steps;
};
void launch_gps_evaluate(const GpsDev& A, hipStream_t s);
// LidarMotionUndistortion::deskew / Trajectory::getStates for a batch of scans (kernels_lidar.hip;
// okvisgpu_lidar_deskew). Device arrays in the layout of okvisgpu_lidar_deskew_batch, plus q_scan
// [n_query] = the scan of every query. launch_lidar_chain: one lane per scan that has queries writes
// table [n_samples][kLidarRow] (Delta_q, acc_integral, acc_doubleintegral before every sample's
// interval; rows of a scan without queries are not written and not read). launch_lidar_points: one
// lane per query; every element of every output that is not nullptr is written. ray / pose_live /
// T_SL are read only when point or point_f64 is set.
constexpr int kLidarRow = 10;
struct LidarDeskewDev {
  int32_t n_scans, n_query;
  double g;
  const double* pose0;
  const double* sb0;
  const int64_t* t_start;
  const int32_t* sbegin;
  const int64_t* ts;
  const double* ga;
  const int32_t* qbegin;
  const int32_t* q_scan;
  const int64_t* qt;
  const double* ray;
  const double* pose_live;
  const double* T_SL;
  double* table;
  uint8_t* valid;
  float* point;
  double* point_f64;
  double* pose;
  double* speed;
  double* omega;
};
void launch_lidar_chain(const LidarDeskewDev& L, hipStream_t s);
void launch_lidar_points(const LidarDeskewDev& L, hipStream_t s);
// VoxelDownSample for a batch of clouds (kernels_lidar.hip; okvisgpu_voxel_downsample): the first
// point, in input order, of every (cloud, voxel). pt_cloud [n_points] = the cloud of every point,
// vsize [n_clouds] = float(voxel_size), use [n_points] or nullptr (all). table / best [table_size]
// (a power of two >= 2 n_points) and slot [n_points] are scratch; the three kernels write every
// element of table, best, slot, keep, n_kept and err [1] (non-zero: the probe ran out of slots).
struct VoxelDev {
  int32_t n_points, n_clouds, table_size;
  const int32_t* pt_cloud;
  const float* point;
  const float* vsize;
  const uint8_t* use;
  int32_t* table;
  int32_t* best;
  int32_t* slot;
  uint8_t* keep;
  int32_t* n_kept;
  int32_t* err;
};
void launch_voxel_downsample(const VoxelDev& V, hipStream_t s);
// ViSlamBackend::overlapFraction / trackingQuality and Frontend::doWeNeedANewKeyframe for a batch of jobs
// (kernels_overlap.hip; okvisgpu_frame_overlap). An item is one (job, side, image) whose two masks one
// workgroup paints in LDS: `other` = the frame whose id table decides "matched" (kind 0: the other
// side's, kind 1: frame A's, else unused), hw_off = the start of the half-width table of the item's R
// in hw (R + 1 entries), area = the pointArea of kind 3. kp_image [n_kp] = the image of every keypoint,
// img_frame / img_gr / img_gc / img_live [n_images] = its frame, grid rows, grid columns and whether it
// is non-empty, tab_begin [n_frames + 1] = the frame's region of table / live (a power of two of slots).
// The kernels write every element of table, live, count, n_matched, overlap, group_best, group_max and
// err [1] (non-zero: a probe ran out of slots); max_words = the largest G_r * ceil(G_c / 32) of an item.
struct OverlapItem {
  int32_t job, side, image, other, kind, R, hw_off, area;
};
struct OverlapDev {
  int32_t n_kp, n_items, n_jobs, n_groups, table_total, max_words;
  const int32_t* kp_begin;
  const int32_t* kp_image;
  const float* kp;
  const uint64_t* lm;
  const uint8_t* flag;
  const int32_t* img_frame;
  const int32_t* img_gr;
  const int32_t* img_gc;
  const uint8_t* img_live;
  const int32_t* tab_begin;
  const OverlapItem* items;
  const int32_t* hw;
  const int32_t* job_kind;
  const int32_t* group_begin;
  unsigned long long* table;
  uint8_t* live;
  int32_t* count;
  int32_t* n_matched;
  double* overlap;
  int32_t* group_best;
  double* group_max;
  int32_t* err;
};
void launch_frame_overlap(const OverlapDev& V, hipStream_t s);
// host-evaluated factors: gather the evaluation points (host_in), scatter the uploaded results
// (host_out) into the linearisation records; the host step between them is the runtime's
void launch_host_gather(const DevProblem& P, int mode, hipStream_t s);
void launch_host_scatter(const DevProblem& P, hipStream_t s);

// landmark / reduced-system kernels (kernels_schur.hip); lin_mode 0 = init, 1 = accepted only
void launch_lm_blocks(const DevProblem& P, int lin_mode, hipStream_t s);
void launch_imu_hess(const DevProblem& P, int lin_mode, hipStream_t s);
void launch_fgrad(const DevProblem& P, int lin_mode, hipStream_t s);
void launch_lm_prep(const DevProblem& P, hipStream_t s);
// few windows, after a step: landmark groups + IMU J^T J as one launch; with P.lin_prep also the GN
// prep of the windows not accepted, so the captured iteration does not start with it and the
// initial linearisation ends with it
void launch_lin_few(const DevProblem& P, hipStream_t s);
void launch_zero_S(const DevProblem& P, hipStream_t s);  // the non-zero tiles of S, once per build
void launch_assemble(const DevProblem& P, hipStream_t s);  // few: one launch, else pp + sb
void launch_lm_backsub(const DevProblem& P, hipStream_t s, bool storeY = false);  // kernels_backsub.hip: + landmark dogleg
                                                                               // vectors, J*v; storeY: y_l too
void launch_assemble_gradnorm_few(const DevProblem& P, hipStream_t s);  // few windows: + the gradient test
void launch_assemble_pp(const DevProblem& P, hipStream_t s);
void launch_assemble_sb(const DevProblem& P, hipStream_t s);
void launch_lm_visit(const DevProblem& P, int mode, hipStream_t s);  // 0/1: linearisation, 2: GN prep

// dense factorisation + both triangular solves, one persistent workgroup per window
// (kernels_chol.hip)
// static LDS of the persistent / the pipelined kernel (the window's solve vector comes on top as
// dynamic LDS); a value nothing fits if the query fails
size_t cholesky_persistent_lds();
size_t cholesky_pipe_lds();  // (kernels_chol_pipe.hip)
void launch_cholesky(const DevProblem& P, hipStream_t s);
void launch_cholesky_pipe(const DevProblem& P, hipStream_t s, bool split);
void launch_cholesky_split_b(const DevProblem& P, hipStream_t s);  // k_cholesky<2> (kernels_chol.hip)

// trust-region control (kernels_control.hip)
enum ReduceMode { R_COST_INIT = 0, R_COST_CAND = 1, R_JV = 2 };
void launch_reduce(const DevProblem& P, int mode, hipStream_t s);
void launch_jv(const DevProblem& P, hipStream_t s);  // (standalone, for okvisgpu_time_kernel; launch_lm_backsub includes it)
void launch_gradnorm(const DevProblem& P, int lin_mode, hipStream_t s);
void launch_dogleg(const DevProblem& P, hipStream_t s);
void launch_select_current(const DevProblem& P, hipStream_t s);  // set 1 -> set 0 where xcur == 1

// pose-graph edges (kernels_twopose.hip): TwoPoseStandardGraphError::compute, one wavefront per edge
void launch_twopose_compute(const TwoPoseDev& T, hipStream_t s);
// calibrating pose-graph edges (kernels_twopose_extr.hip): TwoPoseExtrinsicsGraphError::compute and
// ::EvaluateWithMinimalJacobians, one workgroup per edge
void launch_twopose_extr_compute(const TwoPoseExtrDev& T, hipStream_t s);
void launch_twopose_extr_eval(const TwoPoseExtrEvalDev& T, hipStream_t s);

// Frontend::matchToMap (kernels_match.hip; okvisgpu_match_to_map): the candidate tables of every
// (job, landmark), one lane each, then one wavefront per keypoint of the pass-0 and of the pass-1
// jobs. Every element of the tables and of the per-keypoint outputs is written.
void launch_match_prepare(const MatchDev& M, hipStream_t s);
void launch_match(const MatchDev& M, hipStream_t s);

// Frontend::matchMotionStereo / matchStereo (kernels_match_frames.hip; okvisgpu_match_frames): one lane
// per keypoint of either side and per job (rays in W, side 1's flag, the jobs' transforms; every
// per-keypoint output gets its no-match value), then one wavefront per participating side-0 keypoint
// of the mode-0 and of the mode-1 jobs.
void launch_match_frames_prepare(const FrameMatchDev& F, hipStream_t s);
void launch_match_frames(const FrameMatchDev& F, hipStream_t s);

// Frontend::verifyRecognisedPlace (kernels_place.hip). okvisgpu_place_match: one wavefront per (landmark,
// camera), every element of both outputs written. okvisgpu_place_refine: one workgroup per job runs the
// whole Levenberg-Marquardt solve and the evaluation after it; every element of the outputs written.
void launch_place_match(const PlaceMatchDev& M, hipStream_t s);
void launch_place_refine(const PlaceRefineDev& R, hipStream_t s);

// post-solve landmark pass (kernels_landmarks.hip): ViGraph::updateLandmarks on parameter set 0 (run
// launch_select_current first), one lane per landmark. Outputs in device order: quality [n_lm],
// flags [n_lm] (kLmInitialised | kLmReset | kLmNotInFront), obs_err [n_obs]; dirs [n_obs][3] is
// scratch. Re-placed landmarks are written to both parameter sets.
constexpr uint8_t kLmInitialised = 1, kLmReset = 2, kLmNotInFront = 4;
void launch_update_landmarks(const DevProblem& P, double* quality, uint8_t* flags, double* obs_err, double* dirs,
                             hipStream_t s);

// co-observation counts (kernels_covis.hip): ViGraph::computeCovisibilities as a Gram product of the
// window's 0/1 visibility matrix, counts[i][j] = popcount(v_i & v_j) on bit-vectors over the landmarks.
// One record per window that has states, landmarks and observations (the others are all zero and never
// reach the device); offsets are in elements of the batch-wide arrays.
struct CovisWin {
  int32_t lm_begin, n_lm;       // internal landmarks [lm_begin, lm_begin + n_lm)
  int32_t pose_begin, n_state;  // states = global poses [pose_begin, pose_begin + n_state): extrinsics blocks excluded
  int32_t word_begin, n_words;  // first 64-landmark word among all records' words; ceil(n_lm / 64)
  int32_t state_off, pad_;      // offset into n_observed
  int64_t bits_off;             // offset into bits, [n_state][n_words] state-major
  int64_t counts_off;           // offset into counts, [n_state][n_state] row-major
};
// The constant between the two count kernels: a window whose bitset, at its padded row stride
// covisRowStride(n_words), fits this many bytes of LDS is counted by one workgroup that holds all of it
// (path 0); a larger one by (state tile x state tile) workgroups streaming word chunks (path 1).
// 64 KiB of the CU's 160 KiB keeps two workgroups resident.
constexpr size_t kCovisLdsBudget = 64 * 1024;
constexpr int kCovisTile = 32;   // path 1: states per tile side
constexpr int kCovisChunk = 32;  // path 1: words per chunk
// LDS row stride in 64-bit words: odd, so the rows j, j + 1, ... a half-wave reads lie on distinct banks
constexpr int covisRowStride(int n_words) { return n_words | 1; }
constexpr size_t covisLdsBytes(int n_state, int n_words) { return 8 * (size_t)n_state * (size_t)covisRowStride(n_words); }
constexpr bool covisFitsLds(int n_state, int n_words) { return covisLdsBytes(n_state, n_words) <= kCovisLdsBudget; }
// bits: one wavefront per word; word_rec [n_words_total] = the record of each word (n_words_total = the
// sum of the records' n_words); excluded [P.n_lm] in internal order or nullptr (none). Every word of
// bits is written.
void launch_covis_bits(const DevProblem& P, const CovisWin* wins, int n_wins, const int32_t* word_rec, int n_words_total,
                       const uint8_t* excluded, unsigned long long* bits, hipStream_t s);
// counts: path 0 over items0 [n0] (record indices, lds_bytes = the largest covisLdsBytes among them),
// path 1 over items1 [n1][3] (record, row tile, column tile <= row tile). Every element of counts and
// n_observed of the listed records is written.
void launch_covis_counts(const CovisWin* wins, const int32_t* items0, int n0, size_t lds_bytes, const int32_t* items1,
                         int n1, const unsigned long long* bits, int32_t* counts, int32_t* n_observed, hipStream_t s);

}  // namespace okg
