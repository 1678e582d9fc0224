// plan.cpp — structure analysis of a batch of windows (plan.hpp): residual blocks, constant flags,
// Schur ordering with landmarks as e-blocks, the reduced-system contribution lists, the tile pattern
// of S with its launch schedule, and the arena layout. analyse() is a driver over named phases that
// share one WindowPlan; every phase appends to the HostBatch in window order, and the order of what
// it appends is part of the output (tests/test_plan_digest.py pins it bit for bit).
#include "plan.hpp"

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <stdexcept>

#include "loss.hpp"

namespace okg {

#ifdef OKG_ANALYSE_TIMING  // g_atime[i]: host ms spent before the i-th mark of analyse()'s window loop
double g_atime[kAnalysePhases];
std::chrono::steady_clock::time_point g_alast;
#define ATIME(i)                                                                    \
  g_atime[i] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_alast).count(); \
  g_alast = std::chrono::steady_clock::now();
#else
#define ATIME(i)
#endif

PlanOptions planOptions(int n_windows, int cu_count) {
  // nested-dissection order where the tile-parallel or the split persistent schedule will run
  // (below one window per CU, launchRegime): the chain of a window's factorisation is the
  // latency there.
  PlanOptions o;
  o.nd = belowOneWindowPerCu(n_windows, cu_count);
  // smaller landmark groups where a window's linearisation is a latency chain (fewWindows: one
  // workgroup per group, ~16 us of phases for a 256-visit group): 64 visits / 16 landmarks
  // (one S50 window: 36 -> 144 groups; steady iteration 0.3144 -> 0.3121 ms, S10 0.1580 ->
  // 0.1541 ms, profiles/r06_lmg_ab.txt).
  if (fewWindows(n_windows, cu_count)) { o.lmg_visits = 64; o.lmg_lms = 16; }
  return o;
}

LaunchRegime launchRegime(int n, int cu, bool any_split, bool persistent_fits, bool pipe_fits, int schedule,
                          int serial_override, int prep_override, int iters_override) {
  LaunchRegime r;
  r.few = fewWindows(n, cu);
  r.many = manyWindows(n);
  // Below one window per CU the graph is one stream (a cross-stream edge of the graph costs ~10 us,
  // more than the overlap of a single window's small kernels gains: S50 1488 -> 1614 it/s); a full
  // batch keeps the fork streams (2,048 S50 windows: 135.7k -> 138.5k window-it/s).
  r.serial_graph = serial_override >= 0 ? serial_override != 0 : belowOneWindowPerCu(n, cu);
  r.lin_prep = r.few && prep_override != 0;
  r.fused_gradnorm = r.few && r.serial_graph;
  // consecutive launches of one graph are ~8 us apart on the device (4.5 % of the S10 single-window
  // iteration; batches +0.2-0.3 %, r05bk)
  r.graph_iters = iters_override < 0 ? 4 : std::max(1, std::min(iters_override, 64));
  // Cholesky schedule (measured on MI355X, S50 windows, bench window-it/s, round 4 with the
  // nested-dissection order (nd) below one window per CU: 64 windows: schedule 1 65.2k, 2 (nd)
  // 72.2k; 128: 1 103.6k, 3 (nd) 107.9k, 2 (nd) 98.2k; 256: 1 159.7k, 3 (nd) 152.8k; 512: 1
  // 186.5k, 3 (nd) 166.0k; gpurun_out r04g / r04h nd_probe; round 5, the pipelined two-team
  // kernel (4), gpurun_out r05g: 64: 2 74.1k, 4 67.0k; 128: 3 110.1k, 4 105.7k; 256: 1 161.0k,
  // 4 170.1k; 512: 1 186.7k, 4 178.7k; the split schedule with pipelined parts (5), r05s: 64: 2
  // 73.9k, 3 70.4k, 5 73.7k; 128: 3 109.8k, 5 114.5k; 192: 4 133.6k, 3 127.3k, 5 120.7k; one S50
  // window: 2 2,765, 5 2,336, 3 2,233, 4 1,858 it/s): below half a window per CU the
  // tile-parallel launches spread each window over many CUs; at half a window per CU the split
  // schedule with each part pipelined; up to one window per CU the pipelined kernel (its step is
  // the factor plus one panel and one update); from there one persistent workgroup per window,
  // two per CU. (A wave-specialised kernel and a persistent variant with the panel tiles in LDS were
  // measured slower at every batch size and removed in round 4; a two-window pipelined
  // workgroup, round 5, ran 166.8k against 199.4k at 2,048 windows and was removed.)
  int s = schedule >= 1 && schedule <= 5 ? schedule
          : 2 * n < cu                   ? 2
          : 2 * n <= cu && any_split     ? 5
          : n <= cu                      ? 4
                                         : 1;
  if (s == 3 && !any_split) s = 1;  // (no window with a nested-dissection split)
  if (s == 5 && !any_split) s = 4;
  // the persistent kernels keep the window's rhs / y in dynamic LDS next to their static tiles:
  // a reduced dimension beyond what fits falls back, in the end to the tile-parallel launches
  if (s == 5 && !(pipe_fits && persistent_fits)) s = 3;
  if (s == 4 && !pipe_fits) s = 1;
  if ((s == 1 || s == 3) && !persistent_fits) s = 2;
  r.chol_schedule = s;
  return r;
}

// ---- tile-level symbolic factorisation and the tile-parallel launch schedule -------------------
// Fill of LLT inside the envelope, on the tile pattern nz (T x T, lower triangle).
void symbolicFill(std::vector<uint8_t>& nz, int T) {
  for (int k = 0; k < T; ++k)
    for (int i = k + 1; i < T; ++i)
      if (nz[(size_t)i * T + k])
        for (int j = k + 1; j <= i; ++j)
          if (nz[(size_t)j * T + k]) nz[(size_t)i * T + j] = 1;
}
// Launch schedule of the tile-parallel factorisation for a window's (filled) tile pattern: step k's
// band updates (tiles (i, j), k < j <= i, L_ik and L_jk non-zero) run in launch L[k] >= 1; launch 0
// factors the root tiles (those no update writes); any other tile is factored by the workgroup of
// its last update, so step k starts one launch after that; no tile is written by two updates of
// one launch. last[] holds each tile's last update launch (-1: none). For a block-banded pattern
// this is launch k + 1 for step k (the pre-round-4 schedule); for a nested-dissection order the
// independent parts share launches. Returns the number of launches.
int cholSchedule(const std::vector<uint8_t>& nz, int T, std::vector<int>& L, std::vector<int>& last) {
  L.assign(T, 0);
  last.assign((size_t)T * T, -1);
  int n = 1;
  for (int k = 0; k < T; ++k) {
    int lk = std::max(1, last[(size_t)k * T + k] + 1);
    bool any = false;
    for (int i = k + 1; i < T; ++i)
      if (nz[(size_t)i * T + k])
        for (int j = k + 1; j <= i; ++j)
          if (nz[(size_t)j * T + k]) {
            lk = std::max(lk, last[(size_t)i * T + j] + 1);
            any = true;
          }
    L[k] = lk;
    if (!any) continue;
    for (int i = k + 1; i < T; ++i)
      if (nz[(size_t)i * T + k])
        for (int j = k + 1; j <= i; ++j)
          if (nz[(size_t)j * T + k]) last[(size_t)i * T + j] = lk;
    n = std::max(n, lk + 1);
  }
  return n;
}

namespace {

template <class T>
void appendN(std::vector<T>& v, const T* src, size_t n) {
  if (n) v.insert(v.end(), src, src + n);
}

void validate(const okvisgpu_problem* p, int w) {
  auto bad = [&](const std::string& m) { throw ArgError{"window " + std::to_string(w) + ": " + m}; };
  if (p->n_poses < 0 || p->n_speed_biases < 0 || p->n_landmarks < 0 || p->n_observations < 0 || p->n_imu < 0 ||
      p->n_pose_priors < 0 || p->n_sb_priors < 0 || p->n_cameras < 0 || p->n_relpose < 0)
    bad("negative count");
  if (p->n_poses && !p->poses) bad("poses == NULL");
  if (p->n_speed_biases && !p->speed_biases) bad("speed_biases == NULL");
  if (p->n_landmarks && !p->landmarks) bad("landmarks == NULL");
  if (p->n_observations) {
    if (!p->obs_pose || !p->obs_landmark || !p->obs_camera || !p->obs_keypoint || !p->obs_sqrt_info)
      bad("observation arrays missing");
    if (!p->cameras || !p->extrinsics) bad("cameras / extrinsics missing");
    for (int o = 0; o < p->n_observations; ++o) {
      if (p->obs_pose[o] < 0 || p->obs_pose[o] >= p->n_poses) bad("obs_pose out of range");
      if (p->obs_landmark[o] < 0 || p->obs_landmark[o] >= p->n_landmarks) bad("obs_landmark out of range");
      if (p->obs_camera[o] < 0 || p->obs_camera[o] >= p->n_cameras) bad("obs_camera out of range");
    }
  }
  for (int c = 0; c < p->n_cameras; ++c)
    if (p->cameras[c].distortion < 0 || p->cameras[c].distortion > 3) bad("unknown distortion model");
  if (p->n_extrinsics_priors < 0) bad("negative count");
  if (p->n_extrinsics_priors && (!p->extrinsics_prior_camera || !p->extrinsics_prior_meas || !p->extrinsics_prior_sqrt_info))
    bad("extrinsics prior arrays missing");
  for (int i = 0; i < p->n_extrinsics_priors; ++i)
    if (p->extrinsics_prior_camera[i] < 0 || p->extrinsics_prior_camera[i] >= p->n_cameras)
      bad("extrinsics prior camera out of range");
  if (p->n_cameras && !p->extrinsics) bad("extrinsics == NULL");
  if (p->n_imu) {
    if (!p->imu_blocks || !p->imu_t0_ns || !p->imu_t1_ns || !p->imu_sample_begin || !p->imu_sample_t_ns ||
        !p->imu_sample_gyr_acc)
      bad("imu arrays missing");
    for (int f = 0; f < p->n_imu; ++f) {
      const int* b = &p->imu_blocks[4 * f];
      if (b[0] < 0 || b[0] >= p->n_poses || b[2] < 0 || b[2] >= p->n_poses || b[1] < 0 ||
          b[1] >= p->n_speed_biases || b[3] < 0 || b[3] >= p->n_speed_biases)
        bad("imu block index out of range");
      if (p->imu_sample_begin[f + 1] < p->imu_sample_begin[f]) bad("imu_sample_begin not monotone");
    }
  }
  for (int i = 0; i < p->n_pose_priors; ++i)
    if (p->pose_prior_block[i] < 0 || p->pose_prior_block[i] >= p->n_poses) bad("pose prior block out of range");
  for (int i = 0; i < p->n_sb_priors; ++i)
    if (p->sb_prior_block[i] < 0 || p->sb_prior_block[i] >= p->n_speed_biases) bad("sb prior block out of range");
  if (p->n_relpose) {
    if (!p->relpose_blocks || !p->relpose_delta_x || !p->relpose_sqrt_info || !p->relpose_lin_point)
      bad("relative-pose arrays missing");
    for (int i = 0; i < p->n_relpose; ++i) {
      const int a = p->relpose_blocks[2 * i], b = p->relpose_blocks[2 * i + 1];
      if (a < 0 || a >= p->n_poses || b < 0 || b >= p->n_poses) bad("relative-pose block out of range");
      if (a == b) bad("relative-pose edge connects a pose to itself");
      if (p->relpose_kind && p->relpose_kind[i] > 1) bad("unknown relative-pose kind");
    }
  }
  if (p->n_host < 0) bad("negative count");
  if (p->n_host) {
    if (!p->host_dim || !p->host_param_kind || !p->host_param_index || !p->host_evaluate)
      bad("host factor arrays / host_evaluate missing");
    for (int h = 0; h < p->n_host; ++h) {
      const std::string f = "host factor " + std::to_string(h) + ": ";
      if (p->host_dim[h] < 1 || p->host_dim[h] > OKVISGPU_HOST_MAX_RESIDUALS) bad(f + "residual dimension out of range");
      int np = 0, ns = 0, nb = 0;
      for (int k = 0; k < 4; ++k) {
        const int kind = p->host_param_kind[4 * h + k], idx = p->host_param_index[4 * h + k];
        if (kind < 0) break;
        ++nb;
        if (kind == 0) {
          if (idx < 0 || idx >= p->n_poses + p->n_cameras) bad(f + "pose-kind block out of range");
          ++np;
        } else if (kind == 1) {
          if (idx < 0 || idx >= p->n_speed_biases) bad(f + "speed/bias block out of range");
          ++ns;
        } else {
          throw UnsupportedError{"window " + std::to_string(w) + ": " + f +
                                 "only pose-kind and speed/bias blocks can be host-evaluated"};
        }
        for (int j = 0; j < k; ++j)
          if (p->host_param_kind[4 * h + j] == kind && p->host_param_index[4 * h + j] == idx)
            bad(f + "parameter block repeated");
        if (p->host_loss && !lossValid(p->host_loss[h])) bad(f + "unknown loss kind or non-positive loss scale");
      }
      for (int k = nb; k < 4; ++k)
        if (p->host_param_kind[4 * h + k] >= 0) bad(f + "parameter blocks must be leading (kind -1 = none)");
      if (nb == 0) bad(f + "no parameter block");
      if (np > 2 || ns > 2)
        throw UnsupportedError{"window " + std::to_string(w) + ": " + f +
                               "more than 2 pose-kind or 2 speed/bias blocks"};
    }
  }
}

// One level of nested dissection of a window's state slots (few windows: the latency of a solve is
// the chain of the tile-parallel launches). Slots [0, a) (left) and [b, n) (right) share no factor
// once the separator [a, b) is eliminated last: order left | right reversed | separator, left padded
// to a tile boundary in S, so the two parts factor as independent chains that each reach the
// separator only at their ends (the right part in natural order would touch it from its first
// tile on, and every step would write the separator's tiles). dim[u] = f scalars of slot u,
// reach[u] = largest slot coupled to u (landmarks seen from both, IMU links, edges, host factors).
// The split is chosen on the launch count of the estimated tile pattern (interval couplings);
// returns {-1, -1} unless it saves two launches or more with at most one tile more.
std::pair<int, int> chooseNd(const std::vector<int>& dim, const std::vector<int>& reach) {
  const int n = (int)dim.size();
  auto estimate = [&](int a, int b, int& tiles) {
    std::vector<int> order;  // (a = 0: the natural order)
    for (int u = 0; u < (a > 0 ? a : n); ++u) order.push_back(u);
    if (a > 0) {
      for (int u = n - 1; u >= b; --u) order.push_back(u);
      for (int u = a; u < b; ++u) order.push_back(u);
    }
    std::vector<int> off(n, 0);
    int o = 0;
    for (int t = 0; t < n; ++t) {
      if (t == a && a > 0 && a < n) o = pad64(o);
      off[order[t]] = o;
      o += dim[order[t]];
    }
    const int T = std::max(1, pad64(o) / kTile);
    tiles = T;
    std::vector<uint8_t> nz((size_t)T * T, 0);
    for (int i = 0; i < T; ++i) nz[(size_t)i * T + i] = 1;
    for (int u = 0; u < n; ++u) {
      if (!dim[u]) continue;
      for (int v = u; v <= reach[u]; ++v) {
        if (!dim[v]) continue;
        for (int ti = off[u] / kTile; ti <= (off[u] + dim[u] - 1) / kTile; ++ti)
          for (int tj = off[v] / kTile; tj <= (off[v] + dim[v] - 1) / kTile; ++tj)
            nz[(size_t)std::max(ti, tj) * T + std::min(ti, tj)] = 1;
      }
    }
    symbolicFill(nz, T);
    std::vector<int> L, last;
    return cholSchedule(nz, T, L, last);
  };
  int t0 = 0;
  const int base = estimate(0, 0, t0);
  std::vector<int> pm(n + 1, -1);
  for (int u = 0; u < n; ++u) pm[u + 1] = std::max(pm[u], reach[u]);
  int best = base, ba = -1, bb = -1;
  const int stride = n > 64 ? n / 32 : 1;
  for (int a = std::max(1, n > 64 ? n / 4 : 1); a < (n > 64 ? 3 * n / 4 : n - 1); a += stride) {
    const int b = std::max(a, pm[a] + 1);
    if (b >= n) continue;
    int t = 0;
    const int lv = estimate(a, b, t);
    if (t <= t0 + 1 && lv < best) {
      best = lv;
      ba = a;
      bb = b;
    }
  }
  return best <= base - 2 ? std::make_pair(ba, bb) : std::make_pair(-1, -1);
}

// The planner's state for one window: what the phases hand to one another. Constructed once and
// reused for every window of the batch (the vectors keep their capacity). Each phase appends the
// window's part of the HostBatch arrays named in its comment.
struct WindowPlan {
  HostBatch& B;
  const std::map<std::tuple<int, int, int>, int>& constOverride;
  int w = 0;
  const okvisgpu_problem* p = nullptr;
  // begin(): the window's bases in the batch arrays and its block counts. pose-kind blocks of the
  // window: the states' poses [0, np), then one extrinsics block per camera [np, np + ncam)
  // (okvis: PoseParameterBlocks with the PoseManifold, ViGraph.cpp:330-336)
  int pb = 0, sbb = 0, lb = 0, cb = 0, ob = 0, ib = 0, ppb = 0, sbpb = 0, rpb = 0;
  int np = 0, ncam = 0, npx = 0, nmax = 0;
  // params(): constant flags per block; landmark permutation (internal k = caller's perm[k]) and inverse
  std::vector<uint8_t> pc, sc, lc;
  std::vector<int> perm, inv, firstPose;
  // flags(): active blocks (free and used), residual blocks whose blocks are all constant, the
  // pose priors (states' then extrinsics'), host factors' slot blocks
  std::vector<uint8_t> pa, sa, la, ofix, ifix, rfix, hfix;
  struct PPrior { int blk; const double* meas; const double* L; };
  std::vector<PPrior> pps;
  int hfBase = 0, hgBase = 0;  // first host factor of the window in B.hf / as a global factor index
  std::vector<std::array<int, 4>> hslot;
  // stateOrder(): slot order (nested dissection: left | right reversed | separator), f offset and
  // f-block of every pose-kind / speed-bias block (-1: not free), the order's positions
  std::vector<int> slotOrder, posef, sbf, poseFb, sbFb, lmLo, lmHi;  // (lmLo / lmHi: chooseSlotOrder() scratch)
  int ndLeft = 0, ndSep = 0;  // slots of the left part (0: natural order); order index of the separator
  int gapAt = 0, gap = 0, rightAt = 0, sepAt = 0;
  int fbBase = 0, fo = 0, fpad = 0;
  bool extFree = false;
  std::vector<uint8_t> laNew;  // la in internal landmark order
  // sortObservations(), visits(), extrinsicVisits()
  std::vector<int> order, start, fill, vcount, lmVisitBegin, lmXBegin, freeCams;
  std::vector<int32_t> xobs;
  // groups(): segments per pose-kind block, f-block pair of each partial block of this window
  std::vector<std::vector<int>> segsAtPose;
  std::vector<std::pair<int, int>> partKeys;
  int partBase = 0;
  std::vector<std::pair<int, int>> mem, gitems, gprod;  // closeGroup() scratch
  std::vector<int> glocal, gcount, gfill, fbLocal;
  std::vector<int32_t> gsorted;
  // contributions(): per f-block (gradient / diagonal) and per f-block pair (fi >= fj by reduced offset)
  std::vector<std::vector<Contrib>> fbc;
  std::map<std::pair<int, int>, std::vector<Contrib>> pairs;

  bool isConst(int kind, int idx, const uint8_t* flags) const {
    auto it = constOverride.find(std::make_tuple(w, kind, idx));
    if (it != constOverride.end()) return it->second != 0;
    return flags ? flags[idx] != 0 : false;
  }
  // the phases, in analyse()'s order (closeGroup and emitFactor: helpers of groups and contributions)
  void begin(int window, const okvisgpu_problem* problem);
  void params(), flags(), chooseSlotOrder(), stateOrder(), sortObservations(), visits(), extrinsicVisits();
  void closeGroup(int gl0, int gl1), groups(), factorArrays();
  void emitFactor(int type, int index, const int* fbs, const int* cols, int n), contributions();
  void tilePattern(), emitPairs();
};

void WindowPlan::begin(int window, const okvisgpu_problem* problem) {
  w = window;
  p = problem;
  validate(p, w);
  pb = (int)B.pose_win.size(); sbb = (int)B.sb_win.size(); lb = (int)B.lm_win.size();
  cb = (int)(B.cam.size() / kCamDoubles); ob = (int)B.obs_win.size(); ib = (int)B.imu_win.size();
  ppb = (int)B.pp_win.size(); sbpb = (int)B.sbp_win.size(); rpb = (int)B.rp_win.size();
  B.pose_base.push_back(pb); B.sb_base.push_back(sbb); B.lm_base.push_back(lb);
  B.obs_base.push_back(ob); B.imu_base.push_back(ib); B.rp_base.push_back(rpb);
  np = p->n_poses; ncam = p->n_cameras; npx = np + ncam;
  nmax = std::max(p->n_poses, p->n_speed_biases);
}

// constant flags; pose, sb, lm (permuted), cam, extr, cam_pose, lm_perm, *_win
void WindowPlan::params() {
  pc.resize(npx); sc.resize(p->n_speed_biases); lc.resize(p->n_landmarks);
  for (int i = 0; i < np; ++i) pc[i] = isConst(0, i, p->pose_constant);
  for (int c = 0; c < ncam; ++c) {  // constant unless flagged variable (do_extrinsics: false)
    auto it = constOverride.find(std::make_tuple(w, 3, c));
    pc[np + c] = it != constOverride.end() ? it->second != 0
                                           : (p->extrinsics_constant ? p->extrinsics_constant[c] != 0 : 1);
  }
  for (int i = 0; i < p->n_speed_biases; ++i) sc[i] = isConst(1, i, p->speed_bias_constant);
  for (int i = 0; i < p->n_landmarks; ++i) lc[i] = isConst(2, i, p->landmark_constant);
  appendN(B.pose, p->poses, (size_t)7 * p->n_poses);
  appendN(B.pose, p->extrinsics, (size_t)7 * ncam);
  appendN(B.sb, p->speed_biases, (size_t)9 * p->n_speed_biases);
  // internal landmark order: by first observing pose (then caller order), so that the visits of
  // neighbouring keyframes are close in memory whatever order the caller numbers landmarks in
  // (okvis numbers them by creation, which is nearly this order already)
  perm.resize(p->n_landmarks); inv.resize(p->n_landmarks);
  firstPose.assign(p->n_landmarks, p->n_poses);
  for (int o = 0; o < p->n_observations; ++o)
    firstPose[p->obs_landmark[o]] = std::min(firstPose[p->obs_landmark[o]], p->obs_pose[o]);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return firstPose[a] < firstPose[b]; });
  for (int k = 0; k < p->n_landmarks; ++k) inv[perm[k]] = k;
  for (int k = 0; k < p->n_landmarks; ++k) {
    appendN(B.lm, &p->landmarks[4 * (size_t)perm[k]], 4);
    B.lm_perm.push_back(perm[k]);
  }
  for (int c = 0; c < p->n_cameras; ++c) {
    const okvisgpu_camera& k = p->cameras[c];
    const double cv[kCamDoubles] = {(double)k.distortion, k.fu, k.fv, k.cu, k.cv, k.dist[0], k.dist[1],
                                    k.dist[2], k.dist[3], k.dist[4], k.dist[5], k.dist[6], k.dist[7]};
    appendN(B.cam, cv, kCamDoubles);
    appendN(B.extr, &p->extrinsics[7 * c], 7);
    B.cam_pose.push_back(pb + np + c);
  }
  for (int i = 0; i < npx; ++i) B.pose_win.push_back(w);
  for (int i = 0; i < p->n_speed_biases; ++i) B.sb_win.push_back(w);
  for (int i = 0; i < p->n_landmarks; ++i) B.lm_win.push_back(w);
}

// active blocks: free and used by a residual block that is not entirely constant; hf
void WindowPlan::flags() {
  pa.assign(npx, 0); sa.assign(p->n_speed_biases, 0); la.assign(p->n_landmarks, 0);
  ofix.resize(p->n_observations); ifix.resize(p->n_imu);
  for (int o = 0; o < p->n_observations; ++o) {
    const int ps = p->obs_pose[o], l = p->obs_landmark[o], xe = np + p->obs_camera[o];
    ofix[o] = pc[ps] && lc[l] && pc[xe];
    if (!pc[ps]) pa[ps] = 1;
    if (!lc[l]) la[l] = 1;
    if (!pc[xe]) pa[xe] = 1;
  }
  for (int f = 0; f < p->n_imu; ++f) {
    const int* b = &p->imu_blocks[4 * f];
    ifix[f] = pc[b[0]] && sc[b[1]] && pc[b[2]] && sc[b[3]];
    if (!pc[b[0]]) pa[b[0]] = 1;
    if (!sc[b[1]]) sa[b[1]] = 1;
    if (!pc[b[2]]) pa[b[2]] = 1;
    if (!sc[b[3]]) sa[b[3]] = 1;
  }
  // PoseError priors on pose-kind blocks: the states' (pose_prior_*) then the extrinsics'
  // (extrinsics_prior_*, ViGraph.cpp:372-382), one prior list on the device
  pps.clear();
  for (int i = 0; i < p->n_pose_priors; ++i)
    pps.push_back(PPrior{p->pose_prior_block[i], &p->pose_prior_meas[7 * i], &p->pose_prior_sqrt_info[36 * i]});
  for (int i = 0; i < p->n_extrinsics_priors; ++i)
    pps.push_back(PPrior{np + p->extrinsics_prior_camera[i], &p->extrinsics_prior_meas[7 * i],
                         &p->extrinsics_prior_sqrt_info[36 * i]});
  for (const PPrior& q : pps)
    if (!pc[q.blk]) pa[q.blk] = 1;
  for (int i = 0; i < p->n_sb_priors; ++i)
    if (!sc[p->sb_prior_block[i]]) sa[p->sb_prior_block[i]] = 1;
  rfix.resize(p->n_relpose);
  for (int i = 0; i < p->n_relpose; ++i) {
    const int a = p->relpose_blocks[2 * i], b = p->relpose_blocks[2 * i + 1];
    rfix[i] = pc[a] && pc[b];
    if (!pc[a]) pa[a] = 1;
    if (!pc[b]) pa[b] = 1;
  }
  // host-evaluated factors: IMU-layout slots (pose-kind blocks fill slots 0 then 2, speed/bias
  // blocks 1 then 3, in the functor's order) and window-local block per slot (-1 unused)
  hfBase = (int)B.hf.size();
  hgBase = B.n_imu_total + hfBase;
  hslot.resize(p->n_host);
  hfix.resize(p->n_host);
  for (int h = 0; h < p->n_host; ++h) {
    HostBatch::HostFactor F{w, h, 0, p->host_dim[h], {-1, -1, -1, -1}, hostLoss(p, h)};
    std::array<int, 4>& s = hslot[h];
    s = {-1, -1, -1, -1};
    int npk = 0, nsb = 0;
    bool allConst = true;
    for (int k = 0; k < 4 && p->host_param_kind[4 * h + k] >= 0; ++k) {
      const int kind = p->host_param_kind[4 * h + k], idx = p->host_param_index[4 * h + k];
      const int q = kind == 0 ? 2 * npk++ : 1 + 2 * nsb++;
      F.slot[k] = (int8_t)q;
      F.np = k + 1;
      s[q] = idx;
      const bool c = kind == 0 ? pc[idx] != 0 : sc[idx] != 0;
      allConst = allConst && c;
      if (!c) (kind == 0 ? pa[idx] : sa[idx]) = 1;
    }
    hfix[h] = allConst;
    B.hf.push_back(F);
  }
}

// For the tile-parallel schedule (few windows): a nested-dissection order of the state slots where
// chooseNd finds one, from the couplings of the window's residual blocks.
void WindowPlan::chooseSlotOrder() {
  slotOrder.resize(nmax);
  std::iota(slotOrder.begin(), slotOrder.end(), 0);
  ndLeft = ndSep = 0;
  extFree = std::any_of(pa.begin() + np, pa.end(), [](uint8_t a) { return a != 0; });
  if (!B.opt.nd || extFree || nmax < 8) return;  // (variable extrinsics couple every state: no split)
  std::vector<int> dim(nmax, 0), reach(nmax);
  for (int i = 0; i < nmax; ++i) {
    dim[i] = (i < p->n_poses && pa[i] ? 6 : 0) + (i < p->n_speed_biases && sa[i] ? 9 : 0);
    reach[i] = i;
  }
  auto couple = [&](int lo, int hi) {
    if (lo >= 0 && hi > lo) reach[lo] = std::max(reach[lo], hi);
  };
  {  // landmarks: the free poses observing a free landmark are coupled by its elimination
    std::vector<int>&lo = lmLo, &hi = lmHi;
    lo.assign(p->n_landmarks, INT_MAX);
    hi.assign(p->n_landmarks, -1);
    for (int o = 0; o < p->n_observations; ++o) {
      const int l = p->obs_landmark[o], ps = p->obs_pose[o];
      if (!la[l] || !pa[ps]) continue;
      lo[l] = std::min(lo[l], ps);
      hi[l] = std::max(hi[l], ps);
    }
    for (int l = 0; l < p->n_landmarks; ++l)
      if (hi[l] >= 0) couple(lo[l], hi[l]);
  }
  auto coupleSet = [&](std::initializer_list<int> slots) {
    int lo = INT_MAX, hi = -1;
    for (int u : slots)
      if (u >= 0) { lo = std::min(lo, u); hi = std::max(hi, u); }
    if (hi >= 0) couple(lo, hi);
  };
  for (int f = 0; f < p->n_imu; ++f) {
    const int* b = &p->imu_blocks[4 * f];
    coupleSet({pa[b[0]] ? b[0] : -1, sa[b[1]] ? b[1] : -1, pa[b[2]] ? b[2] : -1, sa[b[3]] ? b[3] : -1});
  }
  for (int i = 0; i < p->n_relpose; ++i) {
    const int a = p->relpose_blocks[2 * i], b = p->relpose_blocks[2 * i + 1];
    coupleSet({a < np && pa[a] ? a : -1, b < np && pa[b] ? b : -1});
  }
  for (int h = 0; h < p->n_host; ++h) {
    int lo = INT_MAX, hi = -1;
    for (int k = 0; k < 4 && p->host_param_kind[4 * h + k] >= 0; ++k) {
      const int kind = p->host_param_kind[4 * h + k], idx = p->host_param_index[4 * h + k];
      const bool act = kind == 0 ? (idx < np && pa[idx]) : sa[idx] != 0;
      if (act) { lo = std::min(lo, idx); hi = std::max(hi, idx); }
    }
    if (hi >= 0) couple(lo, hi);
  }
  const auto ab = chooseNd(dim, reach);
  if (ab.first > 0) {
    slotOrder.clear();
    for (int u = 0; u < ab.first; ++u) slotOrder.push_back(u);
    for (int u = nmax - 1; u >= ab.second; --u) slotOrder.push_back(u);
    for (int u = ab.first; u < ab.second; ++u) slotOrder.push_back(u);
    ndLeft = ab.first;
    ndSep = ab.first + (nmax - ab.second);
  }
}

// f-blocks in the reduced ordering: pose i, then speed/bias i, state slot by slot in slotOrder;
// fb_*, win_ext_free, win_sgap, f_nat, win_fnat, pose_f, sb_f, *_active, lm_free, win_f*, win_*off
void WindowPlan::stateOrder() {
  posef.assign(npx, -1); sbf.assign(p->n_speed_biases, -1); poseFb.assign(npx, -1); sbFb.assign(p->n_speed_biases, -1);
  fo = 0;
  fbBase = (int)B.fb_win.size();
  // (nested dissection: the left part ends on a tile boundary; the gap rows between are identity
  // rows of S with zero rhs, so the f-vector and S share one index)
  gapAt = gap = rightAt = sepAt = 0;
  auto addFb = [&](int kind, int index, int n, int& f, int& fb) {  // the next f-block: n scalars at fo
    f = fo;
    fb = (int)B.fb_win.size();
    B.fb_win.push_back(w); B.fb_kind.push_back(kind); B.fb_index.push_back(index); B.fb_off.push_back(fo);
    fo += n;
  };
  for (int t = 0; t < nmax; ++t) {
    const int i = slotOrder[t];
    if (ndLeft && t == ndLeft) {
      gapAt = fo;
      fo = pad64(fo);
      gap = fo - gapAt;
      rightAt = fo;
    }
    if (ndLeft && t == ndSep) sepAt = fo;
    if (i < p->n_poses && pa[i]) addFb(0, pb + i, 6, posef[i], poseFb[i]);
    if (i < p->n_speed_biases && sa[i]) addFb(1, sbb + i, 9, sbf[i], sbFb[i]);
  }
  // variable extrinsics after all states: S keeps the states' band plus a dense border
  for (int i = np; i < npx; ++i)
    if (pa[i]) addFb(0, pb + i, 6, posef[i], poseFb[i]);
  B.win_ext_free.push_back(fo > 0 && extFree);
  B.win_sgap.push_back(gap ? gapAt : 0); B.win_sgap.push_back(gap);
  // natural order of the f entries (pose i, speed/bias i slot by slot, then extrinsics: the order
  // of okvisgpu_linearize_reduce's export and of the oracle)
  {
    const size_t nat0 = B.f_nat.size();
    B.f_nat.resize(nat0 + fo, -1);
    int32_t* nat = B.f_nat.data() + nat0;
    int no = 0;
    auto put = [&](int f, int n) {
      for (int c = 0; c < n; ++c) nat[f + c] = no++;
    };
    for (int i = 0; i < nmax; ++i) {
      if (i < p->n_poses && posef[i] >= 0) put(posef[i], 6);
      if (i < p->n_speed_biases && sbf[i] >= 0) put(sbf[i], 9);
    }
    for (int c = 0; c < ncam; ++c)
      if (posef[np + c] >= 0) put(posef[np + c], 6);
    B.win_fnat.push_back(no);
  }
  for (int i = 0; i < npx; ++i) { B.pose_f.push_back(posef[i]); B.pose_active.push_back(pa[i]); }
  for (int i = 0; i < p->n_speed_biases; ++i) { B.sb_f.push_back(sbf[i]); B.sb_active.push_back(sa[i]); }
  laNew.resize(p->n_landmarks);
  for (int k = 0; k < p->n_landmarks; ++k) B.lm_free.push_back(laNew[k] = la[perm[k]]);
  fpad = pad64(fo);  // S dimension (leading dimension of the window's S)
  B.win_foff.push_back(B.f_total); B.win_fdim.push_back(fo); B.win_fpad.push_back(fpad);
  B.win_soff.push_back(B.s_total); B.win_linvoff.push_back(B.linv_total); B.win_fwdoff.push_back(B.fwd_total);
  B.fwd_total += fpad;
  B.f_total += fo;
  B.s_total += (int64_t)fpad * fpad;
  B.linv_total += (int64_t)(fpad / kTile) * kTile * kTile;
  B.max_fpad = std::max(B.max_fpad, fpad);
}

// observations sorted by (internal landmark, pose, camera, original index)
// (counting sort by landmark, then insertion sort of each landmark's few observations: the
// order of a stable sort on that key, in linear time)
void WindowPlan::sortObservations() {
  order.resize(p->n_observations);
  start.assign(p->n_landmarks + 1, 0);
  for (int o = 0; o < p->n_observations; ++o) ++start[inv[p->obs_landmark[o]] + 1];
  for (int l = 0; l < p->n_landmarks; ++l) start[l + 1] += start[l];
  fill.assign(start.begin(), start.end() - 1);
  for (int o = 0; o < p->n_observations; ++o) order[fill[inv[p->obs_landmark[o]]]++] = o;
  auto before = [&](int a, int b) {
    if (p->obs_pose[a] != p->obs_pose[b]) return p->obs_pose[a] < p->obs_pose[b];
    if (p->obs_camera[a] != p->obs_camera[b]) return p->obs_camera[a] < p->obs_camera[b];
    return a < b;
  };
  for (int l = 0; l < p->n_landmarks; ++l)
    for (int i = start[l] + 1; i < start[l + 1]; ++i) {
      const int x = order[i];
      int j = i - 1;
      for (; j >= start[l] && before(x, order[j]); --j) order[j + 1] = order[j];
      order[j + 1] = x;
    }
}

// visits and landmark -> visit ranges; obs_*, visit_pose, visit_lm, visit_obs_begin, lm_visit_begin
void WindowPlan::visits() {
  int acc = (int)B.visit_pose.size();  // the window's first visit
  lmVisitBegin.assign(p->n_landmarks + 1, 0);
  int prevL = -1, prevP = -1;
  vcount.assign(p->n_landmarks, 0);
  // per-observation arrays written in place (sized once; push_back per element dominated)
  const size_t nob = (size_t)p->n_observations;
  for (auto* v : {&B.obs_pose, &B.obs_lm, &B.obs_cam, &B.obs_win, &B.obs_orig}) v->resize(ob + nob);
  B.obs_flags.resize(ob + nob);
  B.obs_kp.resize(2 * (ob + nob));
  B.obs_L.resize(4 * (ob + nob));
  int32_t *oPose = B.obs_pose.data() + ob, *oLm = B.obs_lm.data() + ob, *oCam = B.obs_cam.data() + ob,
          *oWin = B.obs_win.data() + ob, *oOrig = B.obs_orig.data() + ob;
  uint8_t* oFl = B.obs_flags.data() + ob;
  double *oKp = B.obs_kp.data() + 2 * (size_t)ob, *oL = B.obs_L.data() + 4 * (size_t)ob;
  for (int k = 0; k < p->n_observations; ++k) {
    const int o = order[k];
    const int l = inv[p->obs_landmark[o]], ps = p->obs_pose[o], cam = p->obs_camera[o];
    oPose[k] = pb + ps;
    oLm[k] = lb + l;
    oCam[k] = cb + cam;
    oWin[k] = w;
    oOrig[k] = o;
    uint8_t fl = 0;
    if (p->obs_cauchy ? p->obs_cauchy[o] != 0 : true) fl |= 1;
    if (ofix[o]) fl |= 2;
    if (posef[np + cam] >= 0) fl |= 4;  // variable extrinsics
    oFl[k] = fl;
    oKp[2 * k] = p->obs_keypoint[2 * o];
    oKp[2 * k + 1] = p->obs_keypoint[2 * o + 1];
    for (int i = 0; i < 4; ++i) oL[4 * k + i] = p->obs_sqrt_info[4 * o + i];
    if (l != prevL || ps != prevP) {
      B.visit_pose.push_back(pb + ps);
      B.visit_lm.push_back(lb + l);
      B.visit_obs_begin.push_back(ob + k);
      vcount[l]++;
      prevL = l;
      prevP = ps;
    }
  }
  for (int l = 0; l < p->n_landmarks; ++l) {
    B.lm_visit_begin.push_back(lmVisitBegin[l] = acc);
    acc += vcount[l];
  }
  lmVisitBegin[p->n_landmarks] = acc;
}

// extrinsic visits: per landmark and variable camera, the landmark's (non-fixed) observations
// through that camera (the extrinsics block is the third parameter block of their
// ReprojectionErrors); global indices, in landmark order like the visits; xvisit_*
void WindowPlan::extrinsicVisits() {
  lmXBegin.assign(p->n_landmarks + 1, (int)B.xvisit_pose.size());
  freeCams.clear();
  for (int c = 0; c < ncam; ++c)
    if (posef[np + c] >= 0) freeCams.push_back(c);
  int k = 0;
  for (int l = 0; l < p->n_landmarks; ++l) {
    lmXBegin[l] = (int)B.xvisit_pose.size();
    const int k0 = k;
    while (k < p->n_observations && inv[p->obs_landmark[order[k]]] == l) ++k;
    for (int c : freeCams) {
      xobs.clear();
      for (int j = k0; j < k; ++j)
        if (p->obs_camera[order[j]] == c && !ofix[order[j]]) xobs.push_back(ob + j);
      if (xobs.empty()) continue;
      B.xvisit_pose.push_back(pb + np + c);
      B.xvisit_lm.push_back(lb + l);
      B.xvisit_obs_begin.push_back((int32_t)B.xvisit_obs.size());
      B.xvisit_obs.insert(B.xvisit_obs.end(), xobs.begin(), xobs.end());
      B.xvisit_slot.push_back(-1);
    }
  }
  lmXBegin[p->n_landmarks] = (int)B.xvisit_pose.size();
}

// One landmark group [gl0, gl1) (internal landmarks of this window): its visit segments and
// partial Schur blocks; seg_*, visit_slot, xvisit_slot, part_*, lmg_begin, lmg_xbegin.
// Each visit of a free pose gets the slot of its position in the group's (pose, visit) order, so a
// segment is a contiguous slot range [seg_range.x, seg_range.y). A group's threads: its pose visits
// first (thread t = v - gv0), then its extrinsic visits (thread t = nvg + xv - gx0).
void WindowPlan::closeGroup(int gl0, int gl1) {
  const int gv0 = lmVisitBegin[gl0], gv1 = lmVisitBegin[gl1], nvg = gv1 - gv0;
  const int gx0 = lmXBegin[gl0], gx1 = lmXBegin[gl1];
  // members (v >= 0 visit, -1 - xv extrinsic visit) grouped by pose-kind block, ascending,
  // each block's members in visit order
  mem.clear();
  for (int v = gv0; v < gv1; ++v) {
    const int ps = B.visit_pose[v] - pb;
    if (posef[ps] >= 0) mem.push_back({ps, v});
    else B.visit_slot[v] = -1;
  }
  for (int xv = gx0; xv < gx1; ++xv) mem.push_back({B.xvisit_pose[xv] - pb, -1 - xv});
  std::stable_sort(mem.begin(), mem.end(),
                   [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
  int slot = 0;
  for (size_t m = 0; m < mem.size();) {
    const int ps = mem[m].first;
    segsAtPose[ps].push_back((int)B.seg_pose.size());
    B.seg_pose.push_back(pb + ps);
    B.seg_range.push_back(slot);
    for (; m < mem.size() && mem[m].first == ps; ++m) {
      const int v = mem[m].second;
      if (v >= 0) B.visit_slot[v] = slot++;
      else B.xvisit_slot[-1 - v] = slot++;
    }
    B.seg_range.push_back(slot);
  }
  // partial Schur blocks (k_lm_visit): per f-block pair (row >= col by f offset) the products
  // Z_a Z_b^T of the group's free landmarks; contributions packed as (a | b << 16), thread
  // offsets within the group
  // products keyed by f-block pair, in (row f-block, col f-block) order, each key's products
  // in generation order: the group's f-blocks get dense local indices in ascending order and
  // the products are counting-sorted by (local row, local col)
  std::vector<std::pair<int, int>>& items = gitems;  // (thread, f-block) of one landmark's free visits
  glocal.clear();
  for (int v = gv0; v < gv1; ++v)
    if (laNew[B.visit_lm[v] - lb] && poseFb[B.visit_pose[v] - pb] >= 0) glocal.push_back(poseFb[B.visit_pose[v] - pb]);
  for (int xv = gx0; xv < gx1; ++xv)
    if (laNew[B.xvisit_lm[xv] - lb]) glocal.push_back(poseFb[B.xvisit_pose[xv] - pb]);
  std::sort(glocal.begin(), glocal.end());
  glocal.erase(std::unique(glocal.begin(), glocal.end()), glocal.end());
  const int nloc = (int)glocal.size();
  for (int i = 0; i < nloc; ++i) fbLocal[glocal[i]] = i;
  gprod.clear();
  for (int l = gl0; l < gl1; ++l) {
    if (!laNew[l]) continue;
    items.clear();
    for (int va = lmVisitBegin[l]; va < lmVisitBegin[l + 1]; ++va) {
      const int fa = poseFb[B.visit_pose[va] - pb];
      if (fa >= 0) items.push_back({va - gv0, fa});
    }
    for (int xv = lmXBegin[l]; xv < lmXBegin[l + 1]; ++xv)
      items.push_back({nvg + xv - gx0, poseFb[B.xvisit_pose[xv] - pb]});
    for (const auto& a : items)
      for (const auto& b : items) {
        if (B.fb_off[a.second] < B.fb_off[b.second]) continue;
        gprod.push_back({fbLocal[a.second] * nloc + fbLocal[b.second], a.first | (b.first << 16)});
      }
  }
  gcount.assign((size_t)nloc * nloc + 1, 0);
  for (const auto& x : gprod) ++gcount[x.first + 1];
  for (int k = 0; k < nloc * nloc; ++k) gcount[k + 1] += gcount[k];
  gsorted.resize(gprod.size());
  gfill.assign(gcount.begin(), gcount.end() - 1);
  for (const auto& x : gprod) gsorted[gfill[x.first]++] = x.second;
  // long blocks are split into chunks of <= kPartChunk products (separate records, summed
  // in order by k_assemble_pp) so that no k_lm_visit thread serialises a whole block
  constexpr int kPartChunk = 24;  // measured: 6 / 12 / 24 / unsplit on 2048 S50 windows
  for (int key = 0; key < nloc * nloc; ++key) {
    const int k0 = gcount[key], k1 = gcount[key + 1];
    for (int c0 = k0; c0 < k1; c0 += kPartChunk) {
      const int c1 = std::min(k1, c0 + kPartChunk);
      partKeys.push_back({glocal[key / nloc], glocal[key % nloc]});
      B.part_cbegin.push_back((int)B.part_contrib.size());
      B.part_contrib.insert(B.part_contrib.end(), gsorted.begin() + c0, gsorted.begin() + c1);
    }
  }
  B.lmg_begin.push_back(lb + gl0);
  B.lmg_xbegin.push_back(gx0);
  B.seg_gbegin.push_back((int)B.seg_pose.size());
  B.part_gbegin.push_back((int)B.part_cbegin.size());
}

// landmark groups of k_lm_visit (consecutive whole landmarks of this window, <= opt.lmg_visits
// (<= kLmGroupVisits) visits and <= opt.lmg_lms (<= kLmGroupMax) landmarks; one workgroup, one thread
// per visit) and their visit segments: the visits of a group that belong to one free pose,
// pre-summed by k_lm_visit into one H | g and one U z record (ascending pose; members in visit order)
void WindowPlan::groups() {
  if ((int)segsAtPose.size() < npx) segsAtPose.resize(npx);
  for (int i = 0; i < npx; ++i) segsAtPose[i].clear();
  partKeys.clear();
  partBase = (int)B.part_cbegin.size();
  fbLocal.resize(std::max<size_t>(1, B.fb_off.size()), -1);  // (stale entries are never read: closeGroup
                                                             // sets every f-block it looks up)
  // landmark-pair products a group stages in LDS (kLmPartStage) bound the group as well; only
  // visits of free poses form products. A landmark with more products than the stage holds
  // (>= 64 free observing poses, e.g. a long track in a full graph) gets a group of its own
  // whose products k_lm_visit streams from HBM instead.
  auto pairCount = [&](int l) {
    if (!laNew[l]) return 0;
    int nf = lmXBegin[l + 1] - lmXBegin[l];
    for (int v = lmVisitBegin[l]; v < lmVisitBegin[l + 1]; ++v) nf += posef[B.visit_pose[v] - pb] >= 0;
    return nf * (nf + 1) / 2;
  };
  int gpc = 0;
  B.visit_slot.resize(B.visit_pose.size(), -1);
  int g0 = 0, gl = 0;
  for (int l = 0; l < p->n_landmarks; ++l) {
    const int nv = lmVisitBegin[l + 1] - lmVisitBegin[l] + lmXBegin[l + 1] - lmXBegin[l];
    if (nv > kLmGroupVisits)
      throw ArgError{"landmark with more than " + std::to_string(kLmGroupVisits) + " observing poses"};
    const int gv = lmVisitBegin[l] - lmVisitBegin[g0] + lmXBegin[l] - lmXBegin[g0];
    const int pcl = pairCount(l);
    if (l > g0 && (gv + nv > B.opt.lmg_visits || gl == B.opt.lmg_lms || gpc + pcl > kLmPartStage)) {
      closeGroup(g0, l);
      g0 = l;
      gl = 0;
      gpc = 0;
    }
    ++gl;
    gpc += pcl;
  }
  if (p->n_landmarks > 0) closeGroup(g0, p->n_landmarks);
}

// imu_*, host_*, win_host_range, pp_*, sbp_*, rp_*, win_*_range
void WindowPlan::factorArrays() {
  const int sBase = (int)B.imu_ts.size();
  for (int f = 0; f < p->n_imu; ++f) {
    const int* b = &p->imu_blocks[4 * f];
    const int32_t gb[4] = {pb + b[0], sbb + b[1], pb + b[2], sbb + b[3]};
    appendN(B.imu_blocks, gb, 4);
    B.imu_win.push_back(w);
    B.imu_flags.push_back(ifix[f] ? 2 : 0);
    B.imu_t0.push_back(p->imu_t0_ns[f]);
    B.imu_t1.push_back(p->imu_t1_ns[f]);
    B.imu_sbegin.push_back(sBase + p->imu_sample_begin[f] - p->imu_sample_begin[0]);
  }
  if (p->n_imu) {
    const int s0 = p->imu_sample_begin[0], s1 = p->imu_sample_begin[p->n_imu];
    appendN(B.imu_ts, &p->imu_sample_t_ns[s0], (size_t)(s1 - s0));
    appendN(B.imu_ga, &p->imu_sample_gyr_acc[6 * (size_t)s0], (size_t)6 * (s1 - s0));
  }
  {
    const okvisgpu_imu_params& ip = p->imu_params;
    const double par[7] = {ip.a_max, ip.g_max, ip.sigma_g_c, ip.sigma_a_c, ip.sigma_gw_c, ip.sigma_aw_c, ip.g};
    appendN(B.imu_par, par, 7);
  }
  for (int f = 0; f < p->n_imu; ++f) {
    if (p->imu_state) appendN(B.imu_state, &p->imu_state[(size_t)f * OKVISGPU_IMU_STATE_DOUBLES], OKVISGPU_IMU_STATE_DOUBLES);
    else B.imu_state.insert(B.imu_state.end(), OKVISGPU_IMU_STATE_DOUBLES, 0.0);
  }
  // host-evaluated factors (global pose-kind / speed-bias indices per slot)
  for (int h = 0; h < p->n_host; ++h) {
    const std::array<int, 4>& s = hslot[h];
    const int32_t gb[4] = {s[0] < 0 ? -1 : pb + s[0], s[1] < 0 ? -1 : sbb + s[1], s[2] < 0 ? -1 : pb + s[2],
                           s[3] < 0 ? -1 : sbb + s[3]};
    appendN(B.host_blocks, gb, 4);
    B.host_win.push_back(w);
    B.host_flags.push_back(hfix[h] ? 2 : 0);
  }
  for (const PPrior& q : pps) {
    B.pp_block.push_back(pb + q.blk);
    B.pp_win.push_back(w);
    appendN(B.pp_meas, q.meas, 7);
    appendN(B.pp_L, q.L, 36);
  }
  for (int i = 0; i < p->n_sb_priors; ++i) {
    B.sbp_block.push_back(sbb + p->sb_prior_block[i]);
    B.sbp_win.push_back(w);
    appendN(B.sbp_meas, &p->sb_prior_meas[9 * i], 9);
    appendN(B.sbp_L, &p->sb_prior_sqrt_info[81 * i], 81);
  }
  for (int i = 0; i < p->n_relpose; ++i) {
    B.rp_blocks.push_back(pb + p->relpose_blocks[2 * i]);
    B.rp_blocks.push_back(pb + p->relpose_blocks[2 * i + 1]);
    B.rp_win.push_back(w);
    B.rp_flags.push_back(rfix[i] ? 2 : 0);
    B.rp_kind.push_back(p->relpose_kind ? p->relpose_kind[i] : 0);
    appendN(B.rp_dx, &p->relpose_delta_x[6 * i], 6);
    appendN(B.rp_J, &p->relpose_sqrt_info[36 * i], 36);
    appendN(B.rp_lp, &p->relpose_lin_point[7 * i], 7);
  }
  auto range = [](std::vector<int32_t>& v, int begin, int n) {
    v.push_back(begin);
    v.push_back(begin + n);
  };
  range(B.win_host_range, hgBase, p->n_host);
  range(B.win_pose_range, pb, npx); range(B.win_sb_range, sbb, p->n_speed_biases); range(B.win_lm_range, lb, p->n_landmarks);
  range(B.win_obs_range, ob, p->n_observations); range(B.win_imu_range, ib, p->n_imu);
  range(B.win_pp_range, ppb, (int)pps.size()); range(B.win_sbp_range, sbpb, p->n_sb_priors);
  range(B.win_rp_range, rpb, p->n_relpose);
}

// One factor's contributions: record `index` of `type` on the f-blocks fbs[0..n) (-1: unused slot or
// constant block), whose Jacobian column blocks start at cols[]. The diagonal entries go to the
// f-block lists (gradient / diagonal), the (u, v) products with row offset >= column offset to the
// pair lists.
void WindowPlan::emitFactor(int type, int index, const int* fbs, const int* cols, int n) {
  for (int u = 0; u < n; ++u) {
    if (fbs[u] < 0) continue;
    fbc[fbs[u] - fbBase].push_back(Contrib{type, index, cols[u], cols[u]});
    for (int v = 0; v < n; ++v) {
      if (fbs[v] < 0 || B.fb_off[fbs[u]] < B.fb_off[fbs[v]]) continue;
      pairs[std::make_pair(fbs[u], fbs[v])].push_back(Contrib{type, index, cols[u], cols[v]});
    }
  }
}

// f-block gradient / diagonal contribution lists (fb_cbegin, fb_contrib) and the block pairs'
// lists (emitted by emitPairs()); pe_*. Within a list the order is the insertion order here:
// visits, partial blocks, IMU, host, pose priors, pose-extrinsics blocks, speed/bias priors,
// relative-pose edges (the kernels stream the runs of a pair list by kind).
void WindowPlan::contributions() {
  const int nFb = (int)B.fb_win.size() - fbBase;
  if ((int)fbc.size() < nFb) fbc.resize(nFb);
  for (int k = 0; k < nFb; ++k) fbc[k].clear();
  pairs.clear();
  for (int i = 0; i < npx; ++i) {
    if (poseFb[i] < 0) continue;
    auto& lst = pairs[std::make_pair(poseFb[i], poseFb[i])];
    for (int sg : segsAtPose[i]) {
      fbc[poseFb[i] - fbBase].push_back(Contrib{C_VISIT, sg, 0, 0});
      lst.push_back(Contrib{C_VISIT, sg, 0, 0});
    }
  }
  for (size_t k = 0; k < partKeys.size(); ++k)  // partial Schur blocks, group order
    pairs[partKeys[k]].push_back(Contrib{C_PAIR, partBase + (int)k, 0, 0});
  const int imuCol[4] = {0, 6, 15, 21}, zero[1] = {0}, rpCol[2] = {0, 6};
  for (int f = 0; f < p->n_imu; ++f) {
    if (ifix[f]) continue;
    const int* b = &p->imu_blocks[4 * f];
    const int fbs[4] = {poseFb[b[0]], sbFb[b[1]], poseFb[b[2]], sbFb[b[3]]};
    emitFactor(C_IMU, ib + f, fbs, imuCol, 4);
  }
  for (int h = 0; h < p->n_host; ++h) {  // host factors' slot f-blocks
    if (hfix[h]) continue;
    const std::array<int, 4>& s = hslot[h];
    int fbs[4];
    for (int q = 0; q < 4; ++q) fbs[q] = s[q] < 0 ? -1 : (q & 1) ? sbFb[s[q]] : poseFb[s[q]];
    emitFactor(C_IMU, hgBase + h, fbs, imuCol, 4);
  }
  for (size_t i = 0; i < pps.size(); ++i) emitFactor(C_PPRIOR, ppb + (int)i, &poseFb[pps[i].blk], zero, 1);
  // pose-extrinsics cross blocks: sum over the observations of a free state pose through a
  // variable camera of J_e^T J_p (k_pose_extr); row = the extrinsics block (after all states)
  for (int ps = 0; ps < np; ++ps) {
    if (poseFb[ps] < 0) continue;
    for (int c = 0; c < ncam; ++c) {
      if (poseFb[np + c] < 0) continue;
      xobs.clear();
      for (int k = 0; k < p->n_observations; ++k) {
        const int o = order[k];
        if (p->obs_pose[o] == ps && p->obs_camera[o] == c && !ofix[o]) xobs.push_back(ob + k);
      }
      if (xobs.empty()) continue;
      pairs[std::make_pair(poseFb[np + c], poseFb[ps])].push_back(Contrib{C_PEXT, (int)B.pe_pose.size(), 0, 0});
      B.pe_pose.push_back(pb + ps);
      B.pe_ext.push_back(pb + np + c);
      B.pe_obs_begin.push_back((int32_t)B.pe_obs.size());
      B.pe_obs.insert(B.pe_obs.end(), xobs.begin(), xobs.end());
    }
  }
  for (int i = 0; i < p->n_sb_priors; ++i) emitFactor(C_SBPRIOR, sbpb + i, &sbFb[p->sb_prior_block[i]], zero, 1);
  for (int i = 0; i < p->n_relpose; ++i) {
    if (rfix[i]) continue;
    const int fbs[2] = {poseFb[p->relpose_blocks[2 * i]], poseFb[p->relpose_blocks[2 * i + 1]]};
    emitFactor(C_RELPOSE, rpb + i, fbs, rpCol, 2);
  }
  for (int k = 0; k < nFb; ++k) {
    B.fb_cbegin.push_back((int)B.fb_contrib.size());
    B.fb_contrib.insert(B.fb_contrib.end(), fbc[k].begin(), fbc[k].end());
  }
  // diagonal pairs must exist for every f-block (they carry the damping, diag and rhs)
  for (int k = fbBase; k < (int)B.fb_win.size(); ++k) pairs[std::make_pair(k, k)];
}

// tile-level structure of S and its symbolic LLT (fill within the envelope); tileNz, tileFu,
// tileT, win_bsplit, win_defoff
void WindowPlan::tilePattern() {
  const int T = fpad / kTile;
  std::vector<uint8_t> nz((size_t)T * T, 0);
  for (int i = 0; i < T; ++i) nz[(size_t)i * T + i] = 1;
  for (auto& kv : pairs) {
    const int fa = kv.first.first, fb2 = kv.first.second;
    const int na = B.fb_kind[fa] == 0 ? 6 : 9, nb = B.fb_kind[fb2] == 0 ? 6 : 9;
    for (int ti = B.fb_off[fa] / kTile; ti <= (B.fb_off[fa] + na - 1) / kTile; ++ti)
      for (int tj = B.fb_off[fb2] / kTile; tj <= (B.fb_off[fb2] + nb - 1) / kTile; ++tj)
        nz[(size_t)std::max(ti, tj) * T + std::min(ti, tj)] = 1;
  }
  symbolicFill(nz, T);
  // first band update of every tile (a step k < j with L_ik and L_jk non-zero): until then the
  // factorisation reads the tile from the assembled S, afterwards from its working copy W
  B.tile_fu.resize(B.tile_fu.size() + (size_t)T * T, kNoUpdate);  // (same offsets as the batch's tile_nz)
  int16_t* fu = B.tile_fu.data() + B.tile_fu.size() - (size_t)T * T;
  for (int i = 0; i < T; ++i)
    for (int j = 0; j <= i; ++j)
      for (int k = 0; k < j; ++k)
        if (nz[(size_t)i * T + k] && nz[(size_t)j * T + k]) {
          fu[(size_t)i * T + j] = (int16_t)k;
          break;
        }
  // backward substitution split (nested dissection): the tiles of the left part [0, tL) and of
  // the right part [tL, tS) share no non-zero tile, so once the separator's tiles [tS, T) are
  // solved the two parts are independent (k_chol_bsub: one workgroup each)
  int tL = rightAt / kTile, tS = sepAt / kTile;
  bool split = ndLeft > 0 && tL > 0 && tS > tL;
  for (int i = tL; split && i < tS; ++i)
    for (int j = 0; j < tL; ++j)
      if (nz[(size_t)i * T + j]) split = false;
  B.win_bsplit.push_back(split ? tL : 0); B.win_bsplit.push_back(split ? tS : 0);
  B.win_defoff.push_back(B.defer_total);
  if (split) B.defer_total += (int64_t)(T - tS) * (tS - tL) * kTile;
  B.any_split = B.any_split || split;
  B.tileNz.push_back(std::move(nz));
  B.tileT.push_back(T);
}

// pair_win, pair_fi, pair_fj, pair_cbegin, pair_runs, pair_contrib: the pairs in (fi, fj) order
void WindowPlan::emitPairs() {
  for (auto& kv : pairs) {
    B.pair_win.push_back(w);
    B.pair_fi.push_back(kv.first.first);
    B.pair_fj.push_back(kv.first.second);
    B.pair_cbegin.push_back((int)B.pair_contrib.size());
    // contributions are grouped by kind (visits, landmark pairs, then factor blocks); the
    // kernels stream each run separately
    const int base = (int)B.pair_contrib.size();
    int npair = 0, nv = 0;
    for (const Contrib& c : kv.second) { nv += c.type == C_VISIT; npair += c.type == C_PAIR; }
    for (size_t i = 0; i < kv.second.size(); ++i) {
      const int t = kv.second[i].type;
      const bool ok = (int)i < nv ? t == C_VISIT : ((int)i < nv + npair ? t == C_PAIR : (t != C_VISIT && t != C_PAIR));
      if (!ok) throw std::logic_error("pair contribution runs out of order");
    }
    B.pair_runs.push_back(base + nv);
    B.pair_runs.push_back(base + nv + npair);
    B.pair_contrib.insert(B.pair_contrib.end(), kv.second.begin(), kv.second.end());
  }
}

// tile-parallel schedule (cholSchedule): launch 0 factors every window's root tiles; launch
// l >= 1 runs the band updates of the steps scheduled there, each item (w, i, j, mode | k << 8):
// mode bit 0 = update of tile (i, j) by step k (panels formed from X_k), bit 1 = factor tile
// i (= j) afterwards (the item is its last update)
void cholLaunchItems(HostBatch& B) {
  std::vector<std::vector<int32_t>> byLaunch(1);
  std::vector<int> L, last;
  for (int w = 0; w < B.n_win; ++w) {
    const int T = B.tileT[w];
    const auto& nz = B.tileNz[w];
    const int nl = cholSchedule(nz, T, L, last);
    B.n_chol_launches = std::max(B.n_chol_launches, nl);
    if ((int)byLaunch.size() < nl) byLaunch.resize(nl);
    bool first = true;
    for (int d = 0; d < T; ++d)
      if (last[(size_t)d * T + d] < 0) {
        B.chol_root_items.push_back(w); B.chol_root_items.push_back(d); B.chol_root_items.push_back(first ? 1 : 0);
        first = false;
      }
    for (int k = 0; k < T; ++k)
      for (int i = k + 1; i < T; ++i)
        if (nz[(size_t)i * T + k]) {
          ++B.n_panels;
          for (int j = k + 1; j <= i; ++j)
            if (nz[(size_t)j * T + k]) {
              const bool fac = i == j && last[(size_t)i * T + i] == L[k];
              auto& v = byLaunch[L[k]];
              v.push_back(w); v.push_back(i); v.push_back(j); v.push_back((fac ? 3 : 1) | (k << 8));
              ++B.n_band_updates;
              if (i == j) ++B.n_band_updates_diag;
            }
        }
  }
  for (size_t l = 0; l < byLaunch.size(); ++l) {
    B.chol_upd_begin.push_back((int)B.chol_upd_items.size() / 4);
    B.chol_upd_items.insert(B.chol_upd_items.end(), byLaunch[l].begin(), byLaunch[l].end());
  }
  B.chol_upd_begin.push_back((int)B.chol_upd_items.size() / 4);
}

// assembly work lists: pose-pose pairs (one wavefront each, 4 per workgroup) are grouped so
// that workgroups b, b+8, ... (one XCD under round-robin placement; speed only) walk the pairs of
// the same windows and share their visit blocks in that XCD's L2
// Off-diagonal pairs with few contributions (no visits; partial blocks and factor blocks only)
// take a 16-lane quarter of a wavefront each (k_assemble_pp_light, 16 per workgroup).
void assemblyLists(HostBatch& B) {
  constexpr int kXcd = 8;
  const int nq = B.n_win >= kXcd ? kXcd : 1;
  std::vector<std::vector<int32_t>> q(nq), ql(nq);
  for (int k = 0; k < (int)B.pair_win.size(); ++k) {
    const bool pp = B.fb_kind[B.pair_fi[k]] == 0 && B.fb_kind[B.pair_fj[k]] == 0;
    const int kend = k + 1 < (int)B.pair_cbegin.size() ? B.pair_cbegin[k + 1] : (int)B.pair_contrib.size();
    const bool light = manyWindows(B.n_win) && B.pair_fi[k] != B.pair_fj[k] &&
                       B.pair_runs[2 * k] == B.pair_cbegin[k] && kend - B.pair_cbegin[k] <= kAsmLightMax;
    if (!pp) B.asm_sb_items.push_back(k);
    else if (light) ql[B.pair_win[k] % nq].push_back(k);
    else q[B.pair_win[k] % nq].push_back(k);
  }
  auto interleave = [&](std::vector<std::vector<int32_t>>& qq, int perWG, std::vector<int32_t>& out) {
    std::vector<size_t> pos(nq, 0);
    bool more = true;
    while (more) {
      more = false;
      for (int x = 0; x < nq; ++x)
        for (int i = 0; i < perWG; ++i) {
          const bool has = pos[x] < qq[x].size();
          out.push_back(has ? qq[x][pos[x]++] : -1);
        }
      for (int x = 0; x < nq; ++x) more = more || pos[x] < qq[x].size();
    }
    while (!out.empty() && out.back() < 0) out.pop_back();
  };
  interleave(q, 4, B.asm_pp_items);
  interleave(ql, 16, B.asm_ppl_items);
}

// the batch's flat tile arrays, the closing sentinels of the CSR arrays, lmg_info, obs_Ls
void closeBatch(HostBatch& B) {
  for (int w = 0; w < B.n_win; ++w) {
    B.win_tnzoff.push_back((int64_t)B.tile_nz.size());
    B.tile_nz.insert(B.tile_nz.end(), B.tileNz[w].begin(), B.tileNz[w].end());
    const int T = B.tileT[w];
    for (int k = 0; k < T; ++k) {
      int np = 0;
      for (int i = k + 1; i < T; ++i) np += B.tileNz[w][(size_t)i * T + k] ? 1 : 0;
      B.max_panels = std::max(B.max_panels, np);
    }
    for (int i = 0; i < T; ++i)
      for (int j = 0; j <= i; ++j)
        if (B.tileNz[w][(size_t)i * T + j]) { B.tile_items.push_back(w); B.tile_items.push_back(i); B.tile_items.push_back(j); }
  }
  B.lm_visit_begin.push_back((int)B.visit_pose.size());
  B.lmg_begin.push_back((int)B.lm_win.size());  // groups: begin of each, then the end
  {  // each window's groups are contiguous (built window by window)
    B.win_lmg_range.assign(2 * (size_t)B.n_win, 0);
    const int ng = (int)B.lmg_begin.size() - 1;
    std::vector<int> first(B.n_win, -1), last(B.n_win, -1);
    for (int g = 0; g < ng; ++g) {
      const int w = B.lm_win[B.lmg_begin[g]];
      if (first[w] < 0) first[w] = g;
      last[w] = g;
    }
    for (int w = 0; w < B.n_win; ++w)
      if (first[w] >= 0) {
        B.win_lmg_range[2 * w] = first[w];
        B.win_lmg_range[2 * w + 1] = last[w] + 1;
      }
  }
  B.lmg_xbegin.push_back((int)B.xvisit_pose.size()); B.xvisit_obs_begin.push_back((int)B.xvisit_obs.size());
  B.pe_obs_begin.push_back((int)B.pe_obs.size()); B.part_cbegin.push_back((int)B.part_contrib.size());
  B.visit_obs_begin.push_back((int)B.obs_win.size()); B.imu_sbegin.push_back((int)B.imu_ts.size());
  // host-evaluated factors share the IMU factors' per-factor arrays, after all of them
  B.imu_blocks.insert(B.imu_blocks.end(), B.host_blocks.begin(), B.host_blocks.end());
  B.imu_win.insert(B.imu_win.end(), B.host_win.begin(), B.host_win.end());
  B.imu_flags.insert(B.imu_flags.end(), B.host_flags.begin(), B.host_flags.end());
  B.fb_cbegin.push_back((int)B.fb_contrib.size());
  B.pair_cbegin.push_back((int)B.pair_contrib.size());
  {  // per-group record (two 16-byte loads; the terminal entry closes the last group)
    const int ng = (int)B.lmg_begin.size() - 1;
    B.lmg_info.assign(kLmgInfo * (size_t)(ng + 1), 0);
    for (int g = 0; g <= ng; ++g) {
      const int l0 = B.lmg_begin[g];
      int32_t* r = &B.lmg_info[kLmgInfo * (size_t)g];
      r[0] = l0;
      r[1] = B.lm_visit_begin[l0];
      r[2] = g < ng ? B.lm_win[l0] : -1;
      r[3] = B.seg_gbegin[g];
      r[4] = B.part_gbegin[g];
      r[5] = B.part_cbegin[B.part_gbegin[g]];
    }
  }
  // every reprojection's square-root information diag(s, s) (okvis' keypoint-size information;
  // +0.0 off the diagonal): k_eval_obs then reads s alone (8 instead of 32 bytes per observation)
  // and forms the same products with the constant zeros, so the same bits
  const int nObs = (int)B.obs_win.size();
  B.obs_iso = nObs > 0;
  B.obs_Ls.assign(std::max(1, nObs), 0.0);
  for (int o = 0; o < nObs && B.obs_iso; ++o) {
    const double* L = B.obs_L.data() + 4 * (size_t)o;
    B.obs_iso = L[1] == 0.0 && !std::signbit(L[1]) && L[2] == 0.0 && !std::signbit(L[2]) && L[0] == L[3] &&
                std::signbit(L[0]) == std::signbit(L[3]);
    B.obs_Ls[o] = L[0];
  }
}

}  // namespace

std::vector<AsmRec> assemblyRecords(const HostBatch& B) {
  std::vector<AsmRec> out;
  out.reserve(B.asm_pp_items.size() + B.asm_ppl_items.size() + B.asm_sb_items.size());
  for (const auto* list : {&B.asm_pp_items, &B.asm_ppl_items, &B.asm_sb_items})
    for (const int32_t k : *list) {
      AsmRec r{};
      r.win = -1;  // pad item: every other field 0 (clamped loads of a pad stay inside the arrays)
      if (k >= 0) {
        const int w = B.pair_win[k], fi = B.pair_fi[k], fj = B.pair_fj[k];
        r.win = w;
        r.cb = B.pair_cbegin[k]; r.pb = B.pair_runs[2 * (size_t)k]; r.ob = B.pair_runs[2 * (size_t)k + 1];
        r.ce = B.pair_cbegin[(size_t)k + 1];
        r.fi = B.win_foff[w] + B.fb_off[fi]; r.fj = B.win_foff[w] + B.fb_off[fj];
        r.ld = B.win_fpad[w];
        r.dst = B.win_soff[w] + (int64_t)B.fb_off[fi] * B.win_fpad[w] + B.fb_off[fj];
        r.flags = (fi == fj ? 1 : 0) | (B.fb_kind[fi] != 0 ? 2 : 0) | (B.fb_kind[fj] != 0 ? 4 : 0);
      }
      out.push_back(r);
    }
  return out;
}

void analyse(const std::vector<const okvisgpu_problem*>& probs,
             const std::map<std::tuple<int, int, int>, int>& constOverride, HostBatch& B) {
  B.seg_gbegin.push_back(0);
  B.part_gbegin.push_back(0);
  B.n_win = (int)probs.size();
  B.probs = probs;
  {  // capacity for the per-observation / per-landmark arrays of the whole batch (no regrowth)
    size_t no = 0, nl = 0;
    for (const okvisgpu_problem* p : probs) {
      no += (size_t)std::max(0, p->n_observations);
      nl += (size_t)std::max(0, p->n_landmarks);
    }
    for (auto* v : {&B.obs_pose, &B.obs_lm, &B.obs_cam, &B.obs_win, &B.obs_orig, &B.visit_pose, &B.visit_lm,
                    &B.visit_obs_begin})
      v->reserve(no + 1);
    B.obs_flags.reserve(no); B.obs_kp.reserve(2 * no); B.obs_L.reserve(4 * no);
    B.lm.reserve(4 * nl); B.lm_perm.reserve(nl); B.lm_visit_begin.reserve(nl + 1); B.lm_win.reserve(nl);
    B.lm_free.reserve(nl);
  }
  B.n_imu_total = 0;  // host factors are numbered after every IMU factor of the batch
  for (const okvisgpu_problem* p : probs) B.n_imu_total += std::max(0, p->n_imu);
  WindowPlan W{B, constOverride};
  for (int w = 0; w < B.n_win; ++w) {
    W.begin(w, probs[w]);     ATIME(0)
    W.params();               ATIME(1)
    W.flags();                ATIME(2)
    W.chooseSlotOrder();
    W.stateOrder();           ATIME(3)
    W.sortObservations();     ATIME(4)
    W.visits();               ATIME(5)
    W.extrinsicVisits();      ATIME(6)
    W.groups();               ATIME(7)
    W.factorArrays();         ATIME(8)
    W.contributions();        ATIME(9)
    W.tilePattern();          ATIME(10)
    W.emitPairs();            ATIME(11)
  }
  cholLaunchItems(B);
  assemblyLists(B);
  closeBatch(B);
  B.asm_rec = assemblyRecords(B);  // (after closeBatch: the closing entry of pair_cbegin)
  ATIME(12)
}

// ---- arena layout -------------------------------------------------------------------------------
namespace {

struct LayoutBuilder {
  ArenaLayout L;
  template <class T>
  void bind(T*& field, int region, size_t bytes, const void* src, const char* name) {
    // 256-byte alignment, 8 bytes at least (no two arrays share an address)
    const size_t off = (L.region_bytes[region] + 255) & ~size_t(255);
    L.region_bytes[region] = off + std::max<size_t>(bytes, 8);
    L.table.push_back(ArenaBinding{&field, [](void* f, char* p) { *static_cast<T**>(f) = reinterpret_cast<T*>(p); },
                                   region, off, bytes, src, name});
  }
  template <class T, class V>
  void upload(T*& field, const std::vector<V>& v, const char* name) {
    static_assert(std::is_same<typename std::remove_const<T>::type, V>::value, "field and source element types differ");
    bind(field, 0, v.size() * sizeof(V), v.data(), name);
  }
};
// UP(x): D.x is uploaded from B.x; UPAS(x, v): D.x from B.v; SCR(x, bytes): D.x is zeroed scratch
#define UP(x) A.upload(D.x, B.x, #x)
#define UPAS(x, v) A.upload(D.x, B.v, #x)
#define SCR(x, bytes) A.bind(D.x, 1, bytes, nullptr, #x)

}  // namespace

ArenaLayout layoutArena(const HostBatch& B, int cu_count, DevProblem& D) {
  D = DevProblem{};
  D.n_win = B.n_win; D.cu_count = cu_count;
  D.n_pose = (int)B.pose_win.size(); D.n_sb = (int)B.sb_win.size(); D.n_lm = (int)B.lm_win.size();
  D.n_obs = (int)B.obs_win.size(); D.n_visit = (int)B.visit_pose.size(); D.n_cam = (int)(B.cam.size() / kCamDoubles);
  D.n_imu = B.n_imu_total; D.n_host = (int)B.hf.size(); D.n_fac = D.n_imu + D.n_host;
  D.n_pprior = (int)B.pp_win.size(); D.n_sbprior = (int)B.sbp_win.size(); D.n_relpose = (int)B.rp_win.size();
  D.n_fblock = (int)B.fb_win.size(); D.n_pair = (int)B.pair_win.size();
  D.max_fpad = B.max_fpad; D.max_tiles = B.max_fpad / kTile;
  D.obs_stride = ((int64_t)D.n_obs + 63) / 64 * 64; D.obs_iso = B.obs_iso;
  D.n_lmg = B.lmg_begin.empty() ? 0 : (int)B.lmg_begin.size() - 1;
  D.n_seg = (int)B.seg_pose.size(); D.n_part = (int)B.part_cbegin.size() - 1;
  D.n_xvisit = (int)B.xvisit_pose.size(); D.n_pe = (int)B.pe_pose.size();
  D.n_chol_roots = (int)B.chol_root_items.size() / 3; D.n_chol_launches = B.n_chol_launches;
  D.h_upd_begin = B.chol_upd_begin.data();
  D.n_asm_pp = (int)B.asm_pp_items.size(); D.n_asm_sb = (int)B.asm_sb_items.size();
  D.n_asm_ppl = (int)B.asm_ppl_items.size(); D.n_tiles = (int)(B.tile_items.size() / 3);
  // The table: reservation order is the layout (each region packs its arrays in this order).
  LayoutBuilder A;
  const size_t d8 = sizeof(double);
  const size_t nObs = D.n_obs, nLm = D.n_lm, nSeg = D.n_seg, nFac = D.n_fac, nHost = D.n_host, nPp = D.n_pprior,
               nSbp = D.n_sbprior, nRp = D.n_relpose;
  UPAS(pose[0], pose); UPAS(pose[1], pose); UPAS(sb[0], sb); UPAS(sb[1], sb); UPAS(lm[0], lm); UPAS(lm[1], lm);  // current / candidate
  UP(extr); UP(cam); UP(pose_win); UP(sb_win); UP(lm_win); UP(pose_f); UP(sb_f); UP(lm_free); UP(pose_active); UP(sb_active);
  UP(obs_pose); UP(obs_lm); UP(obs_cam); UP(obs_win); UP(obs_flags); UP(obs_kp); UP(obs_L); UP(obs_Ls);
  SCR(obs_lin[0], d8 * kObsLin * D.obs_stride); SCR(obs_lin[1], d8 * kObsLin * D.obs_stride);
  SCR(obs_cost[0], d8 * nObs); SCR(obs_cost[1], d8 * nObs);
  SCR(grp_red, d8 * kGrpRed * std::max<size_t>(1, B.lmg_begin.size()));
  UP(lm_visit_begin); UP(visit_pose); UP(visit_obs_begin); UP(visit_lm); UP(lmg_begin); UP(lmg_info);
  SCR(lm_V, d8 * 6 * nLm); SCR(lm_g, d8 * 3 * nLm); SCR(lm_Linv, d8 * 9 * nLm); SCR(lm_zz, d8 * 3 * nLm);
  UP(seg_gbegin); UP(seg_pose); UP(seg_range); UP(visit_slot);
  UP(part_gbegin); UP(part_cbegin); UP(part_contrib); SCR(part_S, d8 * 36 * std::max(1, D.n_part));
  SCR(seg_hg, d8 * kSegHG * nSeg); SCR(seg_uz, d8 * kSegUz * nSeg);
  UP(cam_pose); UP(xvisit_pose); UP(xvisit_lm); UP(xvisit_obs_begin); UP(xvisit_obs); UP(xvisit_slot); UP(lmg_xbegin);
  UP(pe_pose); UP(pe_ext); UP(pe_obs_begin); UP(pe_obs); SCR(pe_H, d8 * 36 * std::max(1, D.n_pe));
  UP(imu_blocks); UP(imu_win); UP(imu_flags); UP(imu_t0); UP(imu_t1); UP(imu_sbegin); UP(imu_ts); UP(imu_ga);
  UP(imu_par); UP(imu_state);
  SCR(imu_lin[0], d8 * kImuLin * nFac); SCR(imu_lin[1], d8 * kImuLin * nFac);
  SCR(imu_cost[0], d8 * nFac); SCR(imu_cost[1], d8 * nFac); SCR(imu_jv, d8 * 3 * nFac); SCR(imu_H, d8 * kImuHess * nFac);
  UP(win_host_range); SCR(host_in, d8 * kHostIn * nHost); SCR(host_out, d8 * kHostOut * nHost);
  UP(pp_block); UP(pp_win); UP(pp_meas); UP(pp_L);
  SCR(pp_lin[0], d8 * 42 * nPp); SCR(pp_lin[1], d8 * 42 * nPp);
  SCR(pp_cost[0], d8 * nPp); SCR(pp_cost[1], d8 * nPp); SCR(pp_jv, d8 * 3 * nPp);
  UP(sbp_block); UP(sbp_win); UP(sbp_meas); UP(sbp_L);
  SCR(sbp_lin[0], d8 * 90 * nSbp); SCR(sbp_lin[1], d8 * 90 * nSbp);
  SCR(sbp_cost[0], d8 * nSbp); SCR(sbp_cost[1], d8 * nSbp); SCR(sbp_jv, d8 * 3 * nSbp);
  UP(rp_blocks); UP(rp_win); UP(rp_flags); UP(rp_kind); UP(rp_dx); UP(rp_J); UP(rp_lp);
  SCR(rp_lin[0], d8 * kRelPoseLin * nRp); SCR(rp_lin[1], d8 * kRelPoseLin * nRp);
  SCR(rp_cost[0], d8 * nRp); SCR(rp_cost[1], d8 * nRp); SCR(rp_jv, d8 * 3 * nRp); UP(win_rp_range);
  UP(win_foff); UP(win_fdim); UP(win_fpad); UP(win_soff); UP(win_linvoff); UP(win_fwdoff);
  UP(win_pose_range); UP(win_sb_range); UP(win_lm_range); UP(win_lmg_range); UP(win_obs_range); UP(win_imu_range);
  UP(win_pp_range); UP(win_sbp_range);
  UP(fb_win); UP(fb_kind); UP(fb_index); UP(fb_off); UP(fb_cbegin); UP(fb_contrib);
  UP(pair_win); UP(pair_fi); UP(pair_fj); UP(pair_cbegin); UP(pair_contrib); UP(pair_runs);
  UP(tile_nz); UP(win_tnzoff); UP(tile_fu); UP(asm_pp_items); UP(asm_sb_items); UP(asm_ppl_items); UP(tile_items);
  UP(chol_root_items); UP(chol_upd_items); UP(chol_upd_begin); UP(win_sgap); UP(win_bsplit); UP(win_defoff);
  SCR(S, d8 * std::max<int64_t>(1, B.s_total)); SCR(W, d8 * std::max<int64_t>(1, B.s_total));
  SCR(Linv, d8 * std::max<int64_t>(1, B.linv_total)); SCR(fwdF, d8 * std::max<int64_t>(1, B.fwd_total));
  SCR(chol_defer, d8 * std::max<int64_t>(1, B.defer_total));
  // the f-vectors (reduced ordering, window-concatenated), then the landmark vectors (gL is lm_g)
  const size_t fBytes = d8 * std::max(1, B.f_total), lBytes = d8 * std::max<size_t>(1, 3 * nLm);
  SCR(sF, fBytes); SCR(diagF, fBytes); SCR(hdF, fBytes); SCR(gF, fBytes); SCR(rhsF, fBytes); SCR(yF, fBytes);
  SCR(gnF, fBytes); SCR(dgF, fBytes); SCR(vF, fBytes); SCR(stepF, fBytes);
  SCR(sL, lBytes); SCR(diagL, lBytes); SCR(stepL, lBytes); SCR(yL, lBytes); SCR(gnL, lBytes); SCR(dgL, lBytes); SCR(vL, lBytes);
  SCR(st, sizeof(WinState) * (size_t)D.n_win);
  SCR(self, sizeof(DevProblem));
#undef UP
#undef UPAS
#undef SCR
  return std::move(A.L);
}

}  // namespace okg

// ---- okvisgpu_plan_digest (okvisgpu.h): the plan's totals and the arena table, uploads hashed -----
extern "C" int okvisgpu_plan_digest(const okvisgpu_problem* problems, int32_t n_windows, int32_t cu_count,
                                    int64_t* totals, int32_t capacity, int32_t* n_entries, char* names, int32_t* region,
                                    int64_t* bytes, uint64_t* hash) {
  using namespace okg;
  if (!problems || n_windows <= 0) return OKVISGPU_ERR_INVALID_ARGUMENT;
  try {
    std::vector<const okvisgpu_problem*> probs;
    for (int i = 0; i < n_windows; ++i) probs.push_back(&problems[i]);
    HostBatch B;
    B.opt = planOptions(n_windows, cu_count);
    analyse(probs, {}, B);
    DevProblem D;
    const ArenaLayout L = layoutArena(B, cu_count, D);
    if (totals) {
      const int64_t t[16] = {B.f_total, B.s_total, B.linv_total, B.fwd_total, B.defer_total, B.max_fpad, B.max_panels,
                             B.n_chol_launches, B.n_panels, B.n_band_updates, B.n_band_updates_diag, B.any_split,
                             B.obs_iso, (int64_t)L.scratchBase(), (int64_t)L.region_bytes[1], 0};
      std::copy(t, t + 16, totals);
    }
    if (n_entries) *n_entries = (int32_t)L.table.size();
    for (int i = 0; i < (int)L.table.size() && i < capacity; ++i) {
      const ArenaBinding& b = L.table[i];
      if (names) std::snprintf(names + 32 * i, 32, "%s", b.name);
      if (region) region[i] = b.region;
      if (bytes) bytes[i] = (int64_t)b.bytes;
      if (!hash) continue;
      // FNV-1a-64 of the uploaded bytes (Contrib: four int32 fields, no padding)
      static_assert(sizeof(Contrib) == 4 * sizeof(int32_t), "hash Contrib field by field if it ever has padding");
      hash[i] = 0;
      if (b.region != 0) continue;
      uint64_t h = 1469598103934665603ull;
      const unsigned char* c = static_cast<const unsigned char*>(b.src);
      for (size_t k = 0; k < b.bytes; ++k) h = (h ^ c[k]) * 1099511628211ull;
      hash[i] = h;
    }
    return OKVISGPU_OK;
  } catch (const UnsupportedError&) {
    return OKVISGPU_ERR_UNSUPPORTED;
  } catch (const std::exception&) {
    return OKVISGPU_ERR_INVALID_ARGUMENT;
  } catch (const ArgError&) {
    return OKVISGPU_ERR_INVALID_ARGUMENT;
  }
}

// ---- okvisgpu_plan_assembly (okvisgpu.h): the assembly records beside the arrays they restate ------
extern "C" int okvisgpu_plan_assembly(const okvisgpu_problem* problems, int32_t n_windows, int32_t cu_count,
                                      int32_t* counts, int32_t capacity, int32_t* records, int64_t* arrays) {
  using namespace okg;
  if (!problems || n_windows <= 0 || !counts) return OKVISGPU_ERR_INVALID_ARGUMENT;
  try {
    std::vector<const okvisgpu_problem*> probs;
    for (int i = 0; i < n_windows; ++i) probs.push_back(&problems[i]);
    HostBatch B;
    B.opt = planOptions(n_windows, cu_count);
    analyse(probs, {}, B);
    counts[0] = (int32_t)B.asm_pp_items.size(); counts[1] = (int32_t)B.asm_ppl_items.size();
    counts[2] = (int32_t)B.asm_sb_items.size(); counts[3] = (int32_t)B.asm_rec.size();
    static_assert(sizeof(AsmRec) == kAsmRecInts * sizeof(int32_t), "records are copied out as int32");
    int n = 0;
    for (const auto* list : {&B.asm_pp_items, &B.asm_ppl_items, &B.asm_sb_items})
      for (const int32_t k : *list) {
        if (n >= capacity) return OKVISGPU_OK;
        if (records && n < (int)B.asm_rec.size()) std::memcpy(records + kAsmRecInts * (size_t)n, &B.asm_rec[n], sizeof(AsmRec));
        if (arrays) {  // what a kernel reached from the item through the separate arrays
          int64_t* a = arrays + 16 * (size_t)n;
          std::fill(a, a + 16, 0);
          a[0] = k;
          if (k >= 0) {
            const int w = B.pair_win[k], fi = B.pair_fi[k], fj = B.pair_fj[k];
            const int64_t v[16] = {k, w, B.pair_cbegin[k], B.pair_runs[2 * (size_t)k], B.pair_runs[2 * (size_t)k + 1],
                                   B.pair_cbegin[(size_t)k + 1], fi, fj, B.fb_off[fi], B.fb_off[fj], B.fb_kind[fi],
                                   B.fb_kind[fj], B.win_foff[w], B.win_fpad[w], B.win_soff[w], 0};
            std::copy(v, v + 16, a);
          }
        }
        ++n;
      }
    return OKVISGPU_OK;
  } catch (const UnsupportedError&) {
    return OKVISGPU_ERR_UNSUPPORTED;
  } catch (const std::exception&) {
    return OKVISGPU_ERR_INVALID_ARGUMENT;
  } catch (const ArgError&) {
    return OKVISGPU_ERR_INVALID_ARGUMENT;
  }
}

// ---- okvisgpu_plan_window (okvisgpu.h): one window's reduced system as analyse() plans it ---------
extern "C" int okvisgpu_plan_window(const okvisgpu_problem* p, int32_t nested_dissection, int64_t* info,
                                    uint8_t* tile_nz, int32_t* step_launch, int32_t* natural) {
  using namespace okg;
  if (!p) return OKVISGPU_ERR_INVALID_ARGUMENT;
  try {
    HostBatch B;
    B.opt.nd = nested_dissection != 0;
#ifdef OKG_ANALYSE_TIMING
    for (double& x : g_atime) x = 0.0;
    g_alast = std::chrono::steady_clock::now();
#endif
    analyse({p}, {}, B);
#ifdef OKG_ANALYSE_TIMING
    std::fprintf(stderr, "analyse ms:");
    for (int i = 0; i < kAnalysePhases; ++i) std::fprintf(stderr, " [%d] %.3f", i, g_atime[i]);
    std::fprintf(stderr, "\n");
#endif
    const int T = B.tileT[0], fpad = B.win_fpad[0];
    const auto& nz = B.tileNz[0];
    std::vector<int> L, last;
    const int nl = cholSchedule(nz, T, L, last);
    if (info) {
      int64_t nnz = 0;
      for (uint8_t v : nz) nnz += v;
      const int64_t v[8] = {B.win_fnat[0], fpad, T, nnz, nl, B.win_bsplit[0], B.win_bsplit[1], B.win_sgap[1]};
      std::copy(v, v + 8, info);
    }
    if (tile_nz) std::copy(nz.begin(), nz.end(), tile_nz);
    if (step_launch)
      for (int k = 0; k < T; ++k) {
        bool any = false;
        for (int i = k + 1; i < T && !any; ++i) any = nz[(size_t)i * T + k] != 0;
        step_launch[k] = any ? L[k] : 0;
      }
    if (natural)
      for (int r = 0; r < fpad; ++r) natural[r] = r < B.win_fdim[0] ? B.f_nat[r] : -1;
    return OKVISGPU_OK;
  } catch (const UnsupportedError&) {
    return OKVISGPU_ERR_UNSUPPORTED;
  } catch (const ArgError&) {  // (a bad problem: as okvisgpu_plan_digest reports it)
    return OKVISGPU_ERR_INVALID_ARGUMENT;
  } catch (const std::exception&) {
    return OKVISGPU_ERR_INVALID_ARGUMENT;
  }
}

// ---- okvisgpu_launch_regime (okvisgpu.h): launchRegime() on plain ints ---------------------------
extern "C" int okvisgpu_launch_regime(int32_t n_windows, int32_t cu_count, int32_t any_split, int32_t persistent_fits,
                                      int32_t pipe_fits, int32_t cholesky_schedule, int32_t serial_graph,
                                      int32_t lin_prep, int32_t graph_iters, int32_t* regime) {
  if (n_windows <= 0 || cu_count <= 0 || !regime) return OKVISGPU_ERR_INVALID_ARGUMENT;
  const okg::LaunchRegime r = okg::launchRegime(n_windows, cu_count, any_split != 0, persistent_fits != 0, pipe_fits != 0,
                                                cholesky_schedule, serial_graph, lin_prep, graph_iters);
  const int32_t v[7] = {r.few, r.many, r.serial_graph, r.lin_prep, r.fused_gradnorm, r.graph_iters, r.chol_schedule};
  std::copy(v, v + 7, regime);
  return OKVISGPU_OK;
}
