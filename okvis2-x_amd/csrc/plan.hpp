// plan.hpp — the window planner and the arena layout: everything the host decides about a batch
// before a byte reaches the device. analyse() turns the caller's problems into the HostBatch (state
// order, observation sort, visits, landmark groups, contribution lists, tile pattern, launch and
// assembly lists); layoutArena() names every device array once and places it. Pure host code: no
// HIP runtime call, so it can be read, compiled and checked on a CPU (okvisgpu_plan_digest).
#pragma once

#include <chrono>
#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/okvisgpu.h"
#include "device_problem.hpp"

namespace okg {

struct ArgError { std::string msg; };          // -> OKVISGPU_ERR_INVALID_ARGUMENT
struct UnsupportedError { std::string msg; };  // -> OKVISGPU_ERR_UNSUPPORTED

// The batch-size predicates, on a device of cu CUs. Few: at most a quarter window per CU, the latency
// regime (per-window reductions at 1,024 threads, fused launches of the iteration's independent small
// kernels, small landmark groups). Many: the fewer-workgroup layouts (light pairs, several S tiles
// per workgroup, the GN prep as a window loop); below it latency rules. Below one window per CU:
// nested-dissection order, one-stream graph.
inline bool fewWindows(int n, int cu) { return 4 * n <= cu; }
inline bool manyWindows(int n) { return n >= 64; }
inline bool belowOneWindowPerCu(int n, int cu) { return n < cu; }

// What a batch's size decides about the plan (planOptions): a function of the window count and the
// CU count only, so a window's bits depend on the batch just through them.
struct PlanOptions {
  bool nd = false;  // order the windows' states for the tile-parallel schedule (nested dissection)
  int lmg_visits = kLmGroupVisits, lmg_lms = kLmGroupMax;  // landmark-group bounds (k_lm_visit workgroups)
};
PlanOptions planOptions(int n_windows, int cu_count);

// What a batch's size decides about the launches (launchRegime): the one place the launch structure
// of a solve is chosen; the runtime stores it and the launchers read it (DevProblem's host-only
// fields). None of it changes a solve's bits.
struct LaunchRegime {
  bool few = false, many = false;
  bool serial_graph = true;     // the captured iteration on one stream (else fork streams)
  bool lin_prep = false;        // the GN prep runs inside the linearisation launch (k_lin_few<.., true>)
  bool fused_gradnorm = false;  // the gradient test runs inside the next assembly launch (k_assemble_few)
  int graph_iters = 4;          // iterations captured as one graph beside the single-iteration graph
  int chol_schedule = 1;        // 1 persistent, 2 tile-parallel, 3 split persistent, 4 pipelined, 5 split pipelined
};
// Pure integer logic (okvisgpu_launch_regime, tests/test_launch_regime.py). persistent_fits /
// pipe_fits: the kernels' LDS holds the largest window (cholesky_persistent_lds / _pipe_lds);
// schedule: options.cholesky_schedule (1..5, else automatic); the overrides are the parsed
// measurement switches OKVISGPU_SERIAL_GRAPH (0 / 1), OKVISGPU_LIN_PREP (0) and
// OKVISGPU_GRAPH_ITERS (K), -1 = not set.
LaunchRegime launchRegime(int n_windows, int cu_count, bool any_split, bool persistent_fits, bool pipe_fits,
                          int schedule, int serial_override, int prep_override, int iters_override);

// Host mirror of everything uploaded (built by analyse()).
struct HostBatch {
  int n_win = 0;
  std::vector<const okvisgpu_problem*> probs;
  // bases per window
  std::vector<int> pose_base, sb_base, lm_base, obs_base, imu_base, rp_base;
  // parameters (initial copies)
  std::vector<double> pose, sb, lm, extr, cam;
  std::vector<int32_t> lm_perm;  // internal landmark k of window w is the caller's landmark lm_perm[lm_base[w] + k]
  // extrinsics: camera c of window w is pose-kind block cam_pose[cam_base[w] + c] (after the states)
  std::vector<int32_t> cam_pose;
  std::vector<uint8_t> win_ext_free;  // window has a variable extrinsics block (write-back)
  // extrinsic visits (landmark, variable camera): observation lists (global obs index), the group's
  // range, segment slots; pose-extrinsics cross blocks (state pose, variable camera) with their obs
  std::vector<int32_t> xvisit_pose, xvisit_lm, xvisit_obs_begin, xvisit_obs, xvisit_slot, lmg_xbegin;
  std::vector<int32_t> pe_pose, pe_ext, pe_obs_begin, pe_obs;
  std::vector<int32_t> pose_win, sb_win, lm_win, pose_f, sb_f;
  std::vector<uint8_t> lm_free, pose_active, sb_active;
  // obs (sorted) + permutation to the caller's order (within the window)
  std::vector<int32_t> obs_pose, obs_lm, obs_cam, obs_win, obs_orig;
  std::vector<uint8_t> obs_flags;
  std::vector<double> obs_kp, obs_L;
  std::vector<double> obs_Ls;  // isotropic batches: L = diag(s, s) per observation, s only (obs_iso)
  bool obs_iso = false;
  // visits
  std::vector<int32_t> lm_visit_begin, visit_pose, visit_obs_begin, visit_lm, lmg_begin;
  std::vector<int32_t> lmg_info;  // [n_lmg+1][kLmgInfo]: first landmark, first visit, window, first segment,
                                  // first partial block, first landmark-pair product
  // visit segments: per landmark group, the visits of one free pose (k_lm_visit pre-sums them)
  std::vector<int32_t> seg_gbegin, seg_pose, seg_range, visit_slot;
  // partial Schur blocks: per landmark group and pose pair, sum of Z_a Z_b^T over the group's landmarks
  std::vector<int32_t> part_gbegin, part_cbegin, part_contrib;
  // imu
  std::vector<int32_t> imu_blocks, imu_win, imu_sbegin;
  std::vector<uint8_t> imu_flags;
  std::vector<int64_t> imu_t0, imu_t1, imu_ts;
  std::vector<double> imu_ga, imu_par, imu_state;
  // host-evaluated factors (ABI 5): global factor index n_imu_total + h, after every IMU factor;
  // slot[k] = IMU-layout slot (0 pose0, 1 sb0, 2 pose1, 3 sb1) of the functor's k-th block
  struct HostFactor { int win, local, np, dim; int8_t slot[4]; okvisgpu_loss loss; };
  int n_imu_total = 0;
  std::vector<HostFactor> hf;
  std::vector<int32_t> host_blocks, host_win, win_host_range;
  std::vector<uint8_t> host_flags;
  // priors
  std::vector<int32_t> pp_block, pp_win, sbp_block, sbp_win;
  std::vector<double> pp_meas, pp_L, sbp_meas, sbp_L;
  // relative-pose edges
  std::vector<int32_t> rp_blocks, rp_win;
  std::vector<uint8_t> rp_flags, rp_kind;
  std::vector<double> rp_dx, rp_J, rp_lp;
  // reduced structure
  std::vector<int32_t> win_foff, win_fdim, win_fpad;
  std::vector<int64_t> win_soff, win_linvoff, win_fwdoff;
  std::vector<int32_t> win_lmg_range;
  std::vector<int32_t> win_pose_range, win_sb_range, win_lm_range, win_obs_range, win_imu_range, win_pp_range,
      win_sbp_range, win_rp_range;
  std::vector<int32_t> fb_win, fb_kind, fb_index, fb_off, fb_cbegin;
  // S offset of every f-block: fb_off, plus the window's gap rows after the left part of a
  // nested-dissection order (win_sgap: f offset of the gap, gap length; 0 0 without one); natural
  // index of every f entry (-1: gap row) and natural dimension per window
  std::vector<int32_t> win_sgap, f_nat, win_fnat, win_bsplit;
  std::vector<int64_t> win_defoff;
  int64_t defer_total = 0;
  bool any_split = false;
  PlanOptions opt;  // set by the caller before analyse()
  std::vector<int32_t> chol_root_items;  // (w, d, first-root-of-window flag): tiles no update writes
  int n_chol_launches = 1;
  std::vector<Contrib> fb_contrib;
  std::vector<int32_t> pair_win, pair_fi, pair_fj, pair_cbegin, pair_runs;
  std::vector<int32_t> asm_pp_items, asm_sb_items, asm_ppl_items;
  // the three lists item by item as AsmRec records (heavy, light, speed/bias; assemblyRecords).
  // Not an arena-table entry: the runtime uploads it into a buffer of its own.
  std::vector<AsmRec> asm_rec;
  std::vector<int32_t> chol_upd_items, chol_upd_begin, tile_items;
  int64_t n_panels = 0;  // structurally non-zero tiles below the diagonal (panel products)
  int64_t n_band_updates = 0;
  int64_t n_band_updates_diag = 0;  // of which symmetric updates of a diagonal tile (SYRK)
  std::vector<Contrib> pair_contrib;
  int64_t s_total = 0, linv_total = 0, fwd_total = 0;
  std::vector<std::vector<uint8_t>> tileNz;  // per window T x T (tileT), concatenated in tile_nz at win_tnzoff
  std::vector<uint8_t> tile_nz;
  std::vector<int16_t> tile_fu;
  std::vector<int64_t> win_tnzoff;
  std::vector<int> tileT;
  int f_total = 0;
  int max_fpad = 0;
  int max_panels = 0;  // most non-zero tiles below a diagonal tile (panels of one Cholesky step)
};

inline int pad64(int x) { return (x + kTile - 1) / kTile * kTile; }
void symbolicFill(std::vector<uint8_t>& nz, int T);
int cholSchedule(const std::vector<uint8_t>& nz, int T, std::vector<int>& L, std::vector<int>& last);

// Build the batch (B.nd / lmg_* set by the caller, planOptions). `constOverride` carries
// okvisgpu_set_block_constant() edits. Throws ArgError / UnsupportedError on a bad problem.
void analyse(const std::vector<const okvisgpu_problem*>& probs,
             const std::map<std::tuple<int, int, int>, int>& constOverride, HostBatch& B);

// The record of every assembly work item (B.asm_pp_items, then B.asm_ppl_items, then
// B.asm_sb_items), from the batch's pair, block and window arrays. Pure: reads B, returns the records
// (analyse() keeps them in B.asm_rec).
std::vector<AsmRec> assemblyRecords(const HostBatch& B);

// Development: host-time split of analyse() by phase (build with -DOKG_ANALYSE_TIMING; printed by
// okvisgpu_plan_window): validate, params, flags, state order, observation sort, visits, extrinsic
// visits, groups, factor arrays, contributions, tile pattern, pair emission, batch tail.
#ifdef OKG_ANALYSE_TIMING
constexpr int kAnalysePhases = 13;
extern double g_atime[kAnalysePhases];
extern std::chrono::steady_clock::time_point g_alast;
#endif

// ---- arena layout: one binding per device array. The uploaded arrays are laid out first (one
// contiguous host -> device copy from a pinned staging buffer), the scratch arrays after them (one memset).
struct ArenaBinding {
  void* field;                        // the DevProblem pointer member
  void (*set)(void* field, char* p);  // stores p with the member's own pointer type
  int region;                         // 0 uploaded, 1 scratch
  size_t off, bytes;                  // offset within the region
  const void* src;                    // uploaded: the host bytes (in the HostBatch)
  const char* name;
};
struct ArenaLayout {
  std::vector<ArenaBinding> table;   // reservation order
  size_t region_bytes[2] = {0, 0};   // extent of the uploaded arrays, of the scratch arrays
  size_t scratchBase() const { return (region_bytes[0] + 255) & ~size_t(255); }  // the uploaded region comes first
  size_t arenaBytes() const { return scratchBase() + region_bytes[1]; }
  // points every bound field into an arena at base
  void patch(char* base) const {
    for (const ArenaBinding& b : table) b.set(b.field, base + (b.region ? scratchBase() : 0) + b.off);
  }
};
// Fills D's counts and scalars from the batch and returns the layout whose bindings point into D.
// A function of (B, cu_count) only; B must outlive D's use (h_upd_begin points into it).
ArenaLayout layoutArena(const HostBatch& B, int cu_count, DevProblem& D);

}  // namespace okg
