// resident_calls.cpp — the entry points of the okvisgpu C ABI that read the resident batch (the one
// okvisgpu_set_problems uploaded) and hand numbers back; none is on the solve's path (runtime.cpp).
// Every call opens with onResident() and brings its results down through the context's stream
// into its pinned stage: one window's arrays with download() (host loops: window_export.hpp), the
// arrays of the two batch-wide calls declared in a BatchLayout (batch_stage.hpp).
#include "runtime.hpp"

#include <algorithm>
#include <cstring>

#include "launch.hpp"
#include "okvisgpu_math.hpp"
#include "window_export.hpp"

using namespace okg;

namespace {

// What every call here opens with, in this order: a context with a problem, `busy` (the call's own
// refusal between solve_begin and solve_end; null: the call is allowed there), the window if the
// call takes one; then the body on the context's device, its exceptions mapped by guarded().
template <class F>
int onResident(okvisgpu_ctx* c, const int32_t* window, const char* busy, F&& body) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (busy && c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, busy);
  if (window && (*window < 0 || *window >= c->P.n_win)) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    return body();
  });
}

// Arrays of doubles brought down through the context's stream into its pinned stage, which is
// taken once for both (paramStage synchronises and may reallocate): a at the returned address, b
// behind it. Nothing is copied for an empty array. The bytes hold until the stage is taken again.
const double* download(okvisgpu_ctx* c, const double* a, size_t na, const double* b = nullptr, size_t nb = 0) {
  double* h = reinterpret_cast<double*>(c->paramStage(8 * (na + nb)));
  if (na) HIPCHK(hipMemcpyAsync(h, a, 8 * na, hipMemcpyDeviceToHost, c->stream));
  if (nb) HIPCHK(hipMemcpyAsync(h + na, b, 8 * nb, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return h;
}

// ---- per-kernel timing with algorithmic work models (bench.py's roofline) ------------------
enum KernelId {
  K_ASSEMBLE_PP, K_ASSEMBLE_SB, K_CHOLESKY, K_LM_VISIT, K_LM_VISIT_PREP, K_EVAL_IMU, K_EVAL_OBS, K_JV,
  K_FGRAD, K_LM_BACKSUB, K_COUNT
};
const char* kKernelNames[K_COUNT] = {"k_assemble_pp", "k_assemble_sb", "k_cholesky", "k_lm_visit", "k_lm_visit_prep",
                                     "k_eval_imu",    "k_eval_obs",    "k_jv",       "k_fgrad",
                                     "k_lm_backsub_jv"};
// bound: 0 = HBM bytes, 1 = FP64 matrix-core FLOPs
const int kKernelBound[K_COUNT] = {0, 0, 1, 0, 0, 0, 0, 0, 0, 0};

// Algorithmic work of one iteration's launches of kernel k over the whole batch: compulsory HBM
// bytes (every operand read once, every result written once) or FP64 FLOPs.
double kernelWork(const HostBatch& B, const DevProblem& P, int k) {
  const double d8 = 8.0;
  const double nObs = P.n_obs, nVis = P.n_visit, nLm = P.n_lm, nImu = P.n_imu;
  switch (k) {
    case K_ASSEMBLE_PP: {
      double desc = 0, pairs = 0;
      for (const auto* list : {&B.asm_pp_items, &B.asm_ppl_items})
        for (int it : *list)
          if (it >= 0) { desc += B.pair_cbegin[it + 1] - B.pair_cbegin[it]; pairs += 1; }
      return desc * 16 + (double)P.n_part * 36 * d8 + (double)P.n_seg * (21 + 6) * d8 + pairs * (36 + 12) * d8;
    }
    case K_ASSEMBLE_SB: {
      double desc = 0, entries = 0;
      for (int it : B.asm_sb_items) {
        desc += B.pair_cbegin[it + 1] - B.pair_cbegin[it];
        const int ni = B.fb_kind[B.pair_fi[it]] == 0 ? 6 : 9, nj = B.fb_kind[B.pair_fj[it]] == 0 ? 6 : 9;
        entries += ni * nj;
      }
      return desc * 16 + nImu * kImuLin * d8 + entries * d8;
    }
    case K_CHOLESKY: {
      // algorithmic FLOPs of the tile-sparse LLT and its two triangular solves, per structurally
      // non-zero 64x64 tile (n = 64; VERDICT r05 "Next" 1, SURVEY §8d "LLT d^3/3"):
      //   diagonal potrf n^3/3, panel TRSM n^3, diagonal band update (SYRK) n^2(n+1), off-diagonal
      //   band update (GEMM) 2n^3, forward + backward substitution 2n^2 per diagonal tile and 4n^2
      //   per panel tile. The kernel's own extras (X = L_kk^-1, full 64-column MFMA blocks) are not
      //   counted; the issued-MFMA figure sits beside this in bench.py (frac_issued).
      const double n = 64.0;
      double diag = 0;
      for (int w = 0; w < P.n_win; ++w) diag += B.tileT[w];
      const double panels = (double)B.n_panels, syrk = (double)B.n_band_updates_diag,
                   gemm = (double)(B.n_band_updates - B.n_band_updates_diag);
      return diag * (n * n * n / 3.0 + 2.0 * n * n) + panels * (n * n * n + 4.0 * n * n) +
             syrk * n * n * (n + 1.0) + gemm * 2.0 * n * n * n;
    }
    case K_LM_VISIT:  // obs linearisation + params in; segments, partial blocks, landmark blocks out
      return nObs * (kObsLin * d8 + 1) + nVis * (7 * d8 + 16) + (double)P.n_seg * (27 + 6) * d8 +
             (double)B.part_contrib.size() * 4 + (double)P.n_part * 36 * d8 + nLm * 40 * d8;
    case K_LM_VISIT_PREP:  // W recomputed from the obs linearisation; U z, partial blocks, L^-1 out
      return nObs * (kObsLin * d8 + 1) + nVis * (7 * d8 + 16) + (double)P.n_seg * 6 * d8 +
             (double)B.part_contrib.size() * 4 + (double)P.n_part * 36 * d8 + nLm * 34 * d8;
    case K_EVAL_IMU: return nImu * (2.0 * kImuState + kImuLin + 2 * 16) * d8 + (double)B.imu_ts.size() * 7 * d8;
    case K_EVAL_OBS: return nObs * (16 + (P.obs_iso ? 8 : 32) + 13 + kObsLin * d8 + 8) + nLm * 4 * d8 + (double)B.pose_f.size() * 7 * d8;
    case K_JV:  // factors: IMU linearisation, prior / edge Jacobians in, their J*v forms out
      return nImu * (kImuLin + 3) * d8 + (double)P.n_pprior * (42 + 3) * d8 + (double)P.n_sbprior * (90 + 3) * d8 +
             (double)P.n_relpose * (kRelPoseLin + 3) * d8;
    case K_LM_BACKSUB:  // obs linearisation (A, flags) once; pose / landmark parameters and vectors once per
                        // block; gauss_newton_step_ and gradient_ of the landmarks (6 doubles) and the
                        // groups' J*v forms out
      return nObs * (6 * d8 + 1) + nVis * (3 * d8 + 16) + (double)P.n_pose * (7 + 18) * d8 +
             nLm * (4 + 9 + 3 + 3 + 3 + 3 + 6) * d8 + (double)P.n_lmg * kGrpRed * d8;
    case K_FGRAD: return (double)P.n_seg * 27 * d8 + nImu * kImuLin * d8 + (double)B.fb_contrib.size() * 16;
  }
  return 0.0;
}

}  // namespace

// ViGraph::updateLandmarks on the current parameter values (okvisgpu_update_landmarks): every
// window's current set is gathered into set 0 as downloadParams does (before the first solve
// WinState is the build's zeroed scratch: xcur = 0, set 0 holds the uploaded values), one kernel
// over the batch's landmarks, the landmarks copied from the arena beside its outputs, one copy
// down, and a threaded scatter into the caller's order (landmarks through lm_perm, observations
// through obs_orig). Of the caller's problem arrays only the re-placed landmarks are written.
void okvisgpu_ctx::updateLandmarks(okvisgpu_landmark_update* U) {
  for (int w = 0; w < B.n_win; ++w) {
    U[w].n_initialised = U[w].n_reset = 0;
    U[w].in_front = 1;
    U[w].reserved = 0;
  }
  const size_t nl = (size_t)P.n_lm, no = (size_t)P.n_obs;
  if (nl == 0) return;  // nothing to launch
  bool wantErr = false;
  for (int w = 0; w < B.n_win; ++w) wantErr = wantErr || U[w].obs_error != nullptr;
  double *dQ = nullptr, *dLm = nullptr, *dErr = nullptr, *dDirs = nullptr;
  uint8_t* dFlags = nullptr;
  BatchLayout S;
  const auto sQ = S.out(dQ, nullptr, nl);
  const auto sLm = S.out(dLm, nullptr, 4 * nl);
  const auto sFlags = S.out(dFlags, nullptr, nl);
  BatchSlot<double> sErr{-1};  // the observation errors travel only when a window asks for them
  if (wantErr) sErr = S.out(dErr, nullptr, no);
  else S.scratch(dErr, no);
  S.scratch(dDirs, 3 * no);
  beginBatch(S);
  launch_select_current(P, stream);
  launch_update_landmarks(P, dQ, dFlags, dErr, dDirs, stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(dLm, P.lm[0], 4 * nl * 8, hipMemcpyDeviceToDevice, stream));
  finishBatch(S);
  const double *hQ = S.host(sQ), *hLm = S.host(sLm), *hErr = wantErr ? S.host(sErr) : nullptr;
  const uint8_t* hFlags = S.host(sFlags);
  forWindows(B.n_win, [&](int w) {
    const okvisgpu_problem* p = probs[w];
    okvisgpu_landmark_update& u = U[w];
    const size_t lb = (size_t)B.lm_base[w];
    const int* perm = &B.lm_perm[lb];
    int nInit = 0, nReset = 0, front = 1;
    for (int k = 0; k < p->n_landmarks; ++k) {
      const int l = perm[k];
      const uint8_t f = hFlags[lb + k];
      if (u.quality) u.quality[l] = hQ[lb + k];
      if (u.initialised) u.initialised[l] = (f & kLmInitialised) ? 1 : 0;
      if (u.reset) u.reset[l] = (f & kLmReset) ? 1 : 0;
      nInit += (f & kLmInitialised) ? 1 : 0;
      if (f & kLmNotInFront) front = 0;
      if (f & kLmReset) {
        ++nReset;
        std::memcpy(&p->landmarks[4 * (size_t)l], hLm + 4 * (lb + k), 32);
      }
    }
    u.n_initialised = nInit;
    u.n_reset = nReset;
    u.in_front = front;
    if (u.obs_error) {
      const size_t ob = (size_t)B.obs_base[w];
      for (int k = 0; k < p->n_observations; ++k) u.obs_error[B.obs_orig[ob + k]] = hErr[ob + k];
    }
  });
}

// ViGraph::computeCovisibilities on the structure of the last set_problems
// (okvisgpu_covisibilities): a record per window that has states, landmarks and observations, the
// record of every 64-landmark word (k_covis_bits' work list), the work lists of the two count
// kernels (covisFitsLds picks a window's), the caller's exclusion masks permuted into internal
// landmark order; all of it staged and uploaded as one copy. k_covis_bits writes every word of the
// bitset and the count kernels every element of counts / n_observed, so nothing is cleared. One
// copy back, then a threaded scatter; the pair and visibility totals are taken on the host. Reads
// no parameter value and writes neither the caller's problem arrays nor the arena.
void okvisgpu_ctx::covisibilities(okvisgpu_covisibility* V) {
  const int nwin = B.n_win;
  std::vector<CovisWin> recs;
  std::vector<int> recOf((size_t)nwin, -1);
  std::vector<int32_t> items0, items1, wordRec;  // wordRec: the record of each 64-landmark word
  size_t lds0 = 0;
  int64_t words = 0, bitsTot = 0, cntTot = 0, stateTot = 0;
  bool anyMask = false;
  for (int w = 0; w < nwin; ++w) {
    const okvisgpu_problem* p = probs[w];
    V[w].n_pairs = V[w].n_visible = V[w].any = V[w].path = 0;
    if (p->n_poses <= 0 || p->n_landmarks <= 0 || p->n_observations <= 0) {  // all zeros, nothing to launch
      const size_t S = (size_t)std::max(p->n_poses, 0);
      if (V[w].counts) std::memset(V[w].counts, 0, 4 * S * S);
      if (V[w].n_observed) std::memset(V[w].n_observed, 0, 4 * S);
      if (V[w].visible) std::memset(V[w].visible, 0, S);
      continue;
    }
    CovisWin r{};
    r.lm_begin = B.lm_base[w];
    r.n_lm = p->n_landmarks;
    r.pose_begin = B.pose_base[w];
    r.n_state = p->n_poses;
    r.word_begin = (int32_t)words;
    r.n_words = (p->n_landmarks + 63) / 64;
    r.state_off = (int32_t)stateTot;
    r.bits_off = bitsTot;
    r.counts_off = cntTot;
    const int idx = (int)recs.size();
    if (covisFitsLds(r.n_state, r.n_words)) {
      items0.push_back(idx);
      lds0 = std::max(lds0, covisLdsBytes(r.n_state, r.n_words));
    } else {
      V[w].path = 1;
      const int T = (r.n_state + kCovisTile - 1) / kCovisTile;
      for (int ti = 0; ti < T; ++ti)
        for (int tj = 0; tj <= ti; ++tj) items1.insert(items1.end(), {idx, ti, tj});
    }
    wordRec.insert(wordRec.end(), (size_t)r.n_words, idx);
    words += r.n_words;
    stateTot += r.n_state;
    bitsTot += (int64_t)r.n_state * r.n_words;
    cntTot += (int64_t)r.n_state * r.n_state;
    anyMask = anyMask || V[w].landmark_excluded != nullptr;
    recOf[w] = idx;
    recs.push_back(r);
  }
  if (recs.empty()) return;

  const CovisWin* dRec = nullptr;
  const int32_t *dWordRec = nullptr, *dItems0 = nullptr, *dItems1 = nullptr;
  const uint8_t* dEx = nullptr;  // stays null without a mask
  unsigned long long* dBits = nullptr;
  int32_t *dCnt = nullptr, *dObs = nullptr;
  BatchLayout S;
  S.in(dRec, recs.data(), recs.size());
  S.in(dWordRec, wordRec.data(), wordRec.size());
  S.in(dItems0, items0.data(), items0.size());
  S.in(dItems1, items1.data(), items1.size());
  BatchSlot<uint8_t> sEx{-1};
  if (anyMask) sEx = S.in(dEx, nullptr, (size_t)P.n_lm);
  const auto sCnt = S.out(dCnt, nullptr, (size_t)cntTot);
  const auto sObs = S.out(dObs, nullptr, (size_t)stateTot);
  S.scratch(dBits, (size_t)bitsTot);
  beginBatch(S);
  if (anyMask)
    forWindows(nwin, [&](int w) {
      const okvisgpu_problem* p = probs[w];
      uint8_t* ex = S.host(sEx) + (size_t)B.lm_base[w];
      const uint8_t* in = V[w].landmark_excluded;
      const int* perm = &B.lm_perm[B.lm_base[w]];
      if (!in) std::memset(ex, 0, (size_t)std::max(p->n_landmarks, 0));
      else
        for (int k = 0; k < p->n_landmarks; ++k) ex[k] = in[perm[k]] ? 1 : 0;
    });
  uploadBatch(S);
  launch_covis_bits(P, dRec, (int)recs.size(), dWordRec, (int)words, dEx, dBits, stream);
  launch_covis_counts(dRec, dItems0, (int)items0.size(), lds0, dItems1, (int)(items1.size() / 3), dBits, dCnt, dObs,
                      stream);
  HIPCHK(hipGetLastError());
  finishBatch(S);
  const int32_t *hCnt = S.host(sCnt), *hObs = S.host(sObs);
  forWindows(nwin, [&](int w) {
    if (recOf[w] < 0) return;
    const CovisWin& r = recs[(size_t)recOf[w]];
    okvisgpu_covisibility& v = V[w];
    const size_t ns = (size_t)r.n_state;
    const int32_t *c = hCnt + r.counts_off, *o = hObs + r.state_off;
    if (v.counts) std::memcpy(v.counts, c, 4 * ns * ns);
    if (v.n_observed) std::memcpy(v.n_observed, o, 4 * ns);
    int pairs = 0, vis = 0;
    for (size_t i = 0; i < ns; ++i) {
      vis += o[i] > 0;
      if (v.visible) v.visible[i] = o[i] > 0 ? 1 : 0;
      for (size_t j = i + 1; j < ns; ++j) pairs += c[i * ns + j] > 0;
    }
    v.n_pairs = pairs;
    v.n_visible = vis;
    v.any = pairs > 0 ? 1 : 0;
  });
}

extern "C" {

int okvisgpu_kernel_count(void) { return K_COUNT; }
const char* okvisgpu_kernel_name(int32_t k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }

int okvisgpu_time_kernel(okvisgpu_ctx* c, int32_t kernel, int32_t reps, double* avg_ms, double* work,
                         int32_t* bound) {
  if (!c || kernel < 0 || kernel >= K_COUNT || reps < 1) return OKVISGPU_ERR_INVALID_ARGUMENT;
  return onResident(c, nullptr, "time_kernel: call after solve_end", [&]() {
    const DevProblem& P = c->P;
    hipStream_t s = c->stream;
    // re-arm every window (the linearisation of the finished solve stays resident); the solve
    // state is scratch afterwards and is rebuilt by the next solve_begin
    std::vector<WinState> st = c->readStates();
    for (WinState& w : st) {
      w.done = 0; w.need_gn = 1; w.gn_failed = 0; w.eval_cand = 1; w.accepted = 1; w.step_valid = 2;
      w.z_mu = -1.0;  // stale: the prep mode recomputes Z
    }
    HIPCHK(hipMemcpyAsync(P.st, st.data(), sizeof(WinState) * st.size(), hipMemcpyHostToDevice, s));
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    auto event = [&]() {
      if (used == ev.size()) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        ev.push_back(e);
      }
      HIPCHK(hipEventRecord(ev[used], s));
      return used++;
    };
    std::vector<std::pair<size_t, size_t>> spans;
    auto timed = [&](auto&& launch) {
      const size_t a = event();
      launch();
      const size_t b = event();
      spans.emplace_back(a, b);
    };
    for (int r = 0; r < reps; ++r) {
      switch (kernel) {
        case K_ASSEMBLE_PP: timed([&] { launch_assemble_pp(P, s); }); break;
        case K_ASSEMBLE_SB: timed([&] { launch_assemble_sb(P, s); }); break;
        case K_LM_VISIT: timed([&] { launch_lm_visit(P, 1, s); }); break;
        case K_LM_VISIT_PREP: timed([&] { launch_lm_visit(P, 2, s); }); break;
        case K_EVAL_IMU:
          // redo counter := 0 forces the re-preintegration the candidate evaluations of a solve
          // mostly perform (the device-side IMU state is scratch afterwards)
          if (P.n_imu > 0)
            HIPCHK(hipMemset2DAsync(P.imu_state, sizeof(double) * kImuState, 0, sizeof(double), P.n_imu, s));
          timed([&] { launch_eval_imu_as_solved(P, 1, s); });
          break;
        case K_EVAL_OBS: timed([&] { launch_eval_obs(P, 1, s); }); break;
        case K_JV: timed([&] { launch_jv(P, s); }); break;
        case K_LM_BACKSUB: timed([&] { launch_lm_backsub(P, s); }); break;
        case K_FGRAD: timed([&] { launch_fgrad(P, 1, s); }); break;
        case K_CHOLESKY:  // (the factorisation reads the assembled S and works in W: repeatable)
          c->ensureS(s);
          launch_assemble(P, s);
          timed([&] { launch_cholesky(P, s); });
          break;
      }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    double tot = 0.0;
    for (auto& sp : spans) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, ev[sp.first], ev[sp.second]));
      tot += t;
    }
    for (auto e : ev) (void)hipEventDestroy(e);
    if (avg_ms) *avg_ms = tot / reps;
    if (work) *work = kernelWork(c->B, P, kernel);
    if (bound) *bound = kKernelBound[kernel];
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_get_stats(okvisgpu_ctx* c, okvisgpu_problem_stats* st) {
  if (!c || !st) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  const HostBatch& B = c->B;
  const DevProblem& P = c->P;
  std::memset(st, 0, sizeof(*st));
  st->n_windows = B.n_win;
  st->n_poses = P.n_pose;
  st->n_speed_biases = P.n_sb;
  st->n_landmarks = P.n_lm;
  for (int w = 0; w < B.n_win; ++w) {
    const okvisgpu_problem* p = B.probs[w];
    for (int c = 0; c < p->n_cameras; ++c) st->n_extrinsics_free += B.pose_f[B.pose_base[w] + p->n_poses + c] >= 0;
  }
  for (uint8_t f : B.lm_free) st->n_landmarks_free += f != 0;
  st->n_observations = P.n_obs;
  st->n_visits = P.n_visit;
  st->n_imu = P.n_imu;
  st->n_imu_samples = (int64_t)B.imu_ts.size();
  st->n_pose_priors = P.n_pprior;
  st->n_sb_priors = P.n_sbprior;
  st->n_relpose = P.n_relpose;
  st->cholesky_launches = B.n_chol_launches;
  st->reduced_dim = 0;
  for (int d : B.win_fnat) st->reduced_dim += d;
  st->s_tiles_nonzero = (int64_t)B.tile_items.size() / 3;
  for (int T : B.tileT) st->s_tiles_dense += (int64_t)T * (T + 1) / 2;
  st->n_block_pairs = P.n_pair;
  st->n_visit_segments = P.n_seg;
  st->n_partial_blocks = P.n_part;
  st->arena_bytes = (int64_t)c->arenaBytes;
  st->cholesky_split_windows = 0;
  for (size_t w = 0; w + 1 < c->B.win_bsplit.size(); w += 2) st->cholesky_split_windows += c->B.win_bsplit[w + 1] > 0;
  return OKVISGPU_OK;
}

int okvisgpu_evaluate(okvisgpu_ctx* c, int32_t window, double* cost) {
  return onResident(c, &window, nullptr, [&]() {
    okvisgpu_options o;
    okvisgpu_default_options(&o);
    c->setOptions(o);
    c->resetStates(1e-8);
    c->evalAll(2, c->stream);
    launch_reduce(c->P, R_COST_INIT, c->stream);
    HIPCHK(hipGetLastError());
    auto st = c->readStates();
    if (cost) *cost = st[window].x_cost + st[window].fixed_cost;
    // a failed host_evaluate leaves +inf in the cost; report it like okvisgpu_eval_host does
    // (ceres::Problem::Evaluate returns false)
    const int h0 = c->B.win_host_range[2 * window], h1 = c->B.win_host_range[2 * window + 1];
    for (int h = h0; h < h1; ++h)
      if (c->hostFail[h - c->P.n_imu]) return fail(c, OKVISGPU_ERR_NUMERICAL, "host_evaluate failed");
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_linearize_reduce(okvisgpu_ctx* c, int32_t window, int32_t jacobi_scaling, double mu, double* S,
                              double* rhs, double* cost, int32_t* dim_out) {
  return onResident(c, &window, nullptr, [&]() {
    okvisgpu_options o;
    okvisgpu_default_options(&o);
    o.jacobi_scaling = jacobi_scaling;
    c->setOptions(o);
    c->resetStates(mu);
    c->launchInit(2);
    launch_lm_prep(c->P, c->stream);
    launch_assemble(c->P, c->stream);
    HIPCHK(hipGetLastError());
    auto st = c->readStates();
    // exported in the natural order, whatever order the window's S is held in (window_export.hpp)
    const HostBatch& B = c->B;
    const int fdim = B.win_fdim[window], fpad = B.win_fpad[window], dn = B.win_fnat[window];
    const int32_t* nat = B.f_nat.data() + B.win_foff[window];
    if (dim_out) *dim_out = dn;
    if (cost) *cost = st[window].x_cost + st[window].fixed_cost;
    const size_t nS = S && dn ? (size_t)fpad * fpad : 0, nRhs = rhs && dn ? (size_t)fdim : 0;
    const double* h = download(c, c->P.S + B.win_soff[window], nS, c->P.rhsF + B.win_foff[window], nRhs);
    if (nS) scatterNaturalSym(h, nat, fdim, fpad, dn, S);
    if (nRhs) scatterNatural(h + nS, nat, fdim, rhs);
    if (st[window].gn_failed) return fail(c, OKVISGPU_ERR_NUMERICAL, "landmark block not positive definite");
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_gauss_newton_step(okvisgpu_ctx* c, int32_t window, const okvisgpu_options* options, double mu,
                               double* y_f, double* y_l, int32_t* dim_out) {
  return onResident(c, &window, "gauss_newton_step: call after solve_end", [&]() {
    okvisgpu_options o;
    okvisgpu_default_options(&o);
    if (options) {
      o.jacobi_scaling = options->jacobi_scaling;
      o.cholesky_schedule = options->cholesky_schedule;
      o.min_lm_diagonal = options->min_lm_diagonal;
      o.max_lm_diagonal = options->max_lm_diagonal;
    }
    c->setOptions(o);
    c->resetStates(mu);
    c->ensureS(c->stream);
    c->launchInit(2);
    // the first iteration's Gauss-Newton solve (unfusedSteps), over the whole resident batch
    launch_lm_prep(c->P, c->stream);
    launch_assemble(c->P, c->stream);
    launch_cholesky(c->P, c->stream);
    launch_lm_backsub(c->P, c->stream, /*storeY=*/true);  // (y_l is stored for this entry point only)
    HIPCHK(hipGetLastError());
    auto st = c->readStates();
    const HostBatch& B = c->B;
    const int fdim = B.win_fdim[window], dn = B.win_fnat[window];
    if (dim_out) *dim_out = dn;
    if (st[window].dev_error)
      throw HipError{"window " + std::to_string(window) + ": the pipelined Cholesky's team wait reached its limit",
                     OKVISGPU_ERR_DEVICE};
    if (st[window].gn_failed) return fail(c, OKVISGPU_ERR_NUMERICAL, "Gauss-Newton step: a block is not positive definite");
    const int nl = c->probs[window]->n_landmarks, lb = B.lm_base[window];
    const size_t nF = y_f && dn ? (size_t)fdim : 0, nL = y_l ? 3 * (size_t)nl : 0;
    const double* h = download(c, c->P.yF + B.win_foff[window], nF, c->P.yL + 3 * (size_t)lb, nL);
    // y_f in the natural order, as okvisgpu_linearize_reduce exports rhs; y_l in the caller's landmark order
    if (nF) scatterNatural(h, B.f_nat.data() + B.win_foff[window], fdim, y_f);
    if (nL) {
      const double* v = h + nF;
      const int* perm = &B.lm_perm[lb];
      for (int k = 0; k < nl; ++k)
        for (int a = 0; a < 3; ++a) y_l[3 * (size_t)perm[k] + a] = B.lm_free[lb + k] ? v[3 * (size_t)k + a] : 0.0;
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_eval_reprojection(okvisgpu_ctx* c, int32_t window, double* r, double* Jp, double* Jl) {
  return onResident(c, &window, nullptr, [&]() {
    c->resetStates(1e-8);
    launch_eval(c->P, 3, c->stream);
    HIPCHK(hipGetLastError());
    const int64_t S = c->P.obs_stride;
    const double* lin = download(c, c->P.obs_lin[0], (size_t)kObsLin * S);
    const okvisgpu_problem* pr = c->probs[window];
    const int ob = c->B.obs_base[window], n = pr->n_observations;
    for (int k = 0; k < n; ++k) {
      const int g = ob + k, o = c->B.obs_orig[g];
      if (r) for (int i = 0; i < 2; ++i) r[2 * o + i] = lin[(size_t)i * S + g];
      double A[6], Jpo[12], Jlo[6];
      for (int i = 0; i < 6; ++i) A[i] = lin[(size_t)(2 + i) * S + g];
      const double* hp = &pr->landmarks[4 * pr->obs_landmark[o]];
      const double* tw = &pr->poses[7 * pr->obs_pose[o]];
      const double p3[3] = {hp[0] - tw[0] * hp[3], hp[1] - tw[1] * hp[3], hp[2] - tw[2] * hp[3]};
      obsJacobians(A, p3, hp[3], Jpo, Jlo);
      if (Jp) for (int i = 0; i < 12; ++i) Jp[12 * o + i] = Jpo[i];
      if (Jl) for (int i = 0; i < 6; ++i) Jl[6 * o + i] = Jlo[i];
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_eval_imu(okvisgpu_ctx* c, int32_t window, int32_t redo_always, double* r, double* J) {
  return onResident(c, &window, nullptr, [&]() {
    okvisgpu_options o;
    okvisgpu_default_options(&o);
    o.redo_propagation_always = redo_always;
    c->setOptions(o);
    c->resetStates(1e-8);
    launch_eval(c->P, 3, c->stream);
    HIPCHK(hipGetLastError());
    const size_t n = (size_t)c->probs[window]->n_imu, ib = (size_t)c->B.imu_base[window];
    splitRecords(download(c, c->P.imu_lin[0] + ib * kImuLin, n * kImuLin), n, kImuLin, 15, r, J);
    // keep the caller's ImuError state in sync (the evaluation may have re-integrated); this takes
    // the stage again, so the records were split first
    c->downloadParams();
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_eval_relpose(okvisgpu_ctx* c, int32_t window, double* r, double* J) {
  return onResident(c, &window, nullptr, [&]() {
    c->resetStates(1e-8);
    launch_eval(c->P, 3, c->stream);
    HIPCHK(hipGetLastError());
    const size_t n = (size_t)c->probs[window]->n_relpose, rb = (size_t)c->B.rp_base[window];
    splitRecords(download(c, c->P.rp_lin[0] + rb * kRelPoseLin, n * kRelPoseLin), n, kRelPoseLin, 6, r, J);
    return (int)OKVISGPU_OK;
  });
}

// the host-evaluated factors' records lie in the IMU linearisation array, behind the IMU factors'
int okvisgpu_eval_host(okvisgpu_ctx* c, int32_t window, double* r, double* J) {
  return onResident(c, &window, nullptr, [&]() {
    c->resetStates(1e-8);
    c->evalHost(3, c->stream);
    HIPCHK(hipGetLastError());
    const int h0 = c->B.win_host_range[2 * window], n = c->B.win_host_range[2 * window + 1] - h0;
    splitRecords(download(c, c->P.imu_lin[0] + (size_t)h0 * kImuLin, (size_t)n * kImuLin), (size_t)n, kImuLin, 15, r, J);
    for (int f = 0; f < n; ++f)
      if (c->hostFail[h0 - c->P.n_imu + f]) return fail(c, OKVISGPU_ERR_NUMERICAL, "host_evaluate failed");
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_update_landmarks(okvisgpu_ctx* c, okvisgpu_landmark_update* updates) {
  if (!c || !updates) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "update_landmarks: bad arguments");
  return onResident(c, nullptr, "update_landmarks: call after solve_end", [&]() {
    c->updateLandmarks(updates);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_covisibilities(okvisgpu_ctx* c, okvisgpu_covisibility* out) {
  if (!c || !out) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "covisibilities: bad arguments");
  return onResident(c, nullptr, "covisibilities: call after solve_end", [&]() {
    c->covisibilities(out);
    return (int)OKVISGPU_OK;
  });
}

}  // extern "C"
