// runtime.cpp — host runtime of the okvisgpu C ABI (include/okvisgpu.h).
//
// The drop-in replacement for `::ceres::Solve(options_, problem_.get(), &summary_)` in
// okvis::ViGraph::optimise (okvis_ceres/src/ViGraph.cpp:1844-1890): structure analysis of each
// window and the arena layout (plan.cpp), one HBM arena per context, upload, and the trust-region
// iteration as a captured hipGraph that is replayed max_num_iterations times with every decision
// taken on the device (kernels_control.hip). The host synchronises once per solve (plus once per
// iteration only when a CeresIterationCallback-style time limit is requested). The call-scoped batch
// entry points are in batch_calls.cpp; the context both files work on is declared in runtime.hpp.
#include "runtime.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "launch.hpp"
#include "loss.hpp"
#include "okvisgpu_math.hpp"

using namespace okg;

namespace {

double nowS() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Per-window host copies (parameter staging / write-back) split over host threads: contiguous
// window ranges, one thread per range. Small batches run on the calling thread. The thread count
// follows OMP_NUM_THREADS (the job's CPU share) and is capped at 16.
template <class F>
void forWindows(int n, F&& fn) {
  static const int cap = [] {
    const char* e = std::getenv("OMP_NUM_THREADS");
    int t = e ? std::atoi(e) : (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(t, 16));
  }();
  const int nt = std::min(cap, n / 64);
  if (nt <= 1) {
    for (int w = 0; w < n; ++w) fn(w);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(nt);
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t]() {
      for (int w = (int)((int64_t)n * t / nt); w < (int)((int64_t)n * (t + 1) / nt); ++w) fn(w);
    });
  for (auto& x : th) x.join();
}

// Offsets of okvisgpu_covisibilities' arrays in batchScratch (the batch's arena is laid out by
// layoutArena, plan.hpp; a call-scoped batch by BatchLayout, batch_stage.hpp).
struct Arena {
  size_t size = 0;
  size_t reserve(size_t bytes) {
    const size_t off = (size + 255) & ~size_t(255);
    size = off + std::max<size_t>(bytes, 8);
    return off;
  }
};

}  // namespace

void okvisgpu_ctx::decideRegime(int schedule) {
  // the persistent kernels keep the window's rhs / y in dynamic LDS next to their static tiles
  auto fits = [&](size_t staticLds) { return staticLds + sizeof(double) * (size_t)P.max_fpad <= ldsPerBlock; };
  const char *ser = std::getenv("OKVISGPU_SERIAL_GRAPH"), *prep = std::getenv("OKVISGPU_LIN_PREP"),
             *gi = std::getenv("OKVISGPU_GRAPH_ITERS");
  const LaunchRegime r = launchRegime(P.n_win, cuCount, B.any_split, fits(persistentLds), fits(pipeLds), schedule,
                                      ser && (ser[0] == '0' || ser[0] == '1') ? ser[0] - '0' : -1,
                                      prep && prep[0] == '0' ? 0 : -1, gi && *gi ? std::max(0, std::atoi(gi)) : -1);
  if (r.chol_schedule != regime.chol_schedule) dropGraph();
  regime = r;
  P.few = r.few; P.many = r.many; P.lin_prep = r.lin_prep; P.chol_schedule = r.chol_schedule;
}

// S is cleared by the build's arena memset; its padded diagonal (rows >= fdim) is set once per
// build before the first factorisation (k_zero_S). The factorisation works in W and the assembly
// overwrites its blocks, so S needs no clearing per iteration.
void okvisgpu_ctx::ensureS(hipStream_t s) {
  if (!sNeedsInit) return;
  launch_zero_S(P, s);
  sNeedsInit = false;
}

void okvisgpu_ctx::fillSummaries(const std::vector<WinState>& st, okvisgpu_summary* sums) {
  if (!sums) return;
  const double t1 = nowS();
  for (int w = 0; w < P.n_win; ++w) {
    const WinState& s = st[w];
    okvisgpu_summary& S = sums[w];
    std::memset(&S, 0, sizeof(S));
    S.initial_cost = s.initial_cost;
    S.final_cost = std::min(s.min_cost, s.x_cost) + s.fixed_cost;
    S.num_iterations = s.iteration;
    S.num_successful_steps = s.num_succ + 1;  // Ceres counts iteration 0
    S.num_unsuccessful_steps = s.num_unsucc;
    S.termination_type = s.done ? s.termination : OKVISGPU_NO_CONVERGENCE;
    S.total_time_s = t1 - solveT0;
    S.final_radius = s.radius;
    S.final_mu = s.mu;
    S.preprocessor_time_s = tPre;
    S.minimizer_time_s = tMin;
    S.postprocessor_time_s = tPost;
    S.linear_solver_time_s = S.residual_evaluation_time_s = S.jacobian_evaluation_time_s = S.step_time_s = -1.0;
    if (phasesTimed) {  // phase ids: kPhaseNames
      auto sum = [&](std::initializer_list<int> ids) {
        double t = 0.0;
        for (int i : ids) t += phaseMs[i];
        return t * 1e-3;
      };
      S.linear_solver_time_s = sum({0, 1, 2, 3, 4, 5, 6, 7});
      S.step_time_s = sum({8});
      S.residual_evaluation_time_s = sum({9, 10, 11, 12});
      S.jacobian_evaluation_time_s = sum({13, 14});
    }
  }
}

// end of a solve: iterations done (states were just read back), write-back, summaries
void okvisgpu_ctx::finish(const std::vector<WinState>& st, okvisgpu_summary* sums) {
  const double t = nowS();
  tMin = t - tIterStart;
  for (int w = 0; w < P.n_win; ++w)
    if (st[w].dev_error) {
      inSolve = false;
      throw HipError{"window " + std::to_string(w) + ": the pipelined Cholesky's team wait reached its limit",
                     OKVISGPU_ERR_DEVICE};
    }
  downloadParams();
  inSolve = false;
  tPost = nowS() - t;
  fillSummaries(st, sums);
}

okvisgpu_ctx::~okvisgpu_ctx() {
  dropGraph();
  if (arena) (void)hipFree(arena);
  if (hostStage) (void)hipHostFree(hostStage);
  if (hostIn) (void)hipHostFree(hostIn);
  if (hostOut) (void)hipHostFree(hostOut);
  for (hipEvent_t e : forkEv) (void)hipEventDestroy(e);
  for (hipStream_t q : side)
    if (q) (void)hipStreamDestroy(q);
  if (stream) (void)hipStreamDestroy(stream);
}

void okvisgpu_ctx::dropGraph() {
  if (iterGraph) {
    (void)hipGraphExecDestroy(iterGraph);
    iterGraph = nullptr;
  }
  if (iterGraphK) {
    (void)hipGraphExecDestroy(iterGraphK);
    iterGraphK = nullptr;
  }
  graphIters = 1;
}
// n iterations of the captured graph(s), in stream order
void okvisgpu_ctx::launchIterations(int n) {
  int k = 0;
  if (iterGraphK)
    for (; k + graphIters <= n; k += graphIters) HIPCHK(hipGraphLaunch(iterGraphK, stream));
  for (; k < n; ++k) HIPCHK(hipGraphLaunch(iterGraph, stream));
}

// ---- host-evaluated factors (SURVEY.md §8b fallback) ------------------------------------------
// Every evaluation point (initial, each candidate) runs, in stream order: k_host_gather (the
// blocks' values of the factors the eval mode selects) -> copy to pinned memory -> host node
// (hostEvaluate: the caller's Evaluate on options.num_threads threads, manifold + loss applied
// here) -> copy back -> k_host_scatter into the IMU-layout linearisation records. All of it is
// graph-capturable (the host step is a host node of the captured iteration).
void okvisgpu_ctx::ensureHostBuffers() {
  hostFail.assign((size_t)P.n_host, 0);
  if (P.n_host <= hostBufFactors) return;
  if (hostIn) HIPCHK(hipHostFree(hostIn));
  if (hostOut) HIPCHK(hipHostFree(hostOut));
  hostIn = hostOut = nullptr;
  hostBufFactors = 0;
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hostIn), sizeof(double) * kHostIn * P.n_host, hipHostMallocDefault));
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hostOut), sizeof(double) * kHostOut * P.n_host, hipHostMallocDefault));
  hostBufFactors = P.n_host;
}

// PoseManifold plus Jacobian at x, 7x6 row-major (PoseLocalParameterization.cpp:56-68): the
// minimal Jacobian of a pose-kind block is J_ambient * this, as Ceres applies a block's manifold.
void okvisgpu_ctx::posePlusJacobian(const double* x, double* J) {
  for (int i = 0; i < 42; ++i) J[i] = 0.0;
  J[0 * 6 + 0] = J[1 * 6 + 1] = J[2 * 6 + 2] = 1.0;
  const double qx = x[3], qy = x[4], qz = x[5], qw = x[6];
  const double Q[4][3] = {{qw, qz, -qy}, {-qz, qw, qx}, {qy, -qx, qw}, {-qx, -qy, -qz}};  // oplus(q), cols 0..2
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 3; ++c) J[(3 + r) * 6 + 3 + c] = Q[r][c] * 0.5;
}

// One host factor: Evaluate at the gathered point; r and the minimal Jacobian (IMU column
// layout), corrected for the factor's loss (Ceres' Corrector, both branches) unless mode 3 (raw
// evaluation), into its host_out record. Failure: cost +inf, r = J = 0.
void okvisgpu_ctx::hostEvaluateOne(int h) {
  const double* in = hostIn + (size_t)h * kHostIn;
  double* out = hostOut + (size_t)h * kHostOut;
  if (in[0] == 0.0) return;
  const int mode = (int)in[1];
  const HostBatch::HostFactor& F = B.hf[h];
  const okvisgpu_problem* p = probs[F.win];
  static const int at[4] = {8, 15, 24, 31}, col[4] = {0, 6, 15, 21};
  const double* prm[4] = {nullptr, nullptr, nullptr, nullptr};
  double amb[4][OKVISGPU_HOST_MAX_RESIDUALS * 9];
  double* jac[4] = {nullptr, nullptr, nullptr, nullptr};
  double r[OKVISGPU_HOST_MAX_RESIDUALS];
  for (int k = 0; k < F.np; ++k) {
    prm[k] = in + at[F.slot[k]];
    jac[k] = amb[k];
    std::memset(amb[k], 0, sizeof(amb[k]));
  }
  std::memset(r, 0, sizeof(r));
  std::memset(out, 0, sizeof(double) * kHostOut);
  int ok = 0;
  try {
    ok = p->host_evaluate(p->host_user, F.local, prm, r, jac);
  } catch (...) {
    ok = 0;
  }
  hostFail[h] = ok ? 0 : 1;
  if (!ok) {
    out[0] = HUGE_VAL;
    return;
  }
  double sq = 0.0;
  for (int i = 0; i < F.dim; ++i) sq += r[i] * r[i];
  // minimal Jacobian (IMU column layout): ambient * PoseManifold plus Jacobian for pose-kind
  // blocks, identity for speed/bias
  double* J = out + 1 + 15;
  for (int k = 0; k < F.np; ++k) {
    const int q = F.slot[k];
    if (q & 1) {  // speed/bias: identity manifold
      for (int i = 0; i < F.dim; ++i)
        for (int c = 0; c < 9; ++c) J[i * 30 + col[q] + c] = amb[k][i * 9 + c];
    } else {
      double Jp[42];
      posePlusJacobian(prm[k], Jp);
      for (int i = 0; i < F.dim; ++i)
        for (int c = 0; c < 6; ++c) {
          double s = 0.0;
          for (int a = 0; a < 7; ++a) s += amb[k][i * 7 + a] * Jp[a * 6 + c];
          J[i * 30 + col[q] + c] = s;
        }
    }
  }
  for (int i = 0; i < F.dim; ++i) out[1 + i] = r[i];
  if (F.loss.kind == OKVISGPU_LOSS_NONE || mode == 3) {
    out[0] = 0.5 * sq;
    return;
  }
  // Ceres' Corrector (internal/ceres/corrector.cc; okvis restates it at TwoPoseGraphError.cpp:
  // 292-337), applied to the minimal Jacobian as Ceres' ResidualBlock does after the manifold
  double rho[3];
  lossRho(F.loss, sq, rho);
  out[0] = 0.5 * rho[0];
  const double sqrtRho1 = std::sqrt(rho[1]);
  double rScale = sqrtRho1, alphaSq = 0.0;
  if (sq != 0.0 && rho[2] > 0.0) {  // second-order (Triggs) correction
    const double D = 1.0 + 2.0 * sq * rho[2] / rho[1];
    const double alpha = 1.0 - std::sqrt(D);
    rScale = sqrtRho1 / (1.0 - alpha);
    alphaSq = alpha / sq;
  }
  for (int k = 0; k < F.np; ++k) {
    const int q = F.slot[k], nc = (q & 1) ? 9 : 6;
    for (int c = 0; c < nc; ++c) {
      double* Jc = J + col[q] + c;
      if (alphaSq == 0.0) {
        for (int i = 0; i < F.dim; ++i) Jc[i * 30] *= sqrtRho1;
        continue;
      }
      double rtj = 0.0;
      for (int i = 0; i < F.dim; ++i) rtj += Jc[i * 30] * r[i];
      for (int i = 0; i < F.dim; ++i) Jc[i * 30] = sqrtRho1 * (Jc[i * 30] - alphaSq * r[i] * rtj);
    }
  }
  for (int i = 0; i < F.dim; ++i) out[1 + i] = r[i] * rScale;
}

void okvisgpu_ctx::hostEvaluate() {
  const int n = P.n_host;
  const int nt = std::min(std::max(1, std::min(16, opts.num_threads)), n / 8);
  if (nt <= 1) {
    for (int h = 0; h < n; ++h) hostEvaluateOne(h);
    return;
  }
  hostWorkers.run(nt, [this, n, nt](int t) {
    for (int h = (int)((int64_t)n * t / nt); h < (int)((int64_t)n * (t + 1) / nt); ++h) hostEvaluateOne(h);
  });
}

void okvisgpu_ctx::evalHost(int mode, hipStream_t s) {
  if (P.n_host == 0) return;
  launch_host_gather(P, mode, s);
  HIPCHK(hipMemcpyAsync(hostIn, P.host_in, sizeof(double) * kHostIn * P.n_host, hipMemcpyDeviceToHost, s));
  HIPCHK(hipLaunchHostFunc(s, hostEvaluateCallback, this));
  HIPCHK(hipMemcpyAsync(P.host_out, hostOut, sizeof(double) * kHostOut * P.n_host, hipMemcpyHostToDevice, s));
  launch_host_scatter(P, s);
}
// every residual of the batch at one evaluation point (mode: launch.hpp)
void okvisgpu_ctx::evalAll(int mode, hipStream_t s) {
  launch_eval(P, mode, s);
  evalHost(mode, s);
}
// after the initial evaluation: a window whose host factor failed there ends with FAILURE
// (Ceres: "Residual and Jacobian evaluation failed" at iteration 0)
void okvisgpu_ctx::failInitialHostEvaluations() {
  if (P.n_host == 0) return;
  HIPCHK(hipStreamSynchronize(stream));
  std::vector<uint8_t> bad(P.n_win, 0);
  bool any = false;
  for (int h = 0; h < P.n_host; ++h)
    if (hostFail[h]) any = bad[B.hf[h].win] = 1;
  if (!any) return;
  std::vector<WinState> st = readStates();
  for (int w = 0; w < P.n_win; ++w)
    if (bad[w]) {
      st[w].done = 1;
      st[w].termination = OKVISGPU_FAILURE;
    }
  HIPCHK(hipMemcpyAsync(P.st, st.data(), sizeof(WinState) * st.size(), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
}

// (Re)build the device problem. Nothing of the previous batch survives a failure: the context
// holds no problem until a build completes (entry points then return OKVISGPU_ERR_NO_PROBLEM).
void okvisgpu_ctx::build() {
  haveProblem = false;
  inSolve = false;
  dropGraph();
  const bool timing = std::getenv("OKVISGPU_BUILD_TIMING") != nullptr;  // development: host cost split
  const auto tb0 = std::chrono::steady_clock::now();
  {
    HostBatch nb;
    nb.opt = planOptions((int)probs.size(), cuCount);
#ifdef OKG_ND_OVERRIDE
    if (const char* e = std::getenv("OKVISGPU_ND")) nb.opt.nd = e[0] == '1';  // (development A/B builds only)
#endif
#ifdef OKG_LMG_OVERRIDE  // (development A/B builds only: OKVISGPU_LMG=visits,landmarks)
    if (const char* e = std::getenv("OKVISGPU_LMG")) {
      int v = 0, m = 0;
      if (std::sscanf(e, "%d,%d", &v, &m) == 2 && v >= 1 && v <= kLmGroupVisits && m >= 1 && m <= kLmGroupMax) {
        nb.opt.lmg_visits = v;
        nb.opt.lmg_lms = m;
      }
    }
#endif
    analyse(probs, constOverride, nb);  // may throw: B is untouched until it succeeds
    B = std::move(nb);
  }
  const auto tb1 = std::chrono::steady_clock::now();
  const ArenaLayout L = layoutArena(B, cuCount, P);
  // ---- allocate (reusing the arena while the batch fits) + upload: one contiguous host -> device
  // copy of the uploaded region from the pinned staging buffer, one memset of the scratch region
  const size_t upBytes = L.region_bytes[0], total = L.arenaBytes();
  if (!arena || total > arenaCap) {
    if (arena) {
      HIPCHK(hipFree(arena));
      arena = nullptr;
      arenaCap = 0;
    }
    HIPCHK(hipMalloc(&arena, total));
    arenaCap = total;
  }
  arenaBytes = total;
  char* base = static_cast<char*>(arena);
  char* stage = paramStage(upBytes);  // (synchronises: the previous upload is done)
  const auto tb2 = std::chrono::steady_clock::now();
  for (const ArenaBinding& b : L.table)
    if (b.region == 0 && b.bytes) std::memcpy(stage + b.off, b.src, b.bytes);
  const auto tb3 = std::chrono::steady_clock::now();
  if (timing) {
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    std::fprintf(stderr, "okvisgpu build: analyse %.3f ms, layout+alloc %.3f ms, stage %.3f ms (%zu B)\n", ms(tb0, tb1),
                 ms(tb1, tb2), ms(tb2, tb3), upBytes);
  }
  if (upBytes) HIPCHK(hipMemcpyAsync(base, stage, upBytes, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(base + L.scratchBase(), 0, L.region_bytes[1], stream));
  sNeedsInit = true;
  L.patch(base);
  P.gL = P.lm_g;  // the landmark gradient is the accumulated J_l^T r
  {  // the assembly records: the context's own buffer (not an arena-table entry)
    const size_t need = std::max<size_t>(sizeof(AsmRec), B.asm_rec.size() * sizeof(AsmRec));
    void* rec = asmRecBuf.need(need);
    if (!B.asm_rec.empty())
      HIPCHK(hipMemcpyAsync(rec, B.asm_rec.data(), B.asm_rec.size() * sizeof(AsmRec), hipMemcpyHostToDevice, stream));
    P.asm_rec = static_cast<const AsmRec*>(rec);
  }
  HIPCHK(hipStreamSynchronize(stream));
  decideRegime(0);  // (default options: the entry points that launch without a solve_begin)
  uploadDescriptor();
  ensureHostBuffers();
  haveProblem = true;
  structureDirty = false;
}

// Kernels read the descriptor through one pointer to device memory (a 1.3 KB by-value kernarg is
// re-fetched field by field on every dependent access).
void okvisgpu_ctx::uploadDescriptor() {
  HIPCHK(hipMemcpyAsync(const_cast<DevProblem*>(P.self), &P, sizeof(DevProblem), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
}

void okvisgpu_ctx::setOptions(const okvisgpu_options& o) {
  DevOptions& d = P.opt;
  d.max_num_iterations = o.max_num_iterations;
  d.jacobi_scaling = o.jacobi_scaling;
  d.max_num_consecutive_invalid_steps = o.max_num_consecutive_invalid_steps;
  d.redo_propagation_always = o.redo_propagation_always;
  d.function_tolerance = o.function_tolerance;
  d.gradient_tolerance = o.gradient_tolerance;
  d.parameter_tolerance = o.parameter_tolerance;
  d.initial_radius = o.initial_trust_region_radius;
  d.max_radius = o.max_trust_region_radius;
  d.min_radius = o.min_trust_region_radius;
  d.min_relative_decrease = o.min_relative_decrease;
  d.min_lm_diagonal = o.min_lm_diagonal;
  d.max_lm_diagonal = o.max_lm_diagonal;
  decideRegime(o.cholesky_schedule);  // (drops the captured graph when the Cholesky schedule changes)
  uploadDescriptor();
}

void okvisgpu_ctx::resetStates(double mu) {
  std::vector<WinState> s(P.n_win);
  for (auto& x : s) {
    std::memset(&x, 0, sizeof(x));
    x.radius = P.opt.initial_radius;
    x.mu = mu;
    x.need_gn = 1;
    x.z_mu = -1.0;
    x.termination = OKVISGPU_NO_CONVERGENCE;
  }
  HIPCHK(hipMemcpyAsync(P.st, s.data(), sizeof(WinState) * s.size(), hipMemcpyHostToDevice, stream));
}

// Pinned staging for the parameter copies: the set_problems staging buffer (it holds both
// parameter sets and the IMU states, so it is large enough), grown if ever needed.
char* okvisgpu_ctx::paramStage(size_t bytes) {
  HIPCHK(hipStreamSynchronize(stream));  // no copy out of / into it is still in flight
  if (bytes > hostStageBytes) {
    if (hostStage) HIPCHK(hipHostFree(hostStage));
    hostStage = nullptr;
    hostStageBytes = 0;
    HIPCHK(hipHostMalloc(&hostStage, bytes, hipHostMallocDefault));
    hostStageBytes = bytes;
  }
  return static_cast<char*>(hostStage);
}

// Upload current host parameter values into both parameter sets (+ IMU state): the windows are
// packed into pinned memory in device order (host threads over windows), set 0 and the IMU
// states go up in one copy each, and set 1 is a device-side copy of set 0.
void okvisgpu_ctx::uploadParams() {
  const size_t np = 7 * (size_t)P.n_pose, ns = 9 * (size_t)P.n_sb, nl = 4 * (size_t)P.n_lm,
               ni = (size_t)P.n_imu * kImuState;
  double* pose = reinterpret_cast<double*>(paramStage((np + ns + nl + ni) * 8));
  double *sb = pose + np, *lm = sb + ns, *imu = lm + nl;
  forWindows(B.n_win, [&](int w) {
    const okvisgpu_problem* p = probs[w];
    double* q = pose + 7 * (size_t)B.pose_base[w];
    std::memcpy(q, p->poses, sizeof(double) * 7 * p->n_poses);
    std::memcpy(q + 7 * (size_t)p->n_poses, p->extrinsics, sizeof(double) * 7 * p->n_cameras);
    std::memcpy(sb + 9 * (size_t)B.sb_base[w], p->speed_biases, sizeof(double) * 9 * p->n_speed_biases);
    double* l = lm + 4 * (size_t)B.lm_base[w];
    const int* perm = &B.lm_perm[B.lm_base[w]];
    for (int k = 0; k < p->n_landmarks; ++k) std::memcpy(l + 4 * (size_t)k, &p->landmarks[4 * (size_t)perm[k]], 32);
    double* f = imu + (size_t)B.imu_base[w] * kImuState;
    if (p->imu_state) std::memcpy(f, p->imu_state, sizeof(double) * kImuState * p->n_imu);
    else std::memset(f, 0, sizeof(double) * kImuState * p->n_imu);
  });
  if (np) HIPCHK(hipMemcpyAsync(P.pose[0], pose, np * 8, hipMemcpyHostToDevice, stream));
  if (ns) HIPCHK(hipMemcpyAsync(P.sb[0], sb, ns * 8, hipMemcpyHostToDevice, stream));
  if (nl) HIPCHK(hipMemcpyAsync(P.lm[0], lm, nl * 8, hipMemcpyHostToDevice, stream));
  if (ni) HIPCHK(hipMemcpyAsync(P.imu_state, imu, ni * 8, hipMemcpyHostToDevice, stream));
  if (np) HIPCHK(hipMemcpyAsync(P.pose[1], P.pose[0], np * 8, hipMemcpyDeviceToDevice, stream));
  if (ns) HIPCHK(hipMemcpyAsync(P.sb[1], P.sb[0], ns * 8, hipMemcpyDeviceToDevice, stream));
  if (nl) HIPCHK(hipMemcpyAsync(P.lm[1], P.lm[0], nl * 8, hipMemcpyDeviceToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
}

// Write device results back into the caller's arrays: k_select_current gathers every window's
// current parameter set into set 0 (WinState::xcur on the device), then one copy per array into
// pinned memory and a threaded scatter into the windows' arrays.
void okvisgpu_ctx::downloadParams() {
  const size_t np = 7 * (size_t)P.n_pose, ns = 9 * (size_t)P.n_sb, nl = 4 * (size_t)P.n_lm,
               ni = (size_t)P.n_imu * kImuState;
  double* pose = reinterpret_cast<double*>(paramStage((np + ns + nl + ni) * 8));
  double *sb = pose + np, *lm = sb + ns, *imu = lm + nl;
  launch_select_current(P, stream);
  HIPCHK(hipGetLastError());
  if (np) HIPCHK(hipMemcpyAsync(pose, P.pose[0], np * 8, hipMemcpyDeviceToHost, stream));
  if (ns) HIPCHK(hipMemcpyAsync(sb, P.sb[0], ns * 8, hipMemcpyDeviceToHost, stream));
  if (nl) HIPCHK(hipMemcpyAsync(lm, P.lm[0], nl * 8, hipMemcpyDeviceToHost, stream));
  if (ni) HIPCHK(hipMemcpyAsync(imu, P.imu_state, ni * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  forWindows(B.n_win, [&](int w) {
    const okvisgpu_problem* p = probs[w];
    const double* q = pose + 7 * (size_t)B.pose_base[w];
    std::memcpy(p->poses, q, sizeof(double) * 7 * p->n_poses);
    if (B.win_ext_free[w])  // variable extrinsics are written back like every other block
      std::memcpy(p->extrinsics, q + 7 * (size_t)p->n_poses, sizeof(double) * 7 * p->n_cameras);
    std::memcpy(p->speed_biases, sb + 9 * (size_t)B.sb_base[w], sizeof(double) * 9 * p->n_speed_biases);
    const double* l = lm + 4 * (size_t)B.lm_base[w];
    const int* perm = &B.lm_perm[B.lm_base[w]];
    for (int k = 0; k < p->n_landmarks; ++k) std::memcpy(&p->landmarks[4 * (size_t)perm[k]], l + 4 * (size_t)k, 32);
    if (p->imu_state && p->n_imu)
      std::memcpy(p->imu_state, imu + (size_t)B.imu_base[w] * kImuState, sizeof(double) * kImuState * p->n_imu);
  });
}

// ViGraph::updateLandmarks on the current parameter values (okvisgpu_update_landmarks): every
// window's current set is gathered into set 0 as downloadParams does (before the first solve
// WinState is the build's zeroed scratch: xcur = 0, set 0 holds the uploaded values), one kernel
// over the batch's landmarks, one copy per output into pinned memory, and a threaded scatter into
// the caller's order (landmarks through lm_perm, observations through obs_orig). Of the caller's
// problem arrays only the re-placed landmarks are written.
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
  // device: quality [nl] | dirs [no][3] | err [no] | flags [nl]; host: quality [nl] | lm [nl][4] | err [no] | flags [nl]
  const size_t need = 8 * (nl + 4 * std::max<size_t>(no, 1)) + nl;
  double* dQ = static_cast<double*>(batchScratch.need(need));
  double *dDirs = dQ + nl, *dErr = dDirs + 3 * no;
  uint8_t* dFlags = reinterpret_cast<uint8_t*>(dErr + std::max<size_t>(no, 1));
  double* hQ = reinterpret_cast<double*>(paramStage(8 * (nl + 4 * nl + no) + nl));
  double *hLm = hQ + nl, *hErr = hLm + 4 * nl;
  uint8_t* hFlags = reinterpret_cast<uint8_t*>(hErr + no);
  launch_select_current(P, stream);
  launch_update_landmarks(P, dQ, dFlags, dErr, dDirs, stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hQ, dQ, nl * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(hLm, P.lm[0], 4 * nl * 8, hipMemcpyDeviceToHost, stream));
  if (wantErr && no) HIPCHK(hipMemcpyAsync(hErr, dErr, no * 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(hFlags, dFlags, nl, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
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
// kernels (covisFitsLds picks a window's), the caller's exclusion masks
// permuted into internal landmark order; all of it packed into pinned memory and uploaded as one
// copy. k_covis_bits writes every word of the bitset and the count kernels every element of
// counts / n_observed, so nothing is cleared. One copy back per output, then a threaded scatter;
// the pair and visibility totals are taken on the host. Reads no parameter value and writes neither
// the caller's problem arrays nor the arena.
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

  // device: uploaded part (records | word records | items0 | items1 | mask), then bits | counts | n_observed
  const size_t nl = (size_t)P.n_lm;
  Arena A;
  const size_t oRec = A.reserve(sizeof(CovisWin) * recs.size()), oWr = A.reserve(4 * wordRec.size()),
               oI0 = A.reserve(4 * items0.size()), oI1 = A.reserve(4 * items1.size()), oEx = A.reserve(anyMask ? nl : 0);
  const size_t upBytes = A.size;
  const size_t oBits = A.reserve(8 * (size_t)bitsTot), oCnt = A.reserve(4 * (size_t)cntTot),
               oObs = A.reserve(4 * (size_t)stateTot);
  char* dev = static_cast<char*>(batchScratch.need(A.size));
  // pinned: the uploaded part as on the device, then counts | n_observed as they come back
  const size_t hCntOff = (upBytes + 255) & ~size_t(255), hObsOff = hCntOff + 4 * (size_t)cntTot;
  char* host = paramStage(hObsOff + 4 * (size_t)stateTot);
  std::memcpy(host + oRec, recs.data(), sizeof(CovisWin) * recs.size());
  std::memcpy(host + oWr, wordRec.data(), 4 * wordRec.size());
  if (!items0.empty()) std::memcpy(host + oI0, items0.data(), 4 * items0.size());
  if (!items1.empty()) std::memcpy(host + oI1, items1.data(), 4 * items1.size());
  if (anyMask)
    forWindows(nwin, [&](int w) {
      const okvisgpu_problem* p = probs[w];
      uint8_t* ex = reinterpret_cast<uint8_t*>(host + oEx) + (size_t)B.lm_base[w];
      const uint8_t* in = V[w].landmark_excluded;
      const int* perm = &B.lm_perm[B.lm_base[w]];
      if (!in) std::memset(ex, 0, (size_t)std::max(p->n_landmarks, 0));
      else
        for (int k = 0; k < p->n_landmarks; ++k) ex[k] = in[perm[k]] ? 1 : 0;
    });
  HIPCHK(hipMemcpyAsync(dev, host, upBytes, hipMemcpyHostToDevice, stream));
  const CovisWin* dRec = reinterpret_cast<const CovisWin*>(dev + oRec);
  unsigned long long* dBits = reinterpret_cast<unsigned long long*>(dev + oBits);
  int32_t *dCnt = reinterpret_cast<int32_t*>(dev + oCnt), *dObs = reinterpret_cast<int32_t*>(dev + oObs);
  launch_covis_bits(P, dRec, (int)recs.size(), reinterpret_cast<const int32_t*>(dev + oWr), (int)words,
                    anyMask ? reinterpret_cast<const uint8_t*>(dev + oEx) : nullptr, dBits, stream);
  launch_covis_counts(dRec, reinterpret_cast<const int32_t*>(dev + oI0), (int)items0.size(), lds0,
                      reinterpret_cast<const int32_t*>(dev + oI1), (int)(items1.size() / 3), dBits, dCnt, dObs, stream);
  HIPCHK(hipGetLastError());
  const int32_t* hCnt = reinterpret_cast<const int32_t*>(host + hCntOff);
  const int32_t* hObs = reinterpret_cast<const int32_t*>(host + hObsOff);
  HIPCHK(hipMemcpyAsync(host + hCntOff, dCnt, 4 * (size_t)cntTot, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(host + hObsOff, dObs, 4 * (size_t)stateTot, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  forWindows(nwin, [&](int w) {
    if (recOf[w] < 0) return;
    const CovisWin& r = recs[(size_t)recOf[w]];
    okvisgpu_covisibility& v = V[w];
    const size_t S = (size_t)r.n_state;
    const int32_t *c = hCnt + r.counts_off, *o = hObs + r.state_off;
    if (v.counts) std::memcpy(v.counts, c, 4 * S * S);
    if (v.n_observed) std::memcpy(v.n_observed, o, 4 * S);
    int pairs = 0, vis = 0;
    for (size_t i = 0; i < S; ++i) {
      vis += o[i] > 0;
      if (v.visible) v.visible[i] = o[i] > 0 ? 1 : 0;
      for (size_t j = i + 1; j < S; ++j) pairs += c[i * S + j] > 0;
    }
    v.n_pairs = pairs;
    v.n_visible = vis;
    v.any = pairs > 0 ? 1 : 0;
  });
}

std::vector<WinState> okvisgpu_ctx::readStates() {
  std::vector<WinState> s(P.n_win);
  HIPCHK(hipMemcpyAsync(s.data(), P.st, sizeof(WinState) * s.size(), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  return s;
}

void okvisgpu_ctx::launchInit(int evalMode) {
  evalAll(evalMode, stream);
  launch_reduce(P, R_COST_INIT, stream);
  launch_lm_blocks(P, 0, stream);
  launch_imu_hess(P, 0, stream);
  launch_fgrad(P, 0, stream);
  launch_gradnorm(P, 0, stream);
  if (regime.lin_prep) launch_lm_prep(P, stream);  // (the first iteration's; later ones: k_lin_few, runTimed)
  HIPCHK(hipGetLastError());
}

// ---- one trust-region iteration: a table of steps, walked by three executors -------------------
// A step is a launcher, the ABI phase its device time is booked to (kPhaseNames) and the lane it
// may run on: a step on a side lane is independent of the main-lane step before it and of the
// other side lane's (disjoint data: pose-pose vs. speed/bias blocks of S; observation / IMU, prior
// and edge / host-factor records; landmark groups vs. IMU Hessians), so a main-lane step and the
// side-lane steps after it are one fork / join group.
#define STEP(phase, lane, call) Step{[](okvisgpu_ctx& c, hipStream_t s) { call; }, phase, lane}
// The iteration of every batch but a few windows on one stream, and of every eager iteration (the
// ABI's phases and the four Summary sums are per kernel, so the timed iteration stays unfused also
// where the solve it reports on runs fewSteps(): the same device code on the same data in the same
// order per buffer, and runTimed() closes with the prep that fewSteps() expects: the same bits,
// also when eager and captured iterations alternate in one solve). Phases 1 zero_S, 5 gn_finalize, 6 jv and 7 reduce_jv no longer
// launch (S is cleared once per build; the others run inside cholesky, lm_backsub and dogleg): they
// stay in the ABI's list and report 0.
const std::vector<okvisgpu_ctx::Step>& okvisgpu_ctx::unfusedSteps() {
  static const std::vector<Step> t = {
      STEP(0, MAIN, launch_lm_prep(c.P, s)),  // GN prep: only windows whose Z is stale
      STEP(2, MAIN, launch_assemble_pp(c.P, s)),
      STEP(2, SIDE0, launch_assemble_sb(c.P, s)),
      STEP(3, MAIN, launch_cholesky(c.P, s)),    // (with the f-blocks' GN vectors)
      STEP(4, MAIN, launch_lm_backsub(c.P, s)),  // (with the dogleg vectors and every J*v)
      STEP(8, MAIN, launch_dogleg(c.P, s)),
      STEP(9, MAIN, launch_eval_obs(c.P, 1, s)),  // candidate evaluation
      STEP(10, SIDE0, launch_eval_imu(c.P, 1, s)),  // (with the priors and edges)
      STEP(11, SIDE1, c.evalHost(1, s)),
      STEP(12, MAIN, launch_reduce(c.P, R_COST_CAND, s)),
      STEP(13, MAIN, launch_lm_blocks(c.P, 1, s)),  // linearisation at the accepted point
      STEP(13, SIDE0, launch_imu_hess(c.P, 1, s)),
      STEP(13, MAIN, launch_fgrad(c.P, 1, s)),
      STEP(14, MAIN, launch_gradnorm(c.P, 1, s)),
  };
  return t;
}
// Few windows on one stream (regime.fused_gradnorm; a latency chain of small launches): the
// independent kernels of a group as one launch, the GN prep inside the linearisation launch unless
// regime.lin_prep is off (then captureIterations() puts launch_lm_prep in front), and the
// gradient test of an iteration inside the next iteration's assembly launch (k_assemble_few; it
// reads nothing the assembly writes, and a window it ends is skipped from the Cholesky on).
// Invariant (prepPending()): with the prep inside the linearisation, this list starts from Z, L^-1
// and partial Schur blocks already formed for every window's current mu, so whatever ran before it
// (launchInit, the list itself, an eager iteration) must have ended with the prep of the windows
// whose step was not accepted: a mu raised by a failed Cholesky or an invalid step is otherwise
// assembled with operands of the old mu. The captured graph ends with one standalone test, so that every graph launch leaves complete window
// states; the test is idempotent (the same state gives the same norms and decision), so the
// repeat at the start of the next graph launch is harmless.
const std::vector<okvisgpu_ctx::Step>& okvisgpu_ctx::fewSteps() {
  static const std::vector<Step> t = {
      STEP(2, MAIN, launch_assemble_gradnorm_few(c.P, s)),
      STEP(3, MAIN, launch_cholesky(c.P, s)),
      STEP(4, MAIN, launch_lm_backsub(c.P, s)),
      STEP(8, MAIN, launch_dogleg(c.P, s)),
      STEP(9, MAIN, launch_eval_few(c.P, 1, s)),
      STEP(11, MAIN, c.evalHost(1, s)),
      STEP(12, MAIN, launch_reduce(c.P, R_COST_CAND, s)),
      STEP(13, MAIN, launch_lin_few(c.P, s)),
      STEP(13, MAIN, launch_fgrad(c.P, 1, s)),
  };
  return t;
}
#undef STEP

// Serial executor (one-stream capture): the lanes are ignored.
void okvisgpu_ctx::runSerial(const std::vector<Step>& steps) {
  for (const Step& st : steps) st.launch(*this, stream);
}
// Forked executor (capture with fork streams, so the graph runs a group's kernels concurrently):
// per group, the side lanes wait for an event of the main stream, the side-lane steps are
// captured, then the main-lane step, and the main stream waits for an event of each side lane.
// Every fork and join of one capture has its own event.
void okvisgpu_ctx::runForked(const std::vector<Step>& steps) {
  hipStream_t lane[3] = {stream, side[0], side[1]};
  auto edge = [&](hipStream_t from, hipStream_t to) {
    if (forkEvUsed == forkEv.size()) {
      hipEvent_t e;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      forkEv.push_back(e);
    }
    hipEvent_t e = forkEv[forkEvUsed++];
    HIPCHK(hipEventRecord(e, from));
    HIPCHK(hipStreamWaitEvent(to, e, 0));
  };
  for (size_t i = 0, j; i < steps.size(); i = j) {
    for (j = i + 1; j < steps.size() && steps[j].lane != MAIN;) ++j;
    for (size_t k = i + 1; k < j; ++k) edge(stream, lane[steps[k].lane]);
    for (size_t k = i + 1; k < j; ++k) steps[k].launch(*this, lane[steps[k].lane]);
    steps[i].launch(*this, stream);
    for (size_t k = i + 1; k < j; ++k) edge(lane[steps[k].lane], stream);
  }
}
// Eager executor (okvisgpu_profile_iteration and the verbose solve): the unfused steps on the
// context's stream with a HIP event after each; ms[phase] += the step's device time. Where the
// captured graph is fewSteps() the iteration closes with the GN prep (the first step again, phase
// 0), as k_lin_few does there: captured iterations may follow.
void okvisgpu_ctx::runTimed(double* ms) {
  std::vector<Step> steps = unfusedSteps();
  if (prepPending()) steps.push_back(steps.front());
  std::vector<hipEvent_t> ev(steps.size() + 1);
  for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(ev[0], stream));
  for (size_t i = 0; i < steps.size(); ++i) {
    steps[i].launch(*this, stream);
    HIPCHK(hipEventRecord(ev[i + 1], stream));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(stream));
  for (size_t i = 0; i < steps.size(); ++i) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
    ms[steps[i].phase] += t;
  }
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
}

// k iterations captured as one graph, as the regime lays them out
hipGraphExec_t okvisgpu_ctx::captureIterations(int k) {
  hipGraph_t g;
  hipGraphExec_t exec = nullptr;
  HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
  forkEvUsed = 0;
  for (int i = 0; i < k; ++i) {
    if (regime.fused_gradnorm && !prepPending()) launch_lm_prep(P, stream);
    if (regime.fused_gradnorm) runSerial(fewSteps());
    else if (regime.serial_graph) runSerial(unfusedSteps());
    else runForked(unfusedSteps());
  }
  if (regime.fused_gradnorm) launch_gradnorm(P, 1, stream);
  HIPCHK(hipStreamEndCapture(stream, &g));
  HIPCHK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
  HIPCHK(hipGraphDestroy(g));
  return exec;
}
void okvisgpu_ctx::ensureGraph() {
  if (iterGraph) return;
  iterGraph = captureIterations(1);
  if (regime.graph_iters > 1) {
    iterGraphK = captureIterations(regime.graph_iters);
    graphIters = regime.graph_iters;
  }
}

namespace {
thread_local std::string g_err;
}

int okg::fail(okvisgpu_ctx* c, int code, const std::string& m) {
  if (c) c->last_error = m;
  g_err = m;
  return code;
}

extern "C" {

int okvisgpu_abi_version(void) { return OKVISGPU_ABI_VERSION; }

int okvisgpu_loss_evaluate(const okvisgpu_loss* loss, double s, double* rho) {
  if (!loss || !rho || !lossValid(*loss)) return fail(nullptr, OKVISGPU_ERR_INVALID_ARGUMENT, "loss_evaluate: bad loss");
  lossRho(*loss, s, rho);
  return OKVISGPU_OK;
}

void okvisgpu_default_options(okvisgpu_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_num_iterations = 50;  // ::ceres::Solver::Options default
  o->linear_solver = OKVISGPU_DENSE_SCHUR;
  o->trust_region_strategy = OKVISGPU_DOGLEG;
  o->jacobi_scaling = 1;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->time_limit_s = -1.0;
  o->min_iterations = 0;
  o->redo_propagation_always = 0;
  o->num_threads = 1;
  o->verbose = 0;
  o->cholesky_schedule = 0;
}

int okvisgpu_device_count(int32_t* count) {
  if (!count) return OKVISGPU_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return OKVISGPU_OK;
}

int okvisgpu_ctx_create(int32_t device, okvisgpu_ctx** out) {
  if (!out) return OKVISGPU_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(nullptr, OKVISGPU_ERR_DEVICE, "no HIP device");
  if (device < 0 || device >= n) return fail(nullptr, OKVISGPU_ERR_INVALID_ARGUMENT, "bad device index");
  auto* c = new okvisgpu_ctx();
  c->device = device;
  const int rc = guarded(c, [&]() {
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
      throw HipError{std::string("okvisgpu is built for gfx950 only; device is ") + prop.gcnArchName,
                     OKVISGPU_ERR_DEVICE};
    c->cuCount = prop.multiProcessorCount;
    c->ldsPerBlock = prop.sharedMemPerBlock;
    c->persistentLds = cholesky_persistent_lds();
    c->pipeLds = cholesky_pipe_lds();
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (hipStream_t& q : c->side) HIPCHK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
    return (int)OKVISGPU_OK;
  });
  if (rc != OKVISGPU_OK) {
    delete c;
    return rc;
  }
  *out = c;
  return OKVISGPU_OK;
}

int okvisgpu_ctx_destroy(okvisgpu_ctx* c) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(c->device);
  delete c;
  return OKVISGPU_OK;
}

const char* okvisgpu_last_error(const okvisgpu_ctx* c) { return c ? c->last_error.c_str() : g_err.c_str(); }

int okvisgpu_set_problems(okvisgpu_ctx* c, const okvisgpu_problem* problems, int32_t n) {
  if (!c || !problems || n <= 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "set_problems: bad arguments");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->probs.clear();
    for (int i = 0; i < n; ++i) c->probs.push_back(&problems[i]);
    c->constOverride.clear();
    c->build();
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_update_params(okvisgpu_ctx* c) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->uploadParams();
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_set_block_constant(okvisgpu_ctx* c, int32_t window, int32_t kind, int32_t index, int32_t is_const) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= (int)c->probs.size() || kind < 0 || kind > 3)
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "set_block_constant: bad window/kind");
  const okvisgpu_problem* p = c->probs[window];
  const int n = kind == 0 ? p->n_poses : kind == 1 ? p->n_speed_biases : kind == 2 ? p->n_landmarks : p->n_cameras;
  if (index < 0 || index >= n) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "set_block_constant: bad index");
  c->constOverride[std::make_tuple(window, kind, index)] = is_const ? 1 : 0;
  c->structureDirty = true;
  return OKVISGPU_OK;
}

int okvisgpu_get_params(okvisgpu_ctx* c) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->downloadParams();
    return (int)OKVISGPU_OK;
  });
}

static int checkSolveOptions(okvisgpu_ctx* c, const okvisgpu_options* o) {
  if (!c || !o) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  // SPARSE_NORMAL_CHOLESKY (the full graph's option, ViGraph.cpp:248) solves the same normal
  // equations; the step is formed through the exact tile-sparse Schur complement either way
  if ((o->linear_solver != OKVISGPU_DENSE_SCHUR && o->linear_solver != OKVISGPU_SPARSE_NORMAL_CHOLESKY) ||
      o->trust_region_strategy != OKVISGPU_DOGLEG)
    return fail(c, OKVISGPU_ERR_UNSUPPORTED,
                "linear solver must be DENSE_SCHUR or SPARSE_NORMAL_CHOLESKY and the strategy DOGLEG");
  if (o->max_num_iterations < 0) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "max_num_iterations < 0");
  return OKVISGPU_OK;
}

int okvisgpu_solve_begin(okvisgpu_ctx* c, const okvisgpu_options* o) {
  const int rc = checkSolveOptions(c, o);
  if (rc != OKVISGPU_OK) return rc;
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->solveT0 = nowS();
    c->opts = *o;
    c->replays = 0;
    if (c->structureDirty) c->build();  // freeze / unfreeze changed the free set
    c->setOptions(*o);
    c->dropGraph();  // options are baked into the captured kernel arguments
    c->uploadParams();
    c->resetStates(1e-8);
    c->ensureS(c->stream);
    c->launchInit(2);
    c->failInitialHostEvaluations();
    c->ensureGraph();
    c->inSolve = true;
    c->phasesTimed = false;
    for (double& t : c->phaseMs) t = 0.0;
    c->tIterStart = nowS();
    c->tPre = c->tIterStart - c->solveT0;
    c->tMin = c->tPost = 0.0;
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_solve_iterate(okvisgpu_ctx* c, int32_t n) {
  if (!c || n < 0) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "solve_iterate without solve_begin");
  return guarded(c, [&]() {
    c->launchIterations(n);
    c->replays += n;
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_synchronize(okvisgpu_ctx* c) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  return guarded(c, [&]() {
    HIPCHK(hipStreamSynchronize(c->stream));
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_solve_end(okvisgpu_ctx* c, okvisgpu_summary* sums) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "solve_end without solve_begin");
  return guarded(c, [&]() {
    const okvisgpu_options& o = c->opts;
    const int maxReplays = std::max(1, o.max_num_iterations) * 8 + 8;
    std::vector<WinState> st = c->readStates();
    // windows that consumed passes on mu-retries (ComputeGaussNewtonStep loop) finish here
    while (c->replays < maxReplays) {
      bool allDone = true;
      for (auto& s : st) allDone = allDone && s.done;
      if (allDone) break;
      c->launchIterations(1);
      ++c->replays;
      st = c->readStates();
    }
    c->finish(st, sums);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_solve(okvisgpu_ctx* c, const okvisgpu_options* o, okvisgpu_summary* sums) {
  int rc = okvisgpu_solve_begin(c, o);
  if (rc != OKVISGPU_OK) return rc;
  if (o->time_limit_s < 0.0 && !o->verbose) {
    rc = okvisgpu_solve_iterate(c, o->max_num_iterations);
    if (rc != OKVISGPU_OK) return rc;
    return okvisgpu_solve_end(c, sums);
  }
  // One iteration at a time (states read back after each): CeresIterationCallback
  // (CeresIterationCallback.cpp:30-38): after the minimum number of iterations, stop once the next
  // iteration would exceed the time budget; verbose: eager iterations timed per phase (the Ceres
  // Summary timing fields, FullReport at ViGraph.cpp:1887-1889).
  return guarded(c, [&]() {
    c->phasesTimed = o->verbose != 0;
    std::vector<WinState> st = c->readStates();
    double iterStart = nowS();
    const int maxReplays = std::max(1, o->max_num_iterations) * 8 + 8;
    while (c->replays < maxReplays) {
      bool allDone = true;
      for (auto& s : st) allDone = allDone && s.done;
      if (allDone) break;
      const double now = nowS();
      const double iterTime = now - iterStart, cum = now - c->solveT0;
      bool changed = false;
      for (auto& s : st)
        if (o->time_limit_s >= 0.0 && !s.done && s.iteration >= o->min_iterations && cum + iterTime > o->time_limit_s) {
          s.done = 1;
          s.termination = OKVISGPU_USER_SUCCESS;
          changed = true;
        }
      if (changed) {
        HIPCHK(hipMemcpyAsync(c->P.st, st.data(), sizeof(WinState) * st.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        continue;
      }
      iterStart = nowS();
      if (o->verbose) c->runTimed(c->phaseMs);
      else c->launchIterations(1);
      ++c->replays;
      st = c->readStates();
    }
    c->finish(st, sums);
    return (int)OKVISGPU_OK;
  });
}

static const char* kPhaseNames[OKVISGPU_N_PHASES] = {
    "lm_prep",     "zero_S",   "assemble",   "cholesky",  "lm_backsub", "gn_finalize",
    "jv",          "reduce_jv", "dogleg",   "eval_obs",
    "eval_imu",    "eval_priors", "reduce_cand", "lin_blocks", "gradnorm"};

const char* okvisgpu_phase_name(int32_t i) { return (i >= 0 && i < OKVISGPU_N_PHASES) ? kPhaseNames[i] : ""; }

int okvisgpu_profile_iteration(okvisgpu_ctx* c, double* ms) {
  if (!c || !ms) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "profile_iteration needs solve_begin");
  return guarded(c, [&]() {
    for (int i = 0; i < OKVISGPU_N_PHASES; ++i) ms[i] = 0.0;
    c->runTimed(ms);
    c->replays += 1;
    return (int)OKVISGPU_OK;
  });
}

// ---- per-kernel timing with algorithmic work models (bench.py's roofline) ------------------
namespace {
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

int okvisgpu_kernel_count(void) { return K_COUNT; }
const char* okvisgpu_kernel_name(int32_t k) { return (k >= 0 && k < K_COUNT) ? kKernelNames[k] : ""; }

int okvisgpu_time_kernel(okvisgpu_ctx* c, int32_t kernel, int32_t reps, double* avg_ms, double* work,
                         int32_t* bound) {
  if (!c || kernel < 0 || kernel >= K_COUNT || reps < 1) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "time_kernel: call after solve_end");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
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

int okvisgpu_plan_window(const okvisgpu_problem* p, int32_t nested_dissection, int64_t* info, uint8_t* tile_nz,
                         int32_t* step_launch, int32_t* natural) {
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

int okvisgpu_evaluate(okvisgpu_ctx* c, int32_t window, double* cost) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
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
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
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
    // exported in the natural order (pose i, speed/bias i, ..., extrinsics), whatever order the
    // window's S is held in (nested dissection: permuted slots and gap rows)
    const int fdim = c->B.win_fdim[window], fpad = c->B.win_fpad[window], dn = c->B.win_fnat[window];
    const int32_t* nat = c->B.f_nat.data() + c->B.win_foff[window];
    if (dim_out) *dim_out = dn;
    if (cost) *cost = st[window].x_cost + st[window].fixed_cost;
    if (S && dn) {
      std::vector<double> full((size_t)fpad * fpad);
      HIPCHK(hipMemcpy(full.data(), c->P.S + c->B.win_soff[window], full.size() * 8, hipMemcpyDeviceToHost));
      for (int r = 0; r < fdim; ++r)
        for (int q = 0; q <= r; ++q) {
          const int a = nat[r], b = nat[q];
          if (a < 0 || b < 0) continue;
          S[(size_t)a * dn + b] = full[(size_t)r * fpad + q];
          S[(size_t)b * dn + a] = full[(size_t)r * fpad + q];
        }
    }
    if (rhs && dn) {
      std::vector<double> v(fdim);
      HIPCHK(hipMemcpy(v.data(), c->P.rhsF + c->B.win_foff[window], sizeof(double) * fdim, hipMemcpyDeviceToHost));
      for (int r = 0; r < fdim; ++r)
        if (nat[r] >= 0) rhs[nat[r]] = v[r];
    }
    if (st[window].gn_failed) return fail(c, OKVISGPU_ERR_NUMERICAL, "landmark block not positive definite");
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_gauss_newton_step(okvisgpu_ctx* c, int32_t window, const okvisgpu_options* options, double mu,
                               double* y_f, double* y_l, int32_t* dim_out) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "gauss_newton_step: call after solve_end");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
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
    if (y_f && dn) {  // natural order, as okvisgpu_linearize_reduce exports rhs
      const int32_t* nat = B.f_nat.data() + B.win_foff[window];
      std::vector<double> v(fdim);
      HIPCHK(hipMemcpy(v.data(), c->P.yF + B.win_foff[window], sizeof(double) * fdim, hipMemcpyDeviceToHost));
      for (int r = 0; r < fdim; ++r)
        if (nat[r] >= 0) y_f[nat[r]] = v[r];
    }
    const int nl = c->probs[window]->n_landmarks;
    if (y_l && nl) {  // the caller's landmark order
      const int lb = B.lm_base[window];
      const int* perm = &B.lm_perm[lb];
      std::vector<double> v(3 * (size_t)nl);
      HIPCHK(hipMemcpy(v.data(), c->P.yL + 3 * (size_t)lb, sizeof(double) * v.size(), hipMemcpyDeviceToHost));
      for (int k = 0; k < nl; ++k)
        for (int a = 0; a < 3; ++a) y_l[3 * (size_t)perm[k] + a] = B.lm_free[lb + k] ? v[3 * (size_t)k + a] : 0.0;
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_eval_reprojection(okvisgpu_ctx* c, int32_t window, double* r, double* Jp, double* Jl) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->resetStates(1e-8);
    launch_eval(c->P, 3, c->stream);
    HIPCHK(hipGetLastError());
    const int64_t S = c->P.obs_stride;
    std::vector<double> lin((size_t)kObsLin * S);
    HIPCHK(hipMemcpyAsync(lin.data(), c->P.obs_lin[0], lin.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
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
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    okvisgpu_options o;
    okvisgpu_default_options(&o);
    o.redo_propagation_always = redo_always;
    c->setOptions(o);
    c->resetStates(1e-8);
    launch_eval(c->P, 3, c->stream);
    HIPCHK(hipGetLastError());
    const int n = c->probs[window]->n_imu, ib = c->B.imu_base[window];
    std::vector<double> lin((size_t)kImuLin * std::max(1, n));
    if (n) HIPCHK(hipMemcpyAsync(lin.data(), c->P.imu_lin[0] + (size_t)ib * kImuLin, (size_t)kImuLin * n * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int f = 0; f < n; ++f) {
      if (r) for (int i = 0; i < 15; ++i) r[15 * f + i] = lin[(size_t)f * kImuLin + i];
      if (J) for (int i = 0; i < 450; ++i) J[450 * (size_t)f + i] = lin[(size_t)f * kImuLin + 15 + i];
    }
    // keep the caller's ImuError state in sync (the evaluation may have re-integrated)
    c->downloadParams();
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_eval_relpose(okvisgpu_ctx* c, int32_t window, double* r, double* J) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->resetStates(1e-8);
    launch_eval(c->P, 3, c->stream);
    HIPCHK(hipGetLastError());
    const int n = c->probs[window]->n_relpose, rb = c->B.rp_base[window];
    std::vector<double> lin((size_t)kRelPoseLin * std::max(1, n));
    if (n) HIPCHK(hipMemcpyAsync(lin.data(), c->P.rp_lin[0] + (size_t)rb * kRelPoseLin, (size_t)kRelPoseLin * n * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {
      if (r) for (int k = 0; k < 6; ++k) r[6 * i + k] = lin[(size_t)i * kRelPoseLin + k];
      if (J) for (int k = 0; k < 72; ++k) J[72 * (size_t)i + k] = lin[(size_t)i * kRelPoseLin + 6 + k];
    }
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_eval_host(okvisgpu_ctx* c, int32_t window, double* r, double* J) {
  if (!c) return OKVISGPU_ERR_INVALID_ARGUMENT;
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (window < 0 || window >= c->P.n_win) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "bad window");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->resetStates(1e-8);
    c->evalHost(3, c->stream);
    HIPCHK(hipGetLastError());
    const int h0 = c->B.win_host_range[2 * window], n = c->B.win_host_range[2 * window + 1] - h0;
    std::vector<double> lin((size_t)kImuLin * std::max(1, n));
    if (n) HIPCHK(hipMemcpyAsync(lin.data(), c->P.imu_lin[0] + (size_t)h0 * kImuLin, (size_t)kImuLin * n * 8,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int f = 0; f < n; ++f) {
      if (r) for (int i = 0; i < 15; ++i) r[15 * f + i] = lin[(size_t)f * kImuLin + i];
      if (J) for (int i = 0; i < 450; ++i) J[450 * (size_t)f + i] = lin[(size_t)f * kImuLin + 15 + i];
    }
    for (int f = 0; f < n; ++f)
      if (c->hostFail[h0 - c->P.n_imu + f]) return fail(c, OKVISGPU_ERR_NUMERICAL, "host_evaluate failed");
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_update_landmarks(okvisgpu_ctx* c, okvisgpu_landmark_update* updates) {
  if (!c || !updates) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "update_landmarks: bad arguments");
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "update_landmarks: call after solve_end");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->updateLandmarks(updates);
    return (int)OKVISGPU_OK;
  });
}

int okvisgpu_covisibilities(okvisgpu_ctx* c, okvisgpu_covisibility* out) {
  if (!c || !out) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "covisibilities: bad arguments");
  if (!c->haveProblem) return fail(c, OKVISGPU_ERR_NO_PROBLEM, "no problem set");
  if (c->inSolve) return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, "covisibilities: call after solve_end");
  return guarded(c, [&]() {
    HIPCHK(hipSetDevice(c->device));
    c->covisibilities(out);
    return (int)OKVISGPU_OK;
  });
}

}  // extern "C"
