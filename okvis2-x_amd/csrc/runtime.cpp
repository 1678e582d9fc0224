// runtime.cpp — the solver path of the okvisgpu C ABI (include/okvisgpu.h), and nothing else.
//
// The drop-in replacement for `::ceres::Solve(options_, problem_.get(), &summary_)` in
// okvis::ViGraph::optimise (okvis_ceres/src/ViGraph.cpp:1844-1890): structure analysis of each
// window and the arena layout (plan.cpp), one HBM arena per context, upload, and the trust-region
// iteration as a captured hipGraph that is replayed max_num_iterations times with every decision
// taken on the device (kernels_control.hip). The host synchronises once per solve (plus once per
// iteration only when a CeresIterationCallback-style time limit is requested). The entry points that
// read the resident batch are in resident_calls.cpp, the call-scoped batch entry points in
// batch_calls.cpp; the context all three work on is declared in runtime.hpp.
#include "runtime.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "launch.hpp"
#include "loss.hpp"

using namespace okg;

static double nowS() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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
  // k_eval_imu_steady's byte per factor wavefront (four factors each): likewise the context's own
  P.imu_wave_redo = static_cast<uint8_t*>(imuWaveRedoBuf.need(std::max<size_t>(64, ((size_t)P.n_imu + 3) / 4)));
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

static thread_local std::string g_err;

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

}  // extern "C"
