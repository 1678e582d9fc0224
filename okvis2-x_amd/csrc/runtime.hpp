// runtime.hpp — what the host files behind the C ABI share: the context (okvisgpu_ctx), the error
// plumbing of the entry points (HIPCHK / HipError, fail, guarded) and the buffers a context owns.
// runtime.cpp holds the solver path; resident_calls.cpp the entry points that read the resident
// batch; batch_calls.cpp the call-scoped batch entry points, which use a context only for its
// stream, its pinned staging buffer and batchScratch.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/okvisgpu.h"
#include "batch_stage.hpp"
#include "device_problem.hpp"
#include "plan.hpp"

namespace okg {

struct HipError {
  std::string msg;
  int code;
};

#define HIPCHK(x)                                                                             \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess)                                                                     \
      throw okg::HipError{std::string(#x) + ": " + hipGetErrorString(e_),                     \
                          e_ == hipErrorOutOfMemory ? OKVISGPU_ERR_OUT_OF_MEMORY : OKVISGPU_ERR_DEVICE}; \
  } while (0)

// A device buffer that only grows: need(bytes) returns at least that many bytes, reallocating (the
// contents are not kept) when the buffer is smaller; a failed allocation leaves it empty.
struct GrowBuffer {
  GrowBuffer() = default;
  GrowBuffer(const GrowBuffer&) = delete;
  GrowBuffer& operator=(const GrowBuffer&) = delete;
  ~GrowBuffer() { release(); }
  void* need(size_t bytes) {
    if (bytes > cap_) {
      release();
      HIPCHK(hipMalloc(&ptr_, bytes));
      cap_ = bytes;
    }
    return ptr_;
  }

 private:
  void release() {
    if (ptr_) (void)hipFree(ptr_);
    ptr_ = nullptr;
    cap_ = 0;
  }
  void* ptr_ = nullptr;
  size_t cap_ = 0;
};

// Persistent host worker threads of one context: the host-evaluated factors (ABI 5) are evaluated
// at every point the solver evaluates, from the HIP callback thread of the iteration graph's host
// node, so the workers are created once (grown on demand) instead of per evaluation. run(n, f)
// calls f(0..n-1) on n workers and returns when all are done.
class HostWorkers {
 public:
  ~HostWorkers() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    wake_.notify_all();
    for (auto& t : th_) t.join();
  }
  void run(int n, const std::function<void(int)>& f) {
    while ((int)th_.size() < n) {
      const int id = (int)th_.size();
      th_.emplace_back([this, id]() { loop(id); });
    }
    std::unique_lock<std::mutex> l(m_);
    job_ = &f;
    njob_ = n;
    pending_ = n;
    ++gen_;
    wake_.notify_all();
    done_.wait(l, [&]() { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  void loop(int id) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> l(m_);
    for (;;) {
      wake_.wait(l, [&]() { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      if (id >= njob_) continue;
      const std::function<void(int)>* f = job_;
      l.unlock();
      (*f)(id);
      l.lock();
      if (--pending_ == 0) done_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable wake_, done_;
  const std::function<void(int)>* job_ = nullptr;
  int njob_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

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

}  // namespace okg

struct okvisgpu_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side[3] = {nullptr, nullptr, nullptr};  // fork streams of the captured iteration graph
  std::vector<hipEvent_t> forkEv;
  size_t forkEvUsed = 0;  // events of forkEv taken by the capture in progress
  std::string last_error;
  okg::HostBatch B;
  std::vector<const okvisgpu_problem*> probs;
  std::map<std::tuple<int, int, int>, int> constOverride;
  void* hostStage = nullptr;  // pinned staging of the uploaded arrays (kept between set_problems)
  size_t hostStageBytes = 0;
  size_t arenaCap = 0;        // bytes allocated at `arena` (reused while a new batch fits)
  bool structureDirty = false;
  okg::DevProblem P{};
  void* arena = nullptr;
  size_t arenaBytes = 0;
  // The captured iteration, and graphIters = regime.graph_iters iterations captured as one graph as
  // well (iterGraphK): solve_iterate runs n iterations as n / K launches of it and n mod K of the single one.
  hipGraphExec_t iterGraph = nullptr, iterGraphK = nullptr;
  int graphIters = 1;  // the K iterGraphK was captured with
  int cuCount = 256;
  size_t ldsPerBlock = 65536, persistentLds = 0, pipeLds = 0;  // device LDS; static LDS of the two Cholesky kernels
  // The launch regime (plan.hpp), decided by setOptions() at solve_begin and, with default options,
  // after a build; the launchers read its copy in P. The measurement switches are parsed here, once
  // per decision: OKVISGPU_SERIAL_GRAPH=0|1, OKVISGPU_LIN_PREP=0, OKVISGPU_GRAPH_ITERS=<K>.
  okg::LaunchRegime regime;
  bool sNeedsInit = true;  // ensureS()
  bool haveProblem = false;
  // split-solve state
  bool inSolve = false;
  okvisgpu_options opts{};
  int replays = 0;
  double solveT0 = 0.0;
  // summary timings (okvisgpu_summary, ABI 6): wall clock of begin / iterations / write-back, and
  // the iterations' device time per phase when the solve ran them eagerly (options.verbose)
  double tPre = 0.0, tIterStart = 0.0, tMin = 0.0, tPost = 0.0;
  bool phasesTimed = false;
  double phaseMs[OKVISGPU_N_PHASES] = {};
  // host-evaluated factors (ABI 5): pinned copies of host_in / host_out and per-factor failure
  // flags of the last evaluation, written by hostEvaluate() on the HIP callback thread
  double* hostIn = nullptr;
  double* hostOut = nullptr;
  int hostBufFactors = 0;
  std::vector<uint8_t> hostFail;
  okg::HostWorkers hostWorkers;
  // The device arrays of whichever call laid out by a BatchLayout is running: the batch calls of
  // batch_calls.cpp, okvisgpu_update_landmarks and okvisgpu_covisibilities
  // (resident_calls.cpp). The context's own, outside the arena table, grown as needed. Each of
  // these calls ends in a stream synchronise, so no two use it at once; what a call finds in it is
  // whatever an earlier call of any of them left, and no kernel reads an array it was not given.
  okg::GrowBuffer batchScratch;
  // the assembly work items as records (HostBatch::asm_rec, DevProblem::asm_rec): likewise outside
  // the arena table, uploaded by build(), kept until the next build
  okg::GrowBuffer asmRecBuf;
  // DevProblem::imu_wave_redo, one byte per wavefront of IMU factors: sized by build(), written by
  // k_eval_imu_steady in every launch before k_eval_imu<false> reads it
  okg::GrowBuffer imuWaveRedoBuf;

  ~okvisgpu_ctx();

  // ---- the staging of one call's arrays (batch_stage.hpp): declare, beginBatch, optional fills
  // through S.host(), uploadBatch, launch, finishBatch ----
  // Commits the layout, sizes the pinned stage and batchScratch for it, points the declared fields
  // into batchScratch and copies the declared sources into the stage.
  void beginBatch(okg::BatchLayout& S) {
    S.commit();
    char* host = paramStage(S.downEnd());  // (synchronises: nothing still uses either buffer)
    S.begin(host, static_cast<char*>(batchScratch.need(S.size())));
  }
  void uploadBatch(const okg::BatchLayout& S) {
    HIPCHK(hipMemcpyAsync(S.devBase(), S.hostBase(), S.upEnd(), hipMemcpyHostToDevice, stream));
  }
  // One copy down, the synchronise, and every output to its destination.
  void finishBatch(const okg::BatchLayout& S) {
    const size_t b = S.downBegin(), n = S.downEnd() - b;
    if (n) HIPCHK(hipMemcpyAsync(S.hostBase() + b, S.devBase() + b, n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    S.deliver();
  }
  char* paramStage(size_t bytes);

  // ---- the solver path (runtime.cpp) ----
  void decideRegime(int schedule);
  void ensureS(hipStream_t s);
  void fillSummaries(const std::vector<okg::WinState>& st, okvisgpu_summary* sums);
  void finish(const std::vector<okg::WinState>& st, okvisgpu_summary* sums);
  void dropGraph();
  void launchIterations(int n);
  void ensureHostBuffers();
  static void posePlusJacobian(const double* x, double* J);
  void hostEvaluateOne(int h);
  void hostEvaluate();
  static void hostEvaluateCallback(void* self) { static_cast<okvisgpu_ctx*>(self)->hostEvaluate(); }
  void evalHost(int mode, hipStream_t s);
  void evalAll(int mode, hipStream_t s);
  void failInitialHostEvaluations();
  void build();
  void uploadDescriptor();
  void setOptions(const okvisgpu_options& o);
  void resetStates(double mu);
  void uploadParams();
  void downloadParams();
  void updateLandmarks(okvisgpu_landmark_update* U);  // (these two: resident_calls.cpp)
  void covisibilities(okvisgpu_covisibility* V);
  std::vector<okg::WinState> readStates();
  void launchInit(int evalMode);

  // One trust-region iteration is a table of steps, walked by three executors (runtime.cpp). A step
  // is a launcher, the ABI phase its device time is booked to (kPhaseNames) and the lane it may run on.
  enum Lane { MAIN = 0, SIDE0 = 1, SIDE1 = 2 };
  struct Step {
    void (*launch)(okvisgpu_ctx& c, hipStream_t s);
    int phase, lane;
  };
  static const std::vector<Step>& unfusedSteps();
  static const std::vector<Step>& fewSteps();
  // fewSteps() follows and will not start with the GN prep: what runs before it must end with one
  bool prepPending() const { return regime.fused_gradnorm && regime.lin_prep; }
  void runSerial(const std::vector<Step>& steps);
  void runForked(const std::vector<Step>& steps);
  void runTimed(double* ms);
  hipGraphExec_t captureIterations(int k);
  void ensureGraph();
};

namespace okg {

// An entry point's failure: the text goes to the context (okvisgpu_last_error) and the code is returned.
int fail(okvisgpu_ctx* c, int code, const std::string& m);

template <class F>
int guarded(okvisgpu_ctx* c, F f) {
  try {
    return f();
  } catch (const HipError& e) {
    return fail(c, e.code, e.msg);
  } catch (const ArgError& e) {
    return fail(c, OKVISGPU_ERR_INVALID_ARGUMENT, e.msg);
  } catch (const UnsupportedError& e) {
    return fail(c, OKVISGPU_ERR_UNSUPPORTED, e.msg);
  } catch (const std::bad_alloc&) {
    return fail(c, OKVISGPU_ERR_OUT_OF_MEMORY, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(c, OKVISGPU_ERR_DEVICE, e.what());
  }
}

}  // namespace okg
