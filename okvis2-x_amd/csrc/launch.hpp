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
void launch_lm_backsub(const DevProblem& P, hipStream_t s);  // kernels_backsub.hip: + landmark dogleg vectors, J*v
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


// post-solve landmark pass (kernels_landmarks.hip): ViGraph::updateLandmarks on parameter set 0 (run
// launch_select_current first), one lane per landmark. Outputs in device order: quality [n_lm],
// flags [n_lm] (kLmInitialised | kLmReset | kLmNotInFront), obs_err [n_obs]; dirs [n_obs][3] is
// scratch. Re-placed landmarks are written to both parameter sets.
constexpr uint8_t kLmInitialised = 1, kLmReset = 2, kLmNotInFront = 4;
void launch_update_landmarks(const DevProblem& P, double* quality, uint8_t* flags, double* obs_err, double* dirs,
                             hipStream_t s);

}  // namespace okg
