/*
 * okvisgpu.h — C ABI of the MI355X-native sliding-window bundle-adjustment backend.
 *
 * This is the drop-in boundary that replaces `::ceres::Solve(options_, problem_.get(), &summary_)`
 * inside `okvis::ViGraph::optimise()` (reference: okvis_ceres/src/ViGraph.cpp:1844-1890, the call
 * itself at :1884). Everything the reference hands to Ceres through the `::ceres::Problem` subset
 *  is handed over here as plain structure-of-arrays host buffers; the library copies
 * them to device memory, solves on the GPU, and writes the optimised parameter blocks back into
 * the SAME caller-owned host arrays (the reference's in-place ParameterBlock semantics,
 * okvis_ceres/include/okvis/ceres/PoseParameterBlock.hpp:62-78).
 *
 * Conventions (all FP64, host memory, caller-owned; the library never frees caller memory):
 *   pose / extrinsics block : [t_x t_y t_z q_x q_y q_z q_w]   (PoseParameterBlock, 7 doubles)
 *   speed-and-bias block    : [v(3) b_g(3) b_a(3)]            (SpeedAndBiasParameterBlock, 9)
 *   landmark block          : [x y z w] homogeneous            (HomogeneousPointParameterBlock, 4)
 *   time stamps             : int64 nanoseconds (okvis::Time sec/nsec, okvis_time/.../Time.hpp:124)
 *
 * No C++ exceptions cross this boundary. Every entry point returns an okvisgpu_status; the text
 * of the last error of a context is available from okvisgpu_last_error().
 *
 * Threading (SURVEY.md §8b "Threading"): one okvisgpu_ctx per graph (realtime graph, full graph);
 * each context owns one HIP stream and its device buffers. Entry points are re-entrant across
 * contexts, not within one.
 */
#ifndef OKVISGPU_H_
#define OKVISGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OKVISGPU_ABI_VERSION 6

/* ---------------------------------------------------------------- status codes */
typedef enum okvisgpu_status {
  OKVISGPU_OK = 0,
  OKVISGPU_ERR_INVALID_ARGUMENT = 1,
  OKVISGPU_ERR_UNSUPPORTED = 2,     /* a problem feature the GPU path does not implement yet */
  OKVISGPU_ERR_DEVICE = 3,          /* HIP runtime error / no device / kernel image missing   */
  OKVISGPU_ERR_OUT_OF_MEMORY = 4,
  OKVISGPU_ERR_NO_PROBLEM = 5,
  OKVISGPU_ERR_NUMERICAL = 6
} okvisgpu_status;

/* ---------------------------------------------------------------- enums mirroring Ceres/okvis */
typedef enum okvisgpu_distortion {
  OKVISGPU_DIST_NONE = 0,           /* okvis_cv/.../NoDistortion.hpp */
  OKVISGPU_DIST_RADTAN = 1,         /* okvis_cv/.../implementation/RadialTangentialDistortion.hpp:70-137 */
  OKVISGPU_DIST_EQUIDISTANT = 2,    /* okvis_cv/.../implementation/EquidistantDistortion.hpp:67-188 */
  OKVISGPU_DIST_RADTAN8 = 3         /* okvis_cv/.../implementation/RadialTangentialDistortion8.hpp:88-170 */
} okvisgpu_distortion;

typedef enum okvisgpu_linear_solver {
  OKVISGPU_DENSE_SCHUR = 0,         /* ViSlamBackend.cpp:877 realtime graph */
  OKVISGPU_SPARSE_NORMAL_CHOLESKY = 1 /* ViGraph.cpp:248 (full graph, ViSlamBackend.cpp:1988-1997):
                                       the Gauss-Newton step solves the same normal equations; it
                                       is computed through the exact tile-sparse Schur complement
                                       (landmarks eliminated, band-envelope LLT of the reduced
                                       matrix), so both options give the same step up to rounding */
} okvisgpu_linear_solver;

typedef enum okvisgpu_tr_strategy {
  OKVISGPU_DOGLEG = 0               /* ViGraph.cpp:249 (traditional dogleg) */
} okvisgpu_tr_strategy;

typedef enum okvisgpu_termination {  /* ::ceres::TerminationType subset */
  OKVISGPU_CONVERGENCE = 0,
  OKVISGPU_NO_CONVERGENCE = 1,
  OKVISGPU_FAILURE = 2,
  OKVISGPU_USER_SUCCESS = 3         /* CeresIterationCallback time limit (CeresIterationCallback.cpp:30-38) */
} okvisgpu_termination;

/* ---------------------------------------------------------------- problem description */
typedef struct okvisgpu_camera {
  int32_t distortion;               /* okvisgpu_distortion */
  int32_t width, height;
  double fu, fv, cu, cv;            /* PinholeCamera intrinsics (PinholeCamera.hpp:288-366) */
  double dist[8];                   /* radtan: k1 k2 p1 p2 ; equidistant: k1 k2 k3 k4 ;
                                       radtan8: k1 k2 p1 p2 k3 k4 k5 k6 (unused entries 0) */
} okvisgpu_camera;

typedef struct okvisgpu_imu_params { /* okvis::ImuParameters subset, okvis_common/.../Parameters.hpp:89-105 */
  double a_max, g_max;
  double sigma_g_c, sigma_a_c, sigma_gw_c, sigma_aw_c;
  double g;
} okvisgpu_imu_params;

/* ---------------------------------------------------------------- robust losses (ABI 6)
 * The ::ceres::LossFunction family (ceres-solver >= 2.1 loss_function.h; un-vendored submodule,
 * SURVEY.md §8c). okvis builds four losses in ViGraph's constructor (ViGraph.cpp:235-238):
 * CauchyLoss(1.0) for reprojections (:338) and Cauchy-robustified submap alignment (:1505),
 * CauchyLoss(3.0) for GPS (:88,:999,:1408), TukeyLoss(2.0) / TukeyLoss(0.1) for LiDAR / depth submap
 * alignment (:1510,:1513). rho(s) of the squared residual norm s, with rho[1] = rho', rho[2] = rho'':
 *   CAUCHY(a)      b = a^2:  b log(1 + s/b)
 *   TUKEY(a)       s <= a^2: a^2/3 (1 - (1 - s/a^2)^3), else a^2/3
 *   HUBER(a)       s <= a^2: s, else 2 a sqrt(s) - a^2
 *   SOFTLONE(a)    2 a^2 (sqrt(1 + s/a^2) - 1)
 *   ARCTAN(a)      a atan2(s, a)
 *   TOLERANT(a, b) b log(1 + exp((s - a)/b)) - b log(1 + exp(-a/b))
 * The backend applies Ceres' Corrector (restated by okvis at TwoPoseGraphError.cpp:292-337): cost
 * 1/2 rho(s); for rho'' <= 0 (or s = 0) r and J scaled by sqrt(rho'); for rho'' > 0 (TOLERANT) the
 * second-order correction alpha = 1 - sqrt(1 + 2 s rho''/rho'), r scaled by sqrt(rho')/(1 - alpha),
 * J <- sqrt(rho') (I - alpha/s r r^T) J. */
typedef enum okvisgpu_loss_kind {
  OKVISGPU_LOSS_NONE = 0,           /* nullptr loss (TrivialLoss)                                */
  OKVISGPU_LOSS_CAUCHY = 1,
  OKVISGPU_LOSS_TUKEY = 2,
  OKVISGPU_LOSS_HUBER = 3,
  OKVISGPU_LOSS_SOFTLONE = 4,
  OKVISGPU_LOSS_ARCTAN = 5,
  OKVISGPU_LOSS_TOLERANT = 6
} okvisgpu_loss_kind;

typedef struct okvisgpu_loss {
  int32_t kind;                     /* okvisgpu_loss_kind                                        */
  int32_t reserved;                 /* 0                                                          */
  double a, b;                      /* scale a (> 0); b: TOLERANT's width (> 0), else unused      */
} okvisgpu_loss;

/* rho[3] = (rho(s), rho'(s), rho''(s)) of a loss, as ::ceres::LossFunction::Evaluate (host only).
 * OKVISGPU_ERR_INVALID_ARGUMENT for an unknown kind or a non-positive scale. */
int okvisgpu_loss_evaluate(const okvisgpu_loss* loss, double s, double* rho);

/* Size (doubles) of one ImuError's persistent preintegration state (in/out, see imu_state). Layout:
 *  [0]       redo counter (0 => never integrated; first Evaluate integrates, ImuError.cpp:837)
 *  [1]       redo_ flag
 *  [2..5]    Delta_q (x y z w)        [6..14]   C_integral (row-major)
 *  [15..23]  C_doubleintegral         [24..26]  acc_integral
 *  [27..29]  acc_doubleintegral       [30..38]  dalpha_db_g
 *  [39..47]  dv_db_g                  [48..56]  dp_db_g
 *  [57..65]  speedAndBiases_ref_ (9)  [66..290] squareRootInformation_ (15x15 row-major)
 *  [291]     steps integrated by the last redo (informational; -1: the samples did not reach t1,
 *            nothing was integrated and the factor evaluates to r = 0, J = 0, ImuError.cpp:849-853)
 *  [292..300] cross_ (row-major)       [301..525] P_delta_ (15x15, symmetric): what
 *            ImuError::append continues from (ABI 4)                                          */
#define OKVISGPU_IMU_STATE_DOUBLES 526

/* Host-evaluated residual block (ABI 5; SURVEY.md §8b fallback): the contract of
 * ::ceres::CostFunction::Evaluate(parameters, residuals, jacobians) plus the caller's user pointer
 * and the factor's index within its window. parameters[k] holds the ambient values of the factor's
 * k-th parameter block (pose-kind 7, speed/bias 9); residuals[dim]; jacobians[k] the row-major
 * dim x ambient-size Jacobian of block k (always requested: the backend evaluates r and J together
 * at every point it evaluates). The backend applies the pose manifold itself (PoseManifold plus
 * Jacobian, PoseLocalParameterization.cpp:56-68), as Ceres does for a block with a manifold.
 * Return nonzero on success; 0 makes the evaluation fail (a candidate point is then rejected, as
 * Ceres does with candidate_cost = max; a failure at the initial point ends the window's solve with
 * OKVISGPU_FAILURE). Called concurrently from up to options.num_threads host threads.
 * The calls are made from a host node of the context's captured iteration graph (hipLaunchHostFunc):
 * the HIP runtime's callback thread fans them out to the context's persistent worker threads while
 * the context's stream waits. A callback must therefore not call HIP or any okvisgpu_* function (it
 * would wait on the stream it is blocking: deadlock); it may only read its parameters and its own
 * data and write residuals / jacobians. */
typedef int (*okvisgpu_host_evaluate_fn)(void* user, int32_t factor, const double* const* parameters,
                                         double* residuals, double** jacobians);
#define OKVISGPU_HOST_MAX_RESIDUALS 15

typedef struct okvisgpu_problem {
  /* --- parameter blocks (written back in place by okvisgpu_solve / okvisgpu_get_params) */
  int32_t n_poses;
  double* poses;                    /* [n_poses][7] T_WS                                       */
  const uint8_t* pose_constant;     /* [n_poses] 1 = SetParameterBlockConstant (may be NULL)    */
  int32_t n_speed_biases;
  double* speed_biases;             /* [n_speed_biases][9]                                     */
  const uint8_t* speed_bias_constant;
  int32_t n_landmarks;
  double* landmarks;                /* [n_landmarks][4]                                        */
  const uint8_t* landmark_constant;
  int32_t n_cameras;
  const okvisgpu_camera* cameras;   /* [n_cameras]                                             */
  double* extrinsics;               /* [n_cameras][7] T_SC, one block per camera shared by all
                                       states (ViGraph::addStatesPropagate re-uses the block,
                                       ViGraph.cpp:469-473); written back when variable          */

  /* --- ReprojectionError<PinholeCamera<D>> residual blocks (ViGraph.hpp:307-352) */
  int32_t n_observations;
  const int32_t* obs_pose;          /* [n_obs] pose block index                                */
  const int32_t* obs_landmark;      /* [n_obs] landmark block index                            */
  const int32_t* obs_camera;        /* [n_obs] camera / extrinsics index                       */
  const double* obs_keypoint;       /* [n_obs][2] measurement_                                 */
  const double* obs_sqrt_info;      /* [n_obs][4] squareRootInformation_ = LLT(info).L^T, row-major
                                       (ReprojectionError.hpp:49-57; info = 64/size^2 I)         */
  const uint8_t* obs_cauchy;        /* [n_obs] 1 = CauchyLoss(1.0) (ViGraph.cpp:235), NULL = all */

  /* --- ImuError residual blocks (ImuError.cpp:797-1003), parameter order (pose0, sb0, pose1, sb1) */
  int32_t n_imu;
  const int32_t* imu_blocks;        /* [n_imu][4] pose0 sb0 pose1 sb1                           */
  const int64_t* imu_t0_ns;         /* [n_imu]                                                  */
  const int64_t* imu_t1_ns;         /* [n_imu]                                                  */
  const int32_t* imu_sample_begin;  /* [n_imu+1] CSR into the sample arrays                     */
  const int64_t* imu_sample_t_ns;   /* [n_samples] a factor's stamps may come in any order: a step is
                                       integrated from the reference's running `time` (the end of the
                                       last integrated step) and skipped when it does not advance it
                                       (ImuError.cpp:315-328, :439), so a duplicate or a stamp that
                                       steps back gives what ImuError gives. Samples that end before
                                       t1 leave the factor unintegrated (ImuError.cpp:270-273).    */
  const double* imu_sample_gyr_acc; /* [n_samples][6] gyroscopes(3) accelerometers(3)           */
  okvisgpu_imu_params imu_params;
  double* imu_state;                /* [n_imu][OKVISGPU_IMU_STATE_DOUBLES] in/out, NULL = fresh  */

  /* --- PoseError priors (PoseError.cpp:73-125) */
  int32_t n_pose_priors;
  const int32_t* pose_prior_block;  /* [n] pose index                                           */
  const double* pose_prior_meas;    /* [n][7]                                                   */
  const double* pose_prior_sqrt_info; /* [n][36] row-major                                      */

  /* --- SpeedAndBiasError priors (SpeedAndBiasError.cpp:67-101) */
  int32_t n_sb_priors;
  const int32_t* sb_prior_block;
  const double* sb_prior_meas;      /* [n][9]                                                   */
  const double* sb_prior_sqrt_info; /* [n][81] row-major                                        */

  /* --- TwoPoseStandardGraphError / TwoPoseStandardGraphErrorConst residual blocks: relative-pose
   * (pose-graph) edges that marginalisation leaves between two keyframes of the window
   * (TwoPoseGraphError.cpp:467-606 and :631-767; added without a loss function at
   * ViGraphEstimator.cpp:770). Parameter order (reference pose, other pose). The edge is the output
   * of TwoPoseStandardGraphError::compute (okvisgpu_twopose_compute below). */
  int32_t n_relpose;
  const int32_t* relpose_blocks;    /* [n][2] reference pose, other pose                        */
  const double* relpose_delta_x;    /* [n][6] DeltaX_                                           */
  const double* relpose_sqrt_info;  /* [n][36] J_ row-major (information = J_^T J_)             */
  const double* relpose_lin_point;  /* [n][7] linearisationPoint_T_S0S1_                        */
  /* [n] residual kind (may be NULL = all 0):
   *   0 TwoPoseStandardGraphError(Const): r = J_ (DeltaX_ + [r_S0S1 - r_lin; 2 vec(q_S0S1 q_lin^-1)])
   *   1 RelativePoseError (RelativePoseError.cpp:59-140, added by ViGraph::addRelativePoseConstraint,
   *     ViGraph.cpp:786-808, no loss): relpose_lin_point = the measured T_AB, relpose_sqrt_info =
   *     LLT(information).L^T, relpose_delta_x unused;
   *     r = L [r_AB_meas - r_AB; 2 vec(q_AB_meas q_AB^-1)], T_AB = T_WA^-1 T_WB                 */
  const uint8_t* relpose_kind;

  /* --- ABI 4: variable extrinsics (online calibration, do_extrinsics: true; ViGraph.cpp:330-386)
   * extrinsics_constant [n_cameras]: 0 = the camera's T_SC block is variable (NULL = all constant,
   * do_extrinsics: false). Its PoseError prior, PoseError(T_SC, sigma_r^2, sigma_alpha^2)
   * (ViGraph.cpp:372-382, PoseError.cpp:73-125), comes through the extrinsics_prior_* arrays. */
  const uint8_t* extrinsics_constant;
  int32_t n_extrinsics_priors;
  const int32_t* extrinsics_prior_camera; /* [n] camera index                                   */
  const double* extrinsics_prior_meas;    /* [n][7]                                             */
  const double* extrinsics_prior_sqrt_info; /* [n][36] row-major                                */

  /* --- ABI 5: residual blocks evaluated on the host (SURVEY.md §8b "host-evaluated fallback"):
   * any residual the GPU path has no functor for (GpsErrorSynchronous/Asynchronous,
   * GpsErrorAsynchronous.hpp:42-55; RelativePoseError-like user factors) whose parameter blocks are
   * pose-kind or speed/bias blocks: at most 2 pose-kind and 2 speed/bias blocks, all distinct, at most
   * OKVISGPU_HOST_MAX_RESIDUALS residuals. Each point the solver evaluates (initial point, every
   * candidate) gathers the blocks' values on the device, calls host_evaluate on options.num_threads
   * host threads, and uploads r and the minimal Jacobian, which are accumulated into the reduced
   * system like any device-evaluated factor. Factors on landmarks are not supported
   * (OKVISGPU_ERR_UNSUPPORTED). n_host = 0 (the zero-initialised struct) = none. */
  int32_t n_host;
  const int32_t* host_dim;          /* [n] residual dimension, 1..OKVISGPU_HOST_MAX_RESIDUALS     */
  const int32_t* host_param_kind;   /* [n][4] parameter block k in the functor's order: 0 pose-kind
                                       (index < n_poses: a state's pose; n_poses + c: camera c's
                                       extrinsics), 1 speed/bias, -1 none (trailing)             */
  const int32_t* host_param_index;  /* [n][4]                                                      */
  const uint8_t* host_cauchy;       /* [n] 1 = CauchyLoss(1.0) (may be NULL = no loss); ignored
                                       when host_loss is set                                    */
  okvisgpu_host_evaluate_fn host_evaluate;
  void* host_user;

  /* --- ABI 6: the loss function of each host-evaluated factor (any okvisgpu_loss_kind, e.g.
   * CauchyLoss(3.0) on GPS factors, ViGraph.cpp:999; TukeyLoss(2.0) on LiDAR submap alignment,
   * :1510). NULL = host_cauchy. */
  const okvisgpu_loss* host_loss;   /* [n_host]                                                     */
} okvisgpu_problem;

/* ---------------------------------------------------------------- solver options / summary */
typedef struct okvisgpu_options {   /* ::ceres::Solver::Options fields okvis sets or relies on */
  int32_t max_num_iterations;       /* ViGraph.cpp:1856                                         */
  int32_t linear_solver;            /* okvisgpu_linear_solver                                   */
  int32_t trust_region_strategy;    /* okvisgpu_tr_strategy                                     */
  int32_t jacobi_scaling;           /* Ceres default true                                       */
  double function_tolerance;        /* 1e-6 default; 1e-3 for the first full-graph pass          */
  double gradient_tolerance;        /* 1e-10                                                    */
  double parameter_tolerance;       /* 1e-8                                                     */
  double initial_trust_region_radius; /* 1e4                                                    */
  double max_trust_region_radius;   /* 1e16                                                     */
  double min_trust_region_radius;   /* 1e-32                                                    */
  double min_relative_decrease;     /* 1e-3                                                     */
  double min_lm_diagonal;           /* 1e-6                                                     */
  double max_lm_diagonal;           /* 1e32                                                     */
  int32_t max_num_consecutive_invalid_steps; /* 5                                               */
  double time_limit_s;              /* <0: none (ViGraph::setOptimisationTimeLimit)              */
  int32_t min_iterations;           /* CeresIterationCallback iterationMinimum_                  */
  int32_t redo_propagation_always;  /* ImuError::redoPropagationAlways (ViSlamBackend.cpp:2036)  */
  int32_t num_threads;              /* host threads (reference path / host evaluation)          */
  int32_t verbose;
  int32_t cholesky_schedule;        /* 0 auto, 1 one persistent workgroup per window (batches of */
                                    /* more windows than CUs), 2 tile-parallel launches (fewer    */
                                    /* than half as many), 3 persistent, split over the two parts */
                                    /* of a nested-dissection window (half as many), 4 pipelined  */
                                    /* persistent, two teams per window (up to one per CU), 5 the */
                                    /* split schedule with each part pipelined; all give the same */
                                    /* bits for one batch. Other values: auto.                    */
} okvisgpu_options;

typedef struct okvisgpu_summary {   /* ::ceres::Solver::Summary subset */
  double initial_cost;
  double final_cost;
  int32_t num_iterations;           /* iterations performed, excluding iteration 0              */
  int32_t num_successful_steps;     /* Ceres counts iteration 0 as successful                    */
  int32_t num_unsuccessful_steps;
  int32_t termination_type;         /* okvisgpu_termination                                     */
  double total_time_s;              /* wall time of okvisgpu_solve for this batch               */
  double final_radius;
  double final_mu;
  /* ABI 6: the ::ceres::Solver::Summary timing fields (seconds; one batch, the same in every
   * window's summary). Wall clock of okvisgpu_solve's parts: preprocessor (parameter upload,
   * structure rebuild after freeze / unfreeze, iteration 0, graph instantiation), minimizer (the
   * trust-region iterations), postprocessor (write-back). Device time of the iterations' phases
   * from HIP events on the context's stream, only when options.verbose is set (the iterations then
   * run as eager launches instead of the captured graph: the same kernels in the same order, the
   * same bits), else -1: linear solver (GN prep, Schur assembly, LLT + back substitution, J*v),
   * residual evaluation (candidate evaluation and its cost reduction), Jacobian evaluation
   * (linearisation at the accepted point and the gradient norms), step (the dogleg step, Plus and
   * the accept / reject decision; no Ceres field: part of its minimizer time). */
  double preprocessor_time_s;
  double minimizer_time_s;
  double postprocessor_time_s;
  double linear_solver_time_s;
  double residual_evaluation_time_s;
  double jacobian_evaluation_time_s;
  double step_time_s;
} okvisgpu_summary;

/* ---------------------------------------------------------------- context */
typedef struct okvisgpu_ctx okvisgpu_ctx;

int okvisgpu_abi_version(void);
void okvisgpu_default_options(okvisgpu_options* options);
int okvisgpu_device_count(int32_t* count);
int okvisgpu_ctx_create(int32_t device, okvisgpu_ctx** ctx);
int okvisgpu_ctx_destroy(okvisgpu_ctx* ctx);
const char* okvisgpu_last_error(const okvisgpu_ctx* ctx);

/* Upload a batch of independent windows (one window = one okvis::ViGraph problem). The structure
 * (residual blocks, parameter blocks, constant flags) is analysed once here. The problem structs
 * and the arrays they point to must stay valid until the next okvisgpu_set_problems() call,
 * because okvisgpu_solve() writes results back into them. */
int okvisgpu_set_problems(okvisgpu_ctx* ctx, const okvisgpu_problem* problems, int32_t n_windows);

/* Re-upload only parameter values (and imu_state) from the host arrays (after the caller changed
 * estimates between solves, e.g. ViSlamBackend re-initialising states). */
int okvisgpu_update_params(okvisgpu_ctx* ctx);

/* SetParameterBlockConstant / SetParameterBlockVariable between solves (freeze / unfreeze:
 * ViGraphEstimator.cpp:216-331; extrinsics: ViGraph::setExtrinsicsVariable, ViGraph.cpp:1733-1739,
 * and the tracking solve's freeze, ViSlamBackend.cpp:866-872). kind: 0 pose, 1 speed/bias,
 * 2 landmark, 3 extrinsics (index = camera). Takes effect at the next
 * okvisgpu_solve (the reduced-system structure is rebuilt on the host, values stay on device). */
int okvisgpu_set_block_constant(okvisgpu_ctx* ctx, int32_t window, int32_t kind, int32_t index,
                                int32_t is_constant);

/* ::ceres::Solve equivalent for every window in the batch. summaries: NULL or an array of n_windows
 * entries (n_windows of the last okvisgpu_set_problems: one summary is written for EVERY window).
 * Results are written back into the caller's parameter arrays (and imu_state when provided). */
int okvisgpu_solve(okvisgpu_ctx* ctx, const okvisgpu_options* options, okvisgpu_summary* summaries);

/* Split form of okvisgpu_solve (okvisgpu_solve == begin + iterate(max_num_iterations) + end):
 *   begin   upload the caller's parameter values, iteration 0 (initial evaluation, Jacobi scaling,
 *           gradient norms) and instantiate the captured iteration graph;
 *   iterate enqueue n trust-region iterations on the context's stream (asynchronous; windows that
 *           have terminated skip all work);
 *   end     synchronise, finish windows that spent iterations on LM-regularisation retries, write
 *           results back into the caller's arrays and fill the summaries.
 * okvisgpu_synchronize waits for the context's stream. */
int okvisgpu_solve_begin(okvisgpu_ctx* ctx, const okvisgpu_options* options);
int okvisgpu_solve_iterate(okvisgpu_ctx* ctx, int32_t n);
int okvisgpu_solve_end(okvisgpu_ctx* ctx, okvisgpu_summary* summaries);
int okvisgpu_synchronize(okvisgpu_ctx* ctx);

/* Device time per kernel of ONE trust-region iteration launched eagerly (not from the graph) on
 * the context's stream, bracketed by HIP events; must follow okvisgpu_solve_begin (it advances the
 * solve by one iteration). phase_ms[OKVISGPU_N_PHASES] (ms, summed over the launches of that
 * kernel in the iteration); phase i is named by okvisgpu_phase_name(i). */
#define OKVISGPU_N_PHASES 15
int okvisgpu_profile_iteration(okvisgpu_ctx* ctx, double* phase_ms);
const char* okvisgpu_phase_name(int32_t phase);

/* Measurement hooks (not part of the reference interface; used by bench.py's roofline).
 * okvisgpu_time_kernel re-arms every window of the last finished solve (call after
 * okvisgpu_solve_end / okvisgpu_solve; the device-side solve and IMU state are scratch afterwards:
 * call okvisgpu_update_params before the next solve) and launches one
 * iteration's worth of kernel `kernel` `reps` times on the context's stream between HIP events.
 * avg_ms = device time per repetition; work = algorithmic work of one repetition over the whole
 * batch (compulsory HBM bytes if *bound == 0, FP64 FLOPs if *bound == 1). */
int okvisgpu_kernel_count(void);
const char* okvisgpu_kernel_name(int32_t kernel);
int okvisgpu_time_kernel(okvisgpu_ctx* ctx, int32_t kernel, int32_t reps, double* avg_ms, double* work,
                         int32_t* bound);

/* ---------------------------------------------------------------- pose-graph edges
 * TwoPoseStandardGraphError::compute (TwoPoseGraphError.cpp:162-397) for a batch of edges on the
 * GPU: the reprojection observations of the landmarks shared by a reference keyframe S0 and another
 * keyframe S1 are linearised in S0 coordinates (Cauchy-corrected, |r| > 3 outliers dropped), every
 * landmark is marginalised with the pseudo-inverse square root of its 3x3 block (dropped when
 * rank < 3 and its depth in S0 < 2.99), and the 6x6 relative system H00_, b0_ is decomposed into
 * J_ = D^(1/2) E^T and DeltaX_ = -H^+ b0_ (eigenvalues <= 1e-8*6*max treated as zero, ascending
 * order as Eigen::SelfAdjointEigenSolver). Inputs are the values TwoPoseGraphError::addObservation
 * recorded: landmarks and the other pose as added, the reference pose as its current estimate.
 * The edges of one call share the camera rig (stayConst_ = true, do_extrinsics: false). */
typedef struct okvisgpu_twopose_edges {
  int32_t n_edges;
  const double* ref_pose;           /* [n_edges][7] T_WS0                                        */
  const double* other_pose;         /* [n_edges][7] T_WS1                                        */
  int32_t n_cameras;
  const okvisgpu_camera* cameras;   /* [n_cameras]                                               */
  const double* extrinsics;         /* [n_cameras][7] T_SC                                       */
  const int32_t* landmark_begin;    /* [n_edges+1] CSR: landmarks of edge e (observations_ map order) */
  const double* landmarks;          /* [n_landmarks][4] hp_W                                     */
  const int32_t* obs_begin;         /* [n_landmarks+1] CSR: observations of landmark l           */
  const uint8_t* obs_other;         /* [n_obs] 0 = seen from the reference pose, 1 = from the other */
  const int32_t* obs_camera;        /* [n_obs]                                                   */
  const double* obs_keypoint;       /* [n_obs][2]                                                */
  const double* obs_sqrt_info;      /* [n_obs][4] (ReprojectionError::setInformation; weight applied) */
  const uint8_t* obs_cauchy;        /* [n_obs] 1 = CauchyLoss(1) (may be NULL = all)             */
} okvisgpu_twopose_edges;

/* Outputs per edge (host, caller-owned): delta_x [6], sqrt_info (J_) [36], lin_point [7];
 * H00 [36] and b0 [6] (the marginalised relative system, may be NULL). Uses the context's device and
 * stream; independent of the problem set with okvisgpu_set_problems. */
int okvisgpu_twopose_compute(okvisgpu_ctx* ctx, const okvisgpu_twopose_edges* edges, double* delta_x,
                             double* sqrt_info, double* lin_point, double* H00, double* b0);

/* ---------------------------------------------------------------- calibrating pose-graph edges
 * (An addition to ABI 6: two new entry points and a new struct; OKVISGPU_ABI_VERSION stays 6.)
 * TwoPoseExtrinsicsGraphError (TwoPoseExtrinsicsGraphError.cpp), the edge
 * ViGraphEstimator::convertToPoseGraphMst creates instead of the standard one with
 * do_extrinsics: true (ViGraphEstimator.cpp:419-427, 562-571): D = 6 + 6 n_cameras residuals over
 * the relative pose and the cameras' T_SC blocks, camera c in rows and columns 6 + 6 c .. 11 + 6 c
 * (stayConst_ = true, the only layout the reference constructs).
 *
 * okvisgpu_twopose_extrinsics_compute is ::compute (:73-330) for a batch of edges, on the inputs of
 * okvisgpu_twopose_compute; `extrinsics` are the current estimates of the T_SC blocks and become the
 * linearisation points of the cameras the edge observes. Per observation the residual and the
 * minimal Jacobians w.r.t. pose (other keyframe only), landmark and the camera's extrinsics; |r| > 3
 * dropped, Cauchy corrector where obs_cauchy is set; every landmark marginalised with
 * PseudoInverse::symmSqrt(V, 1e-7) and left out entirely when rank < 3 and its S0 depth < 2.99; then
 * J_ = D^(1/2) E^T (rows in ascending eigenvalue order, zero rows for eigenvalues <= 1e-8 D max) and
 * DeltaX_ = -E D^-1 E^T b0_. Outputs per edge (host, caller-owned): delta_x [D], sqrt_info (J_)
 * [D*D] row-major, lin_point [7] (T_S0S1 once the edge has any observation from the other keyframe,
 * else the identity), camera_seen [n_cameras] (1 once the edge has any observation of camera c,
 * dropped or not: the reference would have set linearisationPoints_T_SC_[c]); H00 [D*D] and b0 [D]
 * may be NULL. An unseen camera's rows and columns of H00, its columns of sqrt_info (the rows of J_
 * belong to eigenvalues; the camera's six zero ones head the ascending list as zero rows) and its b0
 * and delta_x entries are exactly 0. An edge's result does not depend on the batch it is in, and is the same bits on every
 * run. n_edges = 0 and edges without landmarks are valid (all zeros, identity lin_point). Argument
 * checks as okvisgpu_twopose_compute; n_cameras > OKVISGPU_TWOPOSE_MAX_CAMERAS returns
 * OKVISGPU_ERR_UNSUPPORTED before anything is launched or written. */
#define OKVISGPU_TWOPOSE_MAX_CAMERAS 6
int okvisgpu_twopose_extrinsics_compute(okvisgpu_ctx* ctx, const okvisgpu_twopose_edges* edges, double* delta_x,
                                        double* sqrt_info, double* lin_point, uint8_t* camera_seen, double* H00,
                                        double* b0);

/* TwoPoseExtrinsicsGraphError(Const)::EvaluateWithMinimalJacobians (:393-610, :680-860) for a batch
 * of computed edges at given parameter values: error = DeltaX_ + [r_S0S1 - r_lin; 2 vec(q_S0S1
 * q_lin^-1); per seen camera r_SC - r_SC,lin; 2 vec(q_SC q_SC,lin^-1)], r = J_ error. Independent of
 * the problem set with okvisgpu_set_problems. */
typedef struct okvisgpu_twopose_extrinsics_eval {
  int32_t n_edges;
  int32_t n_cameras;
  const double* ref_pose;           /* [n_edges][7] T_WS0                                         */
  const double* other_pose;         /* [n_edges][7] T_WS1                                         */
  const double* extrinsics;         /* [n_cameras][7] current T_SC (shared by the edges)          */
  const double* delta_x;            /* [n_edges][D]                                               */
  const double* sqrt_info;          /* [n_edges][D*D] J_ row-major                                */
  const double* lin_point;          /* [n_edges][7] linearisationPoint_T_S0S1_                    */
  const double* lin_extrinsics;     /* [n_edges][n_cameras][7] linearisationPoints_T_SC_ (read where seen) */
  const uint8_t* camera_seen;       /* [n_edges][n_cameras]                                       */
} okvisgpu_twopose_extrinsics_eval;
/* Outputs (host, caller-owned, any may be NULL): r [n][D]; minimal Jacobians, row-major: J_ref
 * [n][D][6], J_other [n][D][6], J_extrinsics [n][n_cameras][D][6] (zero for an unseen camera). */
int okvisgpu_twopose_extrinsics_evaluate(okvisgpu_ctx* ctx, const okvisgpu_twopose_extrinsics_eval* edges, double* r,
                                         double* J_ref, double* J_other, double* J_extrinsics);

/* ---------------------------------------------------------------- IMU-merge elimination
 * ImuError::append (ImuError.cpp:63-255) for a batch of factors on the GPU: the step of
 * ViGraphEstimator::eliminateStateByImuMerge (ViGraphEstimator.cpp:38-171) that extends the IMU
 * link into an eliminated state k with the link out of it. Per factor: `state` is the link's
 * preintegration state (OKVISGPU_IMU_STATE_DOUBLES layout, e.g. written back by a solve), t1_old its
 * t1, t1_new the next link's t1, speed_biases the estimate of state k (the bias the appended part
 * is integrated with), and the samples the next link's imuMeasurements(). On return `state` holds the
 * merged link's state (t0 unchanged, t1 = t1_new; redo counter, redo flag and speedAndBiases_ref_
 * unchanged, as in the reference) and steps[i] the integrated steps (-1: the samples do not reach
 * t1_new, state untouched). The merged factor's samples are the link's followed by the appended ones
 * newer than its last (ImuError.cpp:74-81); the caller rebuilds its problem with them. */
typedef struct okvisgpu_imu_append_batch {
  int32_t n;
  okvisgpu_imu_params imu_params;
  double* state;                    /* [n][OKVISGPU_IMU_STATE_DOUBLES] in/out                     */
  const int64_t* t1_old_ns;         /* [n]                                                         */
  const int64_t* t1_new_ns;         /* [n]                                                         */
  const double* speed_biases;       /* [n][9]                                                      */
  const int32_t* sample_begin;      /* [n+1] CSR of the appended samples                           */
  const int64_t* sample_t_ns;       /* [n_samples]                                                 */
  const double* sample_gyr_acc;     /* [n_samples][6]                                              */
} okvisgpu_imu_append_batch;
int okvisgpu_imu_append(okvisgpu_ctx* ctx, const okvisgpu_imu_append_batch* batch, int32_t* steps);

/* ---------------------------------------------------------------- IMU propagation
 * (An addition to ABI 6: a new entry point and a new struct; OKVISGPU_ABI_VERSION stays 6.)
 * The static ImuError::propagation (ImuError.cpp:537-759) for a batch of independent items on the
 * GPU: what ViGraph::addStatesPropagate (ViGraph.cpp:400-417) and ThreadedSlam::processFrame
 * (ThreadedSlam.cpp:613-627) call for the new state's pose and speed, and Frontend::propagation
 * (Frontend.cpp:1146-1162) with the 15x15 covariance and Jacobian. Per item i: poses[i] (T_WS as
 * [r, q xyzw]) and speed_biases[i] at t_start are replaced by the propagated pose and speed at t_end
 * (the biases are unchanged), integrating the item's samples with the trapezoid chain of :644-668
 * and the stepping rules of :584-617 and :716-721 (interpolation at both ends, steps with dt <= 0
 * skipped, dt from integer nanosecond differences). covariance / jacobian (each may be NULL) receive
 * P = T P_delta T^T (:748-757; per-step noise with the saturation factors of :619-640 and :688-707)
 * and F (:735-746) in the error-state order [r, alpha, v, b_g, b_a], row-major. steps[i] (steps may
 * be NULL) is the number of integrated steps, or -1 when the item's last sample is older than t_end
 * (:552-553): then nothing of the item is written, covariance and Jacobian rows included. With 0
 * steps (t_end <= t_start) the pose and speed/bias keep their bits, the Jacobian is the identity
 * and the covariance zero. An item without samples, or whose first sample is newer than t_start
 * (the reference's assertion at :550), makes the whole call return OKVISGPU_ERR_INVALID_ARGUMENT
 * before anything is launched or written; okvisgpu_last_error names the item. Also refused between
 * okvisgpu_solve_begin and _solve_end. Uses the context's device and stream and returns with the
 * results in the caller's arrays; independent of the problem set with okvisgpu_set_problems (needs
 * none, leaves the device parameter sets alone). An item's result does not depend on the batch. */
typedef struct okvisgpu_imu_propagate_batch {
  int32_t n;
  okvisgpu_imu_params imu_params;
  double* poses;                    /* [n][7] T_WS, in/out                                         */
  double* speed_biases;             /* [n][9] in/out (only v changes)                              */
  const int64_t* t_start_ns;        /* [n]                                                         */
  const int64_t* t_end_ns;          /* [n]                                                         */
  const int32_t* sample_begin;      /* [n+1] CSR into the sample arrays                            */
  const int64_t* sample_t_ns;       /* [n_samples]                                                 */
  const double*  sample_gyr_acc;    /* [n_samples][6]                                              */
  double* covariance;               /* [n][225] row-major, out, may be NULL                        */
  double* jacobian;                 /* [n][225] row-major, out, may be NULL                        */
} okvisgpu_imu_propagate_batch;
int okvisgpu_imu_propagate(okvisgpu_ctx* ctx, const okvisgpu_imu_propagate_batch* batch, int32_t* steps);

/* ---------------------------------------------------------------- GNSS factors
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * The factor ViGraph::addGpsMeasurement (ViGraph.cpp:973-1006) adds for every GPS fix, evaluated for a
 * batch of independent factors on the GPU at given parameter values: kind 0 is
 * GpsErrorAsynchronous::EvaluateWithMinimalJacobians (GpsErrorAsynchronous.cpp:98-300) with its own IMU
 * pre-integration from the state's stamp t_k to the fix's stamp t_g (redoPreintegration, :303-507), kind 1
 * GpsErrorSynchronous (GpsErrorSynchronous.cpp:41-144). Parameters per factor: poses[i] = T_WS at t_k
 * ([r, q xyzw]), speed_biases[i], and T_GW[gw_index[i]] (gw_index NULL: block 0 for every factor, so that
 * one call serves the realtime and the full graph); the antenna offset r_SA (gpsParameters_.r_SA) is the
 * call's. `information` is the constructor's argument, the fix's inverse covariance.
 *
 * Kind 0, per factor, on its `state` (layout below; state NULL: every factor is fresh and nothing is kept):
 *   Redo decision (:134-142): Delta_b = speed_bias[3:9] - ref[3:9]; redo = flag || |Delta_b_g| > 0.0003;
 *   the factor re-integrates if redo_propagation_always || (redo && n_samples < 50) || counter == 0. After
 *   a redo the counter is incremented, Delta_b = 0, the flag is 0 and ref is the current speed/biases;
 *   without one the flag keeps `redo` and nothing else of the state changes.
 *   Redo chain (:303-507): the stepping rules of :341-375 and :480-483 (interpolation at both ends, steps
 *   with dt <= 0 skipped, dt from integer nanosecond differences through Duration::toSec), the saturation
 *   factors of :378-398 (100 for a step with a gyro resp. accelerometer component above g_max resp.
 *   a_max), the trapezoid chain and the bias Jacobians of :402-432 (dalpha_db_g with the right Jacobian),
 *   and with use_imu_covariance the recursion X <- F_delta X F_delta^T + K (:437-467), the symmetrisation
 *   and the sigma-weighted sum P_delta (:494-500); without it P_delta stays zero (:331).
 *   Then (:145-166) T_WS(t_g) = (r + v Dt - g_W Dt^2 / 2 + C_WS (acc_doubleintegral + dp_db_g Delta_b_g -
 *   C_doubleintegral Delta_b_a), normalised(q Delta_q deltaQ(-dalpha_db_g Delta_b_g))) with Dt = t_g - t_k,
 *   g_W = (0, 0, g) and C_WS from the normalised q, and Jprop as at :156-166. With use_imu_covariance
 *   (:173-187) P = T P_delta T^T, Jws = [C_GW, -C_GW [C_WS r_SA]x], covOverall = information^-1 + Jws P_66
 *   Jws^T and sqrt_info = LLT(covOverall^-1).L^T; without (:192-193) sqrt_info = LLT((information^-1)^-1).L^T.
 *   error = z - (C_GW (r_tg + C_tg r_SA) + r_GW), r = sqrt_info error, and the Jacobians exactly as
 *   :213-294: sqrt_info is not differentiated. C_GW is toRotationMatrix of T_GW's quaternion as stored.
 * Kind 1 (GpsErrorSynchronous.cpp:41-144): sqrt_info = LLT(information).L^T, error = z - (C_GW (r + C_WS r_SA)
 * + r_GW) with both rotation matrices from the quaternions as stored; speed_biases, the stamps, the samples,
 * state and the two flags are ignored, J_speed_bias is zero and steps 0.
 *
 * Deviations: (1) the four dPdsigma_ matrices are carried as their sigma-weighted sum (the
 * recursion and the symmetrisation are linear, and the reference reads dPdsigma_ nowhere else). (2) A factor
 * whose samples do not reach t_g (the reference then evaluates uninitialised members: :137-141 ignores the
 * -1), whose first sample is newer than t_k (the assertion at :311), or with t_g < t_k is an argument error;
 * these are the assertions of ViGraph.cpp:976-982. (3) With t_g == t_k the reference's loop reads (it + 1)
 * past the end and uses nothing of it; here the result is 0 steps, identity increments and P_delta = 0.
 *
 * State, OKVISGPU_GPS_STATE_DOUBLES per factor: [0..65] as OKVISGPU_IMU_STATE_DOUBLES (redo counter, redo
 * flag, Delta_q, C_integral, C_doubleintegral, acc_integral, acc_doubleintegral, dalpha_db_g, dv_db_g,
 * dp_db_g, speedAndBiases_ref_), [66] the steps of the last redo, [67..291] P_delta_ (15x15 row-major).
 * cross_ is not kept: nothing reads it after a redo, because this functor has no append.
 *
 * OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a NULL ctx, batch or result, a
 * missing array, a negative count, n_gw < 1, a gw_index outside [0, n_gw), an unknown kind, an `information`
 * that is not finite, symmetric (to 1e-12 of its largest entry) and positive definite (a 3x3 Cholesky on
 * the host), for kind 0 a sample_begin not starting at 0 or not monotone and the cases of deviation 2, and
 * between okvisgpu_solve_begin and _solve_end; okvisgpu_last_error names the factor. n = 0 is valid.
 * Independent of the problem set with okvisgpu_set_problems (needs none, leaves the device parameter sets
 * alone); uses the context's device and stream and returns with the results in the caller's arrays. A
 * factor's result does not depend on the rest of the batch and is the same bits on every run. */
#define OKVISGPU_GPS_STATE_DOUBLES 292
typedef struct okvisgpu_gps_batch {
  int32_t n;
  int32_t kind;                     /* 0 GpsErrorAsynchronous, 1 GpsErrorSynchronous               */
  int32_t use_imu_covariance;       /* the reference's static useImuCovariance (default true)      */
  int32_t redo_propagation_always;  /* the reference's static redoPropagationAlways                */
  okvisgpu_imu_params imu_params;
  double r_SA[3];                   /* gpsParameters_.r_SA                                         */
  const double* poses;              /* [n][7] T_WS at t_k                                          */
  const double* speed_biases;       /* [n][9]                                                      */
  int32_t n_gw;
  const double* T_GW;               /* [n_gw][7]                                                   */
  const int32_t* gw_index;          /* [n] or NULL = block 0                                       */
  const double* measurement;        /* [n][3]                                                      */
  const double* information;        /* [n][9] row-major                                            */
  const int64_t* t_k_ns;            /* [n]                                                         */
  const int64_t* t_g_ns;            /* [n]                                                         */
  const int32_t* sample_begin;      /* [n+1] CSR into the sample arrays                            */
  const int64_t* sample_t_ns;       /* [n_samples]                                                 */
  const double* sample_gyr_acc;     /* [n_samples][6]                                              */
  double* state;                    /* [n][OKVISGPU_GPS_STATE_DOUBLES] in/out, NULL = fresh        */
} okvisgpu_gps_batch;

typedef struct okvisgpu_gps_result {  /* caller-owned, any may be NULL; Jacobians row-major */
  double* r;                        /* [n][3]                                                      */
  double* error;                    /* [n][3] the unweighted error, error()                        */
  double* sqrt_info;                /* [n][9]                                                      */
  double* J_pose;                   /* [n][3][6] jacobiansMinimal[0]                               */
  double* J_speed_bias;             /* [n][3][9] jacobiansMinimal[1]                               */
  double* J_T_GW;                   /* [n][3][6] jacobiansMinimal[2]                               */
  double* J_pose_ambient;           /* [n][3][7] minimal x PoseManifold::minusJacobian: jacobians[0] */
  double* J_T_GW_ambient;           /* [n][3][7] jacobians[2]                                      */
  int32_t* steps;                   /* [n] integrated steps of this call's redo, else the stored value */
} okvisgpu_gps_result;
int okvisgpu_gps_evaluate(okvisgpu_ctx* ctx, const okvisgpu_gps_batch* batch, okvisgpu_gps_result* result);

/* ---------------------------------------------------------------- LiDAR motion undistortion
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * LidarMotionUndistortion::deskew (okvis_mapping/src/LidarMotionUndistortion.cpp:27-85; timer "8.1 Live
 * undistortion" of ThreadedSlam.cpp:785-818) for a batch of independent scans on the GPU, with the
 * BatchedLidarPropagator behind it (okvis_common/src/ViInterface.cpp:635-798); the per-query pose,
 * speed and omega_S are also what Trajectory::getStates (ViInterface.cpp:233-348) asks of the same
 * propagator for the submapping thread (SubmappingInterface.cpp:1255-1268).
 *
 * A scan is a state (pose0 = T_WS, speed_bias0) at t_start, the IMU samples around it, and queries: the
 * stamps of its LiDAR points in non-decreasing order, each with its ray in the LiDAR frame. Per query
 * the state is propagated from t_start to the query's stamp T and the ray is moved into the live sensor
 * frame: point = (T_live^-1 T_WS(T) T_SL [ray; 1]) (:79-81), in double (point_f64) and cast to float
 * (point). The reference's serial loop is restated per query; that is exact because deskew and
 * getStates never change T_WS_0 / speedAndBias_0 and re-set the propagator's reference biases to the
 * same values on every appendTo, so Delta_b = 0 and every bias-Jacobian term is multiplied by zero.
 *   step(k, tau, T), ts[k] < T <= ts[k+1], tau < T (:660-715): with (w0, a0) and (w1, a1) the samples k
 *   and k+1: if T < ts[k+1], dt = T - tau, r = dt / (ts[k+1] - ts[k]) and (w1, a1) <- (1-r)(w0, a0) +
 *   r (w1, a1) (dt from tau, as written at :674-681), else dt = ts[k+1] - tau; then r' = dt / (T - ts[k])
 *   and (w0, a0) <- r' (w0, a0) + (1-r') (w1, a1) (:686-691; exact when tau = ts[k]); then the trapezoid
 *   chain of :696-715 on Delta_q, acc_integral and acc_doubleintegral with omega_S_true = (w0+w1)/2 -
 *   b_g. All time differences go through Duration::toSec of the integer nanosecond difference.
 *   The committed chain starts at the identity with tau = t_start; for k = 0..N-2, if ts[k+1] > tau the
 *   state after interval k is step(k, tau, ts[k+1]) and tau = ts[k+1], else the interval is skipped
 *   (:683-685). It depends on the scan's samples, t_start and biases only.
 *   Query T < t_start: valid = 0, every output of the query zero (deskew skips the point, :61); such
 *   queries are counted in n_before. T = t_start: valid = 1, pose and speed are the input bits, omega_S
 *   = 0. T beyond the scan's last sample: valid = 0, zeros (appendTo returns false, :653). Otherwise
 *   valid = 1: with k the largest index with ts[k] < T, step(k, max(t_start, ts[k]), T) from the
 *   committed state before interval k, then getState (:762-798): Dt = T - t_start, r = r0 + v0 Dt -
 *   g_W Dt^2 / 2 + C_WS0 acc_doubleintegral, q = normalised(q0 Delta_q), v = v0 - g_W Dt + C_WS0
 *   acc_integral, omega_S = omega_S_true, with g_W = (0, 0, g) and C_WS0 from the normalised q0. The
 *   reference hard-codes g = 9.81 (:768).
 * Deviation: a query at exactly t_start that is not the scan's first point. The reference
 * takes the state itself only for the first point (:52-57); for a later point at t_start its sample loop
 * finds no step with dt > 0, runs off the end of the IMU deque and leaves the propagator unusable for
 * the rest of the scan. Here every query at t_start is the state itself.
 *
 * ray, pose_live and T_SL may be NULL when result->point and ->point_f64 are NULL (the getStates use).
 * Every output may be NULL. n_scans = 0 and scans without queries are valid. Independent of the problem
 * set with okvisgpu_set_problems (needs none, leaves the device parameter sets alone); uses the
 * context's device and stream and returns with the results in the caller's arrays. A scan's result does
 * not depend on the rest of the batch and is the same bits on every run.
 * OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a NULL ctx, batch or
 * result, a missing array, a negative count, a CSR not starting at 0 or not monotone, a scan with
 * queries but fewer than two samples, a first sample newer than t_start (the assertion at
 * LidarMotionUndistortion.cpp:34), sample or query stamps of a scan that decrease (the reference's
 * iterator cannot go back), a non-finite g, and between okvisgpu_solve_begin and _solve_end;
 * okvisgpu_last_error names the scan and the query or sample. */
typedef struct okvisgpu_lidar_deskew_batch {
  int32_t n_scans;
  double g;                         /* the reference: 9.81                                         */
  const double* pose0;              /* [n_scans][7] T_WS at t_start                                */
  const double* speed_bias0;        /* [n_scans][9]                                                */
  const int64_t* t_start_ns;        /* [n_scans]                                                   */
  const int32_t* sample_begin;      /* [n_scans+1] CSR into the sample arrays                      */
  const int64_t* sample_t_ns;       /* [n_samples]                                                 */
  const double* sample_gyr_acc;     /* [n_samples][6]                                              */
  const int32_t* query_begin;       /* [n_scans+1] CSR into the query arrays                       */
  const int64_t* query_t_ns;        /* [n_queries] non-decreasing within a scan                    */
  const double* ray;                /* [n_queries][3] rayMeasurement, LiDAR frame; see above       */
  const double* pose_live;          /* [n_scans][7] T_WS of the live frame; see above              */
  const double* T_SL;               /* [n_scans][7]; see above                                     */
} okvisgpu_lidar_deskew_batch;

typedef struct okvisgpu_lidar_deskew_result {  /* caller-owned, any may be NULL */
  uint8_t* valid;                   /* [n_queries]                                                 */
  float* point;                     /* [n_queries][3] the deskewed ray (:79-81)                    */
  double* point_f64;                /* [n_queries][3] the same before the cast                     */
  double* pose;                     /* [n_queries][7] T_WS at the query's stamp                    */
  double* speed;                    /* [n_queries][3] v_W                                          */
  double* omega_S;                  /* [n_queries][3]                                              */
  int32_t* n_before;                /* [n_scans] queries older than t_start                        */
} okvisgpu_lidar_deskew_result;
int okvisgpu_lidar_deskew(okvisgpu_ctx* ctx, const okvisgpu_lidar_deskew_batch* batch,
                          okvisgpu_lidar_deskew_result* result);

/* ---------------------------------------------------------------- voxel-grid downsampling
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * VoxelDownSample<float> (okvis_mapping/include/okvis/VoxelGridFilter.hpp:46-67; timer "8.3
 * Downsampling", LidarMotionUndistortion::downsample :87-103) for a batch of clouds on the GPU: keep[i]
 * = 1 for the first point, in input order, of every voxel of its cloud, among the points with use[i] !=
 * 0 (use = NULL: all; the host's filterObserved result, so that the deskewed array need not be
 * compacted). The voxel of a point is, per component, the single-precision quotient p /
 * float(voxel_size), correctly rounded (Eigen promotes the double divisor to the expression's float
 * scalar; lattice points sit on voxel faces, so a reciprocal multiply would move them), truncated toward
 * zero to int32: the voxels around 0 are double width, as in the reference. A point with a non-finite
 * component or a quotient outside int32 is never kept (undefined behaviour in the reference).
 * Deviation: the kept points are reported in input order; the reference emits them in
 * std::unordered_map iteration order, which is implementation-defined, and then subsamples randomly
 * (downsamplePointCloud, which stays with the caller).
 * Either output may be NULL. n_clouds = 0 and empty clouds are valid. Independent of the problem set
 * with okvisgpu_set_problems; uses the context's device and stream and returns with the results in the
 * caller's arrays. A cloud's result does not depend on the rest of the batch and is the same bits on
 * every run. OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a NULL ctx,
 * batch or result, a missing array, a negative count, cloud_begin not starting at 0 or not monotone, a
 * voxel_size that is not finite and positive (okvisgpu_last_error names the cloud), more than 2^29
 * points, and between okvisgpu_solve_begin and _solve_end. OKVISGPU_ERR_DEVICE if the hash table ran
 * out of slots (it holds two per point, so it cannot). */
typedef struct okvisgpu_voxel_downsample_batch {
  int32_t n_clouds;
  const int32_t* cloud_begin;       /* [n_clouds+1] CSR into the point arrays                      */
  const float* point;               /* [n_points][3]                                               */
  const double* voxel_size;         /* [n_clouds]                                                  */
  const uint8_t* use;               /* [n_points] or NULL = all                                    */
} okvisgpu_voxel_downsample_batch;

typedef struct okvisgpu_voxel_downsample_result {  /* caller-owned, either may be NULL */
  uint8_t* keep;                    /* [n_points]                                                  */
  int32_t* n_kept;                  /* [n_clouds]                                                  */
} okvisgpu_voxel_downsample_result;
int okvisgpu_voxel_downsample(okvisgpu_ctx* ctx, const okvisgpu_voxel_downsample_batch* batch,
                              okvisgpu_voxel_downsample_result* result);

/* ---------------------------------------------------------------- keypoint-coverage overlap
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * The mask painting by which the reference picks a frame's keyframe, decides on a new keyframe and rates
 * the tracking, for a batch of jobs on the GPU: ViSlamBackend::overlapFraction
 * (okvis_ceres/src/ViSlamBackend.cpp:2903-2989; the loops of mostOverlappedStateId :2780-2809,
 * currentLoopclosureStateId :2811-2836, prunePlaceRecognitionFrames :2838-2870 and
 * Frontend::matchMotionStereo, okvis_frontend/src/Frontend.cpp:1985-2014), the two parts of
 * Frontend::doWeNeedANewKeyframe (Frontend.cpp:1186-1295) and ViSlamBackend::trackingQuality
 * (ViSlamBackend.cpp:261-300). Every result is an integer count or one IEEE division of two counts.
 *
 * Frames: image_begin is a CSR of camera images per frame; an image has its full-resolution rows and cols
 * (rows == 0 or cols == 0: image(im).empty()) and, through kp_begin, its keypoints: keypoint =
 * cv::KeyPoint::pt as getCvKeypoint returns it, landmark = MultiFrame::landmarkId raw (0 = none; whether
 * the landmark still exists is not looked at, as in overlapFraction), flag read by kind 3 only.
 * Grid and disc, per image and job: G_r = rows / 10, G_c = cols / 10 (integer division), R =
 * int(double(min(G_r, G_c)) * factor) truncated. A keypoint's centre is, per component, cvRound(float(
 * double(pt) * 0.1)), ties to even (Point2f * double is computed in double and stored as float; the
 * cv::Point conversion is cvRound). The disc is what OpenCV's 8-connected integer Circle() fills for
 * cv::FILLED (cv::circle with LINE_8 and shift 0), cut to the grid: with the midpoint recurrence (err = 0,
 * dx = R, dy = 0, plus = 1, minus = 2R - 1; while dx >= dy: visit (dx, dy); dy++, err += plus, plus += 2,
 * if err > 0 { err -= minus, dx--, minus -= 2 }) and hw[dy] = max(hw[dy], dx), hw[dx] = max(hw[dx], dy)
 * over the visits, the disc is {(cx + ox, cy + oy): |ox| <= hw[|oy|], |oy| <= R}; R = 4 gives hw =
 * [4, 3, 3, 2, 0], 49 pixels. `detections` is the union of the discs of all keypoints of the image,
 * `matches` that of the matched ones; per image I = popcount(matches & detections), U = popcount(matches |
 * detections), both computed as written.
 * Deviations: OpenCV is not part of the reference snapshot, so the disc and the rounding are
 * this library's reading of OpenCV 4, pinned by the tables of DESIGN.md §4; a keypoint with a non-finite
 * coordinate, or one whose centre lies beyond 2^30, paints nothing (cvRound is undefined there).
 *
 * Kind 0, overlapFraction(A, B): over the non-empty images of each frame, M = {non-zero ids of A} n {those
 * of B}; a keypoint is matched iff its id is in M. M empty: exactly 0.0 (the counts are still those
 * painted). Else per side overlap = sum I / sum U by plain IEEE division and the result is (o_B < o_A) ? o_B
 * : o_A (std::min). Keypoints of an empty image take no part (:2922). A and B need the same image count;
 * A = B is allowed.
 * Kind 1, the "other frames" loop of doWeNeedANewKeyframe (:1245-1280): only B is painted, a keypoint of B
 * is matched iff its id is non-zero and among the ids of A (all images of A, :1219); the result is sum I /
 * sum U of B as it falls.
 * Kind 2, its current-frame part (:1202-1231): frame A alone, matched iff id != 0; sum I / sum U.
 * n_keypoints serves the caller's `< 7 * numFrames` test.
 * Kind 3, trackingQuality: frame A alone, matched iff flag != 0 (the caller evaluates "the landmark exists
 * and is observed from another frame", :282-291). Per image pointArea = int(radius * radius * pi) with the
 * untruncated double radius, I += max(0, popcount(matches) - pointArea), U += G_r G_c - pointArea; the
 * result is matchedPoints < 8 ? 0.0 : I / U with matchedPoints the flagged keypoints of the frame.
 * 0 / 0 gives the quiet NaN 0xFFF8000000000000, the result of that division on x86-64.
 *
 * Groups (optional): group_begin is a CSR over the jobs in job order. group_best = the last job of the
 * group whose overlap is >= the running best (starting at 0.0 and updated by it): the `>=` of
 * mostOverlappedStateId; a NaN never qualifies; -1 for an empty or all-NaN group. group_max = the fold m =
 * (m < v) ? v : m from 0.0 (std::max of :1279).
 *
 * Every output may be NULL. n_jobs = 0, frames without images and images without keypoints are valid.
 * Independent of the problem set with okvisgpu_set_problems (needs none, leaves the device parameter sets
 * alone); uses the context's device and stream and returns with the results in the caller's arrays. A
 * job's result does not depend on the rest of the batch and is the same bits on every run.
 * OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a NULL ctx, batch or result,
 * a missing array, a negative count, a CSR not starting at 0 or not monotone, group_begin beyond n_jobs, a
 * negative rows or cols, a frame index out of range, an unknown kind, kind 0 with differing image counts,
 * kind 3 without flag, a factor that is not finite and >= 0, a radius above
 * OKVISGPU_OVERLAP_MAX_RADIUS, an image whose grid needs more than OKVISGPU_OVERLAP_MASK_WORDS 32-bit
 * words per mask (G_r * ceil(G_c / 32); both masks of an image live in 64 KiB of LDS), and between
 * okvisgpu_solve_begin and _solve_end; okvisgpu_last_error names the offender. OKVISGPU_ERR_DEVICE if an
 * id table ran out of slots (a frame's table holds the smallest power of two >= two slots per keypoint, so
 * it cannot). */
#define OKVISGPU_OVERLAP_MASK_WORDS 8192
#define OKVISGPU_OVERLAP_MAX_RADIUS 1024
typedef struct okvisgpu_frame_overlap_batch {
  int32_t n_frames;
  const int32_t* image_begin;       /* [n_frames+1] CSR into the image arrays                      */
  const int32_t* rows;              /* [n_images] full resolution                                  */
  const int32_t* cols;              /* [n_images]                                                  */
  const int32_t* kp_begin;          /* [n_images+1] CSR into the keypoint arrays                   */
  const float* keypoint;            /* [n_kp][2] cv::KeyPoint::pt (x, y)                           */
  const uint64_t* landmark;         /* [n_kp] landmarkId, 0 = none                                 */
  const uint8_t* flag;              /* [n_kp] or NULL; kind 3                                      */
  int32_t n_jobs;
  const int32_t* job_kind;          /* [n_jobs] 0..3                                               */
  const int32_t* job_frame_a;       /* [n_jobs]                                                    */
  const int32_t* job_frame_b;       /* [n_jobs] kinds 0 and 1 (NULL when there are none)           */
  const double* job_radius_factor;  /* [n_jobs] kptradius_ / kptrad                                */
  int32_t n_groups;
  const int32_t* group_begin;       /* [n_groups+1] CSR into the jobs, or NULL with n_groups = 0   */
} okvisgpu_frame_overlap_batch;

typedef struct okvisgpu_frame_overlap_result {  /* caller-owned, any may be NULL */
  double* overlap;                  /* [n_jobs]                                                    */
  int32_t* count;                   /* [n_jobs][4] I, U of side A, I, U of side B; unpainted: 0    */
  int32_t* n_matched;               /* [n_jobs][2] matched keypoints per side                      */
  int32_t* n_keypoints;             /* [n_jobs] keypoints of frame A, all images                   */
  int32_t* group_best;              /* [n_groups] a job index or -1                                */
  double* group_max;                /* [n_groups]                                                  */
} okvisgpu_frame_overlap_result;
int okvisgpu_frame_overlap(okvisgpu_ctx* ctx, const okvisgpu_frame_overlap_batch* batch,
                           okvisgpu_frame_overlap_result* result);

/* ---------------------------------------------------------------- map matching
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * The matching of Frontend::matchToMap (okvis_frontend/src/Frontend.cpp:1299-1741) on the GPU: the
 * candidate preparation of :1335-1508 and the two matching passes, matchToMapByThread (:1745-1827)
 * and matchToMapByThreadUnitialised (:1831-1956, with triangulateFast, stereo_triangulation.cpp:30-112).
 * One batch is one map shared by n_jobs jobs; a job is one camera image of the current frame in one
 * pass (0: the initialised-landmark pass, 1: the uninitialised pass). Landmarks are in ascending
 * LandmarkId order and each landmark's observations in std::set<KeypointIdentifier> order (ascending
 * frame, camera, keypoint): the iteration orders of the reference's maps; observations are walked
 * backwards, as rbegin() does. normalised(v) below is v / |v| for |v|^2 > 0 and v otherwise (Eigen).
 *
 * Candidates, per job and landmark passing landmark_use: T_WC1 = pose_prepare T_SC[camera], p_W =
 * hp.xyz / hp.w, r_W = p_W - r_WC1, e_W = normalised(r_W), r = max(0.01, |r_W|). The landmark is
 * skipped when projectHomogeneous(T_WC1^-1 hp_W) is Invalid (|z| < 1e-12; radtan8 with rho > 9) or
 * Behind (inside the image and z <= 0: a point behind the camera that projects outside the image is not
 * skipped; no mask), or lies more than reprThreshold = 3 + f (imu_use ? 0.06 : 0.34), f = (fu + fv) / 2,
 * outside [0, width] x [0, height]. Per observation, newest first, with F = fu + fv (the sum here, the
 * mean elsewhere, as in the reference), T_WC_old = T_WS[obs_pose] T_SC[obs_camera] and r_old = p_W -
 * r_WC_old: while the landmark is not yet 3D it becomes 3D if normalised(r_W) . normalised(r_W -
 * (0.2 / F / quality) r_old) > cos(10 / F) (plain IEEE arithmetic: quality 0 gives NaN and the
 * landmark stays not-3D); unless loop_closure the observation is skipped if cosV = e_W .
 * normalised(r_old) < cos(0.6) or scaleChange = |r - |r_old|| / r > 0.5; score = 0.5 (acos(cosV) / 0.6 +
 * scaleChange / 0.5). Three slots start at score 1.0; the slot to replace is the first holding the
 * strictly largest score (the scan starting from 0.0), and the observation is stored there only if its
 * score is below that slot's; a slot keeps the descriptor, e0_W = C_WC_old normalised(obs_ray) and
 * r0_W = r_WC_old.
 * Deviation: a landmark without a stored slot is left out (cand_n = -1); the reference keeps one row
 * of uninitialised descriptor-pool memory for it (:1488).
 *
 * Pass 0: a keypoint takes part unless it carries a landmark and loop_closure is 0. It walks the 3D
 * candidates in landmark order and within a landmark in slot order; a landmark is skipped when
 * |projection - keypoint|^2 > reprThreshold^2; a candidate is a record iff its Hamming distance over
 * the 48 bytes is < best (as doubles; best starts at matching_threshold and then holds the last
 * record's distance). A record sets the match, adds 1 to n_records and the reprojection distance to
 * record_repr_sum.
 * Pass 1: T_WC1 from pose_match, sigma = 1 / f (the mean f); a keypoint takes part if ray_valid and the
 * rule above; e1_W = C_WC1 normalised(ray). It walks the candidates that are not 3D. For a candidate
 * with dist < best: if e0 . e1 < cos 6 sigma, with et = normalised(r_WC1 - r0), n0 = normalised(e0 x
 * et), n1 = normalised(e1 x et), it is rejected if n0 . n1 < cos 6 sigma or (e0 x e1) . normalised(n0 +
 * n0) > 0 (n0 twice, as written at :1914); then triangulateFast(r0, e0, r_WC1, e1, sigma); rejected if
 * not valid or if the point is closer than 0.2 m to r0 or to r_WC1. If the landmark is the one the
 * keypoint carries, n_records grows by 1 and the landmark's remaining slots are left, nothing else
 * changing; otherwise it is a record (best, match, n_records) and the triangulated point is stored
 * only if the result is not parallel: `point` is that of the keypoint's last non-parallel record,
 * which may belong to an earlier landmark than its match, and zero when there is none.
 * Both passes are independent of the reference's thread count; the result equals the serial walk's:
 * the match is the first candidate in order attaining the minimum over the admissible ones, the
 * records are the strict prefix minima.
 * The reference's per-thread reprErr (:1821, :1826) is the sum of the reprojection distances of a
 * thread's records over their count; the caller forms it from n_records and record_repr_sum of the
 * thread's keypoints. That regrouping of the sum changes rounding only.
 *
 * Independent of the problem set with okvisgpu_set_problems (needs none, leaves the device parameter
 * sets alone); uses the context's device and stream and returns with the results in the caller's
 * arrays. A job's result does not depend on the other jobs of the batch and is the same bits on every
 * run. n_jobs = 0, jobs without keypoints and maps without landmarks or observations are valid (-1 /
 * zero outputs). OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a NULL ctx,
 * batch or result, missing arrays, a CSR array not starting at 0 or not monotone, a camera, pose, pass
 * or carried-landmark index out of range, and between okvisgpu_solve_begin and _solve_end;
 * okvisgpu_last_error names the offender. */
typedef struct okvisgpu_match_batch {
  /* --- the map */
  int32_t n_poses;
  const double* poses;              /* [n_poses][7] T_WS of the old frames                         */
  int32_t n_cameras;
  const okvisgpu_camera* cameras;   /* [n_cameras]                                                 */
  const double* extrinsics;         /* [n_cameras][7] T_SC                                         */
  int32_t n_landmarks;
  const double* landmarks;          /* [n_landmarks][4] hp_W, ascending LandmarkId                 */
  const double* landmark_quality;   /* [n_landmarks]                                               */
  const uint8_t* landmark_use;      /* [n_landmarks] loopClosureLandmarksToUseExclusively, NULL = all */
  const int32_t* obs_begin;         /* [n_landmarks+1] CSR: observations of landmark l             */
  const int32_t* obs_pose;          /* [n_obs] index into poses                                    */
  const int32_t* obs_camera;        /* [n_obs]                                                     */
  const uint8_t* obs_descriptor;    /* [n_obs][48]                                                 */
  const double* obs_ray;            /* [n_obs][3] e_C of getBackProjection, not normalised         */
  /* --- scalars */
  int32_t imu_use;                  /* params.imu.use                                              */
  int32_t loop_closure;             /* 1 = called with a non-null exclusive set                    */
  double matching_threshold;        /* briskMatchingThreshold_, 60.0 in the reference              */
  /* --- jobs */
  int32_t n_jobs;
  const int32_t* job_camera;        /* [n_jobs]                                                    */
  const int32_t* job_pass;          /* [n_jobs] 0 / 1                                              */
  const double* job_pose_prepare;   /* [n_jobs][7] T_WS1 when the candidates were prepared         */
  const double* job_pose_match;     /* [n_jobs][7] T_WS1 now (pass 1 runs after a solve moved it)  */
  const int32_t* kp_begin;          /* [n_jobs+1] CSR into the keypoint arrays                     */
  /* --- keypoints */
  const double* keypoint;           /* [n_kp][2]                                                   */
  const uint8_t* descriptor;        /* [n_kp][48]                                                  */
  const double* ray;                /* [n_kp][3] the back-projection ...                           */
  const uint8_t* ray_valid;         /* [n_kp]    ... and its bool                                  */
  const int32_t* landmark;          /* [n_kp] index of the landmark the keypoint carries, -1 = none */
} okvisgpu_match_batch;

typedef struct okvisgpu_match_result {  /* caller-owned, any may be NULL */
  int32_t* match_landmark;          /* [n_kp] landmark index, -1 = none                            */
  int32_t* match_distance;          /* [n_kp] Hamming distance of the match, -1 = none             */
  int32_t* n_records;               /* [n_kp]                                                      */
  double* record_repr_sum;          /* [n_kp] pass 0 (0 in a pass-1 job)                           */
  double* point;                    /* [n_kp][4] pass 1 (0 in a pass-0 job)                        */
  int32_t* cand_n;                  /* [n_jobs][n_landmarks] -1 = not a candidate, else 1..3 slots */
  uint8_t* cand_is3d;               /* [n_jobs][n_landmarks]                                       */
  int32_t* cand_obs;                /* [n_jobs][n_landmarks][3] observation of each slot, -1 unused */
  double* cand_projection;          /* [n_jobs][n_landmarks][2] (0 for a non-candidate)            */
} okvisgpu_match_result;
int okvisgpu_match_to_map(okvisgpu_ctx* ctx, const okvisgpu_match_batch* batch, okvisgpu_match_result* result);

/* ---------------------------------------------------------------- frame-to-frame matching
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * The keypoint-against-keypoint BRISK matching of Frontend::matchMotionStereo's worker loop
 * (okvis_frontend/src/Frontend.cpp:2057-2149) and of Frontend::matchStereo's inner loop (:2259-2316) on
 * the GPU, with triangulateFast (stereo_triangulation.cpp:30-112). One batch is n_jobs independent jobs;
 * a job matches the keypoints of image 0 ("side 0", suffix 0) against those of image 1 ("side 1",
 * suffix 1) in one mode: 0 = motion stereo (side 0 an older keyframe's image `im`, side 1 the current
 * frame's image `im`; job_camera0 = job_camera1 = im), 1 = stereo (two images of one multiframe;
 * job_pose0 = job_pose1). The keypoints of each side are stored job after job (kp0_begin / kp1_begin).
 * normalised(v) below is v / |v| for |v|^2 > 0 and v otherwise (Eigen).
 *
 * Both modes, per job: T_WCi = job_pose_i job_extrinsics_i (C_WCi, r_WCi), f_i = (fu + fv) / 2 of camera
 * job_camera_i; per keypoint e_W = normalised(C_WCi ray). depth_i(p) = (C_WCi^T (p - r_WCi))_z.
 * A side-0 keypoint k0 walks the side-1 keypoints of its job that have use1 != 0, in ascending index,
 * with a running `best`; a candidate k1 whose Hamming distance over the 48 bytes is < best is tested
 * for admissibility and, if admissible, becomes the record: best = its distance, match = k1, point =
 * [p, 1] with p the triangulated point, initialisable = triangulateFast did not report parallel.
 *
 * Mode 0 (:2057-2149). k0 takes part iff use0 and ray_valid0; use0 is the caller's fold of the
 * landmarkId / isLandmarkAdded / isLandmarkInitialised / isObserved rules (:2058-2066, :2085) and use1
 * "carries no landmark" (:2037-2041). sigma = size0 / f0 * 0.125. best starts at matching_threshold
 * truncated to an unsigned integer (uint32_t distances = briskMatchingThreshold_). A candidate is
 * admissible iff ray_valid1, e0 . e1 >= 0.5, triangulateFast(r_WC0, e0, r_WC1, e1, sigma) is valid,
 * e0 . e1 >= 0.8, depth_0(p) >= 0.2 and depth_1(p) >= 0.2 (each written as "not <", so a NaN passes, as
 * in the reference). The record also holds quality = acos(normalised(p - r_WC0) . normalised(p -
 * r_WC1)) in plain IEEE arithmetic (a rounded argument above 1 gives NaN, as in the reference). After
 * the walk the record is kept only if best < matching_threshold (as doubles) and projectHomogeneous(
 * camera1, T_WC1^-1 point) is Successful (|z| >= 1e-12; radtan8: rho <= 9; inside [0, width) x [0,
 * height); z > 0; no mask) and lands less than 4.0 px from keypoint1 (:2140-2147). If that check fails
 * the keypoint has no match: there is no fall-back to another candidate.
 * Mode 1 (:2259-2316). k0 takes part iff use0. best starts at matching_threshold as a double. A
 * candidate is admissible iff ray_valid0, ray_valid1, triangulateFast valid with sigma = max(size0 /
 * f0, size1 / f1) * 0.125, depth_0(p) >= 0.1, depth_1(p) >= 0.1 and e0 . e1 >= 0.8. quality is 0 and
 * there is no final projection test. What follows in the reference (:2318-2387: merge, setLandmark,
 * addLandmark and the two 4-px checks against the estimator's point) reads and mutates estimator state
 * and stays with the caller, as does the insertion loop of mode 0 (:2159-2201).
 * In both modes admissibility does not depend on best, so the result equals the serial walk's and is
 * independent of the reference's thread count: the match is the first admissible side-1 keypoint
 * attaining the minimum admissible distance below the threshold; point, initialisable and quality are
 * that candidate's.
 *
 * Results are indexed by side-0 keypoint; a keypoint without a match (or not taking part) gets match
 * -1, distance -1, point 0, initialisable 0, quality 0. `match` is the side-1 index within the job
 * (0 .. kp1_begin[j+1] - kp1_begin[j] - 1).
 *
 * Independent of the problem set with okvisgpu_set_problems (needs none, leaves the device parameter
 * sets alone); uses the context's device and stream and returns with the results in the caller's
 * arrays. A job's result does not depend on the other jobs of the batch and is the same bits on every
 * run. n_jobs = 0, a job with an empty side 0 or side 1 and all-zero use arrays are valid (empty / -1
 * outputs). OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a NULL ctx,
 * batch or result, missing arrays, negative counts, a CSR array not starting at 0 or not monotone, a
 * camera index or a mode out of range, and between okvisgpu_solve_begin and _solve_end;
 * okvisgpu_last_error names the offender. */
typedef struct okvisgpu_frame_match_batch {
  /* --- shared */
  int32_t n_cameras;
  const okvisgpu_camera* cameras;   /* [n_cameras]                                                 */
  double matching_threshold;        /* briskMatchingThreshold_, 60.0 in the reference              */
  /* --- jobs */
  int32_t n_jobs;
  const int32_t* job_mode;          /* [n_jobs] 0 = motion stereo, 1 = stereo                      */
  const int32_t* job_camera0;       /* [n_jobs] intrinsics of side 0                               */
  const int32_t* job_camera1;       /* [n_jobs] intrinsics of side 1 (mode 0: the same camera)     */
  const double* job_pose0;          /* [n_jobs][7] T_WS of side 0's frame                          */
  const double* job_pose1;          /* [n_jobs][7] T_WS of side 1's frame (mode 1: the same pose)  */
  const double* job_extrinsics0;    /* [n_jobs][7] T_SC of side 0 (mode 0: the older state's, :2021) */
  const double* job_extrinsics1;    /* [n_jobs][7] T_SC of side 1 (mode 0: the current state's, :2022) */
  const int32_t* kp0_begin;         /* [n_jobs+1] CSR into the side-0 keypoint arrays              */
  const int32_t* kp1_begin;         /* [n_jobs+1] CSR into the side-1 keypoint arrays              */
  /* --- side-0 keypoints */
  const double* keypoint0;          /* [n_kp0][2] (not read by the matching: for symmetry, may be NULL) */
  const double* size0;              /* [n_kp0]    getKeypointSize                                  */
  const uint8_t* descriptor0;       /* [n_kp0][48]                                                 */
  const double* ray0;               /* [n_kp0][3] getBackProjection, not normalised ...            */
  const uint8_t* ray_valid0;        /* [n_kp0]    ... and its bool                                 */
  const uint8_t* use0;              /* [n_kp0]    NULL = all 1                                     */
  /* --- side-1 keypoints */
  const double* keypoint1;          /* [n_kp1][2]                                                  */
  const double* size1;              /* [n_kp1]                                                     */
  const uint8_t* descriptor1;       /* [n_kp1][48]                                                 */
  const double* ray1;               /* [n_kp1][3]                                                  */
  const uint8_t* ray_valid1;        /* [n_kp1]                                                     */
  const uint8_t* use1;              /* [n_kp1]    NULL = all 1                                     */
} okvisgpu_frame_match_batch;

typedef struct okvisgpu_frame_match_result {  /* caller-owned, any may be NULL; all [n_kp0] */
  int32_t* match;                   /* side-1 keypoint index within the job, -1 = none             */
  int32_t* distance;                /* Hamming distance of the match, -1 = none                    */
  double* point;                    /* [n_kp0][4] hp_W = [p, 1], 0 without a match                 */
  uint8_t* initialisable;           /* 1 = the match's triangulation is not parallel               */
  double* quality;                  /* mode 0: the parallax angle of the match; mode 1: 0          */
} okvisgpu_frame_match_result;
int okvisgpu_match_frames(okvisgpu_ctx* ctx, const okvisgpu_frame_match_batch* batch,
                          okvisgpu_frame_match_result* result);

/* ---------------------------------------------------------------- place verification: matching
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * The descriptor matching of Frontend::verifyRecognisedPlace (okvis_frontend/src/Frontend.cpp:316-345,
 * timer "2.04 loop closure descriptor matching") on the GPU for a batch of candidates. A job is one
 * candidate: the landmarks of one old frame against the images of the new multiframe. Neither this
 * call nor okvisgpu_place_refine depends on the outcome of an earlier candidate, so every candidate of
 * a frame (:833, :877) can go into one batch and the host walks the results in candidate order.
 *
 * Images: n_images images of new frames, their descriptors stored image after image (kp_begin); jobs
 * normally share the images of one new multiframe. job_image[j][im] is the image of camera im, or -1
 * where that camera has no image. Landmarks: stored job after job (lm_begin), within a job in ascending
 * LandmarkId, as `landmarks` iterates at :317; a landmark's descriptors (desc_begin) are those of the old
 * frame's keypoints carrying it, in (camera, keypoint) order, as :276-313 pushes them. The filter of
 * :278-303 (lmId != 0, initialised, landmark.norm() >= 1e-12, the CNN classes) is the caller's fold: only
 * the surviving landmarks are passed.
 *
 * Per (landmark, camera) with K > 0 keypoints in the camera's image: distMin starts at
 * matching_threshold truncated to an unsigned integer (:326); the walk goes over the landmark's
 * descriptors in order and within a descriptor over k ascending; a candidate replaces the best iff its
 * Hamming distance over the 48 bytes is strictly smaller (:331); there is a match iff distMin <
 * matching_threshold, compared as doubles (:338). So the match is the first (descriptor, keypoint) in
 * that order attaining the minimum distance, if that minimum is below the truncated threshold. (:338
 * tests distMin itself: with a threshold that has a fractional part its start already passes, so a pair
 * whose walk replaces nothing is reported as the reference reports it, keypoint kMin = 0 at the truncated
 * threshold. okvis configures an integer, 60.) job_image = -1, K = 0 or a landmark without descriptors
 * (which the reference cannot have) give -1 / -1. job_matches is the reference's
 * ctr (:339), the number of (landmark, camera) matches of the job; the `ctr < minInliers` test (:349)
 * needs nothing else. The maps of :340-342 (`matches`, keyed by keypoint so that a later landmark
 * overwrites an earlier one on the same keypoint, and `points`) stay with the caller, as do the RANSAC
 * (:353-388, opengv) and the float-precision distinctiveness test (:390-432).
 *
 * Independent of the problem set with okvisgpu_set_problems (needs none, leaves the device parameter
 * sets alone); uses the context's device and stream and returns with the results in the caller's
 * arrays. A job's result does not depend on the rest of the batch and is the same bits on every run.
 * n_jobs = 0 is valid. OKVISGPU_ERR_INVALID_ARGUMENT, before anything is launched or written, for a
 * NULL ctx, batch or result, a missing array, a negative count, a CSR array not starting at 0 or not
 * monotone, an image index outside [-1, n_images), and between okvisgpu_solve_begin and _solve_end;
 * okvisgpu_last_error names the offender. */
typedef struct okvisgpu_place_match_batch {
  double matching_threshold;        /* briskMatchingThreshold_, 60.0 in the reference              */
  int32_t n_cameras;
  /* --- images of new frames */
  int32_t n_images;
  const int32_t* kp_begin;          /* [n_images+1] CSR into descriptor                            */
  const uint8_t* descriptor;        /* [n_kp][48]                                                  */
  /* --- jobs (candidates) */
  int32_t n_jobs;
  const int32_t* job_image;         /* [n_jobs][n_cameras] image of camera im, -1 = none           */
  const int32_t* lm_begin;          /* [n_jobs+1] CSR over the landmarks                           */
  /* --- landmarks */
  const int32_t* desc_begin;        /* [n_lm+1] CSR into old_descriptor                            */
  const uint8_t* old_descriptor;    /* [n_desc][48]                                                */
} okvisgpu_place_match_batch;

typedef struct okvisgpu_place_match_result {  /* caller-owned, any may be NULL */
  int32_t* match_keypoint;          /* [n_lm][n_cameras] keypoint index within the image, -1 = none */
  int32_t* match_distance;          /* [n_lm][n_cameras] Hamming distance of the match, -1 = none  */
  int32_t* job_matches;             /* [n_jobs] ctr                                                */
} okvisgpu_place_match_result;
int okvisgpu_place_match(okvisgpu_ctx* ctx, const okvisgpu_place_match_batch* batch,
                         okvisgpu_place_match_result* result);

/* ---------------------------------------------------------------- place verification: refinement
 * (An addition to ABI 6: a new entry point and two new structs; OKVISGPU_ABI_VERSION stays 6.)
 * The pose-only refinement of Frontend::verifyRecognisedPlace after its RANSAC and the evaluation that
 * follows (Frontend.cpp:434-598, timer "2.06 loop closure pose refinement") on the GPU. A job is one
 * candidate that survived the RANSAC: pose = T_Sold_Snew enters as the RANSAC model (:438) and leaves
 * as the solve's result (:562); its observations are the inlier correspondences in correspondence order
 * (:468), each with the landmark in the old frame's S coordinates (constant, :480; a landmark seen in
 * two cameras is simply given twice). The extrinsics are the current frame's T_SC (:456), constant (:460)
 * and shared by the batch, as is the loss: the reference uses {OKVISGPU_LOSS_CAUCHY, 0, 3.0, 0} (:447).
 *
 * The solve is ::ceres::Solve with the default Solver::Options but for max_num_iterations (:559):
 * TRUST_REGION / LEVENBERG_MARQUARDT over one 6-dimensional PoseManifold block, Jacobi scaling,
 * tolerances 1e-6 (function) / 1e-10 (gradient) / 1e-8 (parameter), radius 1e4 in [1e-32, 1e16],
 * min_relative_decrease 1e-3, LM diagonal clamped to [1e-6, 1e32], at most 5 consecutive invalid steps,
 * monotonic steps. Every residual is ReprojectionError::EvaluateWithMinimalJacobians(pose, obs_point,
 * T_SC of obs_camera), exactly what okvisgpu_eval_reprojection evaluates, with the loss applied through
 * Ceres' Corrector ("robust losses" above); cost = 1/2 sum rho(|r|^2). The trust-region loop is
 * TrustRegionMinimizer's as okvisgpu_solve runs it (iteration 0 with the gradient test, step validity
 * from the model cost change, the parameter and the function tolerance test before the acceptance test,
 * the same counting rules); the strategy is LevenbergMarquardtStrategy: with J the Jacobi-scaled
 * corrected Jacobian, diagonal = clamp(diag(J^T J), 1e-6, 1e32) (formed anew unless it is being reused),
 * D^2 = diagonal / radius, step = -(J^T J + D^2)^-1 J^T r; a failed factorisation or a non-finite step
 * is an invalid step. Accepted with step quality q: radius = min(1e16, radius / max(1/3, 1 - (2q -
 * 1)^3)), the decrease factor goes back to 2, a new diagonal is formed; rejected or invalid: radius /=
 * decrease factor, the decrease factor doubles, the diagonal is reused. Ceres solves the damped problem
 * by dense QR, the device solves the 6x6 normal equations by an FP64 Cholesky factorisation (a
 * rounding-level deviation). The pose written back is the lowest-cost accepted point.
 *
 * After the solve (:565-598), at the refined pose: per observation the weighted residual r without the
 * loss and its 2x6 minimal pose Jacobian J; the observation is an outlier iff |r| > 3.0 (written so: a
 * NaN counts as an inlier, as in the reference); inliers add J^T J to H, n_outliers counts the outliers.
 * The two ratio tests of :593-598 stay with the caller.
 *
 * num_iterations, num_successful_steps (iteration 0 included), num_unsuccessful_steps and
 * termination_type have the meaning of okvisgpu_summary's. A job without observations: pose untouched, H
 * zero, 0 iterations, costs 0, OKVISGPU_CONVERGENCE. A job whose initial evaluation is not finite:
 * OKVISGPU_FAILURE, 0 iterations, pose untouched (H and n_outliers are still evaluated there).
 *
 * Independent of the problem set with okvisgpu_set_problems; uses the context's device and stream and
 * returns with the results in the caller's arrays. A job's result does not depend on the rest of the
 * batch and is the same bits on every run. n_jobs = 0 is valid. OKVISGPU_ERR_INVALID_ARGUMENT, before
 * anything is launched or written, for a NULL ctx, batch or result, a missing array, a negative count,
 * obs_begin not starting at 0 or not monotone, a camera index out of range, an unknown distortion
 * model, an unknown loss kind, a non-positive loss scale, and between okvisgpu_solve_begin and
 * _solve_end; okvisgpu_last_error names the offender. */
typedef struct okvisgpu_place_refine_batch {
  /* --- the camera rig, shared by the batch */
  int32_t n_cameras;
  const okvisgpu_camera* cameras;   /* [n_cameras]                                                 */
  const double* extrinsics;         /* [n_cameras][7] T_SC of the current frame (:456)             */
  okvisgpu_loss loss;               /* the reference: {OKVISGPU_LOSS_CAUCHY, 0, 3.0, 0} (:447)     */
  int32_t max_num_iterations;       /* realtime_max_iterations (:559)                              */
  /* --- jobs (candidates that survived the RANSAC) */
  int32_t n_jobs;
  double* pose;                     /* [n_jobs][7] T_Sold_Snew, in: the RANSAC model, out: refined */
  const int32_t* obs_begin;         /* [n_jobs+1] CSR over the inlier observations                 */
  /* --- observations */
  const int32_t* obs_camera;        /* [n_obs]                                                     */
  const double* obs_keypoint;       /* [n_obs][2]                                                  */
  const double* obs_sqrt_info;      /* [n_obs][4] row-major 2x2, (8 / size) I                      */
  const double* obs_point;          /* [n_obs][4] the landmark in the old frame's S coordinates    */
} okvisgpu_place_refine_batch;

typedef struct okvisgpu_place_refine_result {  /* caller-owned, any may be NULL; all [n_jobs] */
  double* H;                        /* [n_jobs][36] row-major sum of J^T J over the inliers        */
  int32_t* n_outliers;              /* additionalOutliers (:587)                                   */
  double* initial_cost;
  double* final_cost;
  int32_t* num_iterations;
  int32_t* num_successful_steps;
  int32_t* num_unsuccessful_steps;
  int32_t* termination_type;        /* okvisgpu_termination                                        */
} okvisgpu_place_refine_result;
int okvisgpu_place_refine(okvisgpu_ctx* ctx, const okvisgpu_place_refine_batch* batch,
                          okvisgpu_place_refine_result* result);

/* ---------------------------------------------------------------- post-solve landmark pass
 * (An addition to ABI 6: a new entry point and a new struct; no existing struct or call changes, so
 * OKVISGPU_ABI_VERSION stays 6 and a caller built against the earlier header keeps working.)
 * ViGraph::updateLandmarks (ViGraph.cpp:1762-1841) and ViGraph::areLandmarksInFrontOfCameras
 * (:1621-1642) for every window of the batch on the GPU, on the parameter values okvisgpu_get_params
 * would return now (after a solve the solved ones, after okvisgpu_set_problems / _update_params the
 * uploaded ones; T_SC is the camera's pose-kind block, so a variable extrinsics block counts with its
 * solved value). Per landmark, over its observations in (pose, camera) order: the unit ray dir_W from
 * the camera to the landmark (reversed when the landmark lies behind the camera) and the norm of the
 * weighted reprojection residual without loss (what okvisgpu_eval_reprojection returns);
 * observations with a norm above 2.5 are skipped. quality = the norm of the per-axis root sums of
 * squared deviations of the kept rays from their mean (0 without a kept ray); quality > 0.04 makes
 * the landmark initialised; otherwise, if an observation (kept or not) saw it closer than 0.1 m in
 * depth, it is re-placed on the ray of the kept observation with the smallest residual, at its
 * distance (at least 0.1 m) in front of that camera, as [x y z 1]: in both device parameter sets and
 * in the caller's `landmarks` array. Nothing else in the caller's arrays changes. Indices are the
 * caller's (landmark l of okvisgpu_problem.landmarks, observation o of obs_*). A landmark without
 * observations: quality 0, not initialised, untouched. Constant landmarks are treated like any other.
 * in_front is evaluated on the values at entry, before any landmark is re-placed. */
typedef struct okvisgpu_landmark_update {   /* one per window; arrays caller-owned, any may be NULL */
  double*  quality;                 /* [n_landmarks]   ViGraph::Landmark::quality                    */
  uint8_t* initialised;             /* [n_landmarks]   hPoint->setInitialized()                      */
  uint8_t* reset;                   /* [n_landmarks]   1 = the estimate was replaced (best-ray reset) */
  double*  obs_error;               /* [n_observations] |weighted reprojection residual|, no loss    */
  int32_t  n_initialised, n_reset;  /* out                                                           */
  int32_t  in_front;                /* out: ViGraph::areLandmarksInFrontOfCameras() on the entry values */
  int32_t  reserved;
} okvisgpu_landmark_update;
/* updates: [n_windows of the last okvisgpu_set_problems]. OKVISGPU_ERR_INVALID_ARGUMENT for a NULL
 * ctx or updates and between okvisgpu_solve_begin and _solve_end; OKVISGPU_ERR_NO_PROBLEM when no
 * problem is set. */
int okvisgpu_update_landmarks(okvisgpu_ctx* ctx, okvisgpu_landmark_update* updates);

/* ---------------------------------------------------------------- co-observation counts
 * (An addition to ABI 6 like the landmark pass: a new entry point and a new struct.)
 * ViGraph::computeCovisibilities (ViGraph.cpp:727-785) for every window of the batch on the GPU, in
 * the caller's pose and landmark indices. A landmark adds 1 to counts[i][j] when it is not excluded
 * and has at least one observation in pose i and at least one in pose j, i != j; two cameras of one
 * frame count once. Every observation counts, whatever its residual, its loss flag or the landmark's
 * constant flag; extrinsics blocks are not states and never appear. A landmark observed from a single
 * pose makes that pose visible and adds to its n_observed, but adds no pair (visibleFrames_ is filled
 * before the pair loop, :740-743). The result depends only on the structure given to the last
 * okvisgpu_set_problems and on landmark_excluded, not on parameter values; nothing in the caller's
 * problem arrays or on the device's parameter sets changes. A window without landmarks or
 * observations gives all zeros and any = 0. */
typedef struct okvisgpu_covisibility {   /* one per window; arrays caller-owned, any may be NULL */
  const uint8_t* landmark_excluded; /* in  [n_landmarks] 1 = leave out (classification 10 / 11, ViGraph.cpp:735); NULL = none */
  int32_t* counts;                  /* out [n_poses][n_poses] row-major, symmetric, zero diagonal:
                                           counts[i][j] = ViGraph::covisibilities(i, j)              */
  int32_t* n_observed;              /* out [n_poses] included landmarks the state observes          */
  uint8_t* visible;                 /* out [n_poses] state is in visibleFrames_ (n_observed > 0)     */
  int32_t  n_pairs;                 /* out: unordered pairs i<j with counts > 0                      */
  int32_t  n_visible;               /* out                                                           */
  int32_t  any;                     /* out: computeCovisibilities' return value (n_pairs > 0)        */
  int32_t  path;                    /* out: 0 = window-in-LDS kernel, 1 = tiled kernel (informational) */
} okvisgpu_covisibility;
/* out: [n_windows of the last okvisgpu_set_problems]. OKVISGPU_ERR_INVALID_ARGUMENT for a NULL ctx or
 * out and between okvisgpu_solve_begin and _solve_end; OKVISGPU_ERR_NO_PROBLEM when no problem is set. */
int okvisgpu_covisibilities(okvisgpu_ctx* ctx, okvisgpu_covisibility* out);

/* ---------------------------------------------------------------- okvis Component graphs
 * Component::load (okvis_ceres/src/Component.cpp:50-383) as an okvisgpu_problem: states (pose and
 * speed/bias blocks, ordered by state id), landmarks (ordered by id), one extrinsics block per camera,
 * EDGE_IMU factors with their measurements, EDGE_OBS reprojections with the measurement and the
 * information 64/size^2 of the frame's FRAME:KEYPOINT (float, as cv::KeyPoint) and Cauchy(1). The
 * camera intrinsics and IMU parameters are configuration (not in the file) and are passed in. No
 * priors and no constant blocks are added: the caller freezes what its solve needs. Host only. */
typedef struct okvisgpu_graph okvisgpu_graph;
int okvisgpu_graph_load(const char* path, const okvisgpu_camera* cameras, int32_t n_cameras,
                        const okvisgpu_imu_params* imu, okvisgpu_graph** out);
/* The problem view into the graph's arrays (valid until destroy; solves write into them). */
const okvisgpu_problem* okvisgpu_graph_problem(okvisgpu_graph* g);
/* File ids of the states / landmarks in problem order and the state time stamps (may be NULL). */
int okvisgpu_graph_ids(const okvisgpu_graph* g, uint64_t* state_ids, int64_t* state_t_ns, uint64_t* landmark_ids);
void okvisgpu_graph_destroy(okvisgpu_graph* g);
/* Component::save (Component.cpp:385-506) of a problem (one speed/bias block per state, isotropic
 * reprojection information): ids = problem indices, time stamps from state_t_ns or the IMU factors. */
int okvisgpu_graph_save(const okvisgpu_problem* p, const int64_t* state_t_ns, const char* path);

/* Problem statistics of the batch held by a context (the ::ceres::Solver::Summary counters
 * num_parameter_blocks / num_residual_blocks / num_effective_parameters_reduced analogues, plus the
 * layout figures bench.py's roofline work model needs). Sums over all windows. */
typedef struct okvisgpu_problem_stats {
  int32_t n_windows;
  int32_t cholesky_launches;        /* launches of the tile-parallel factorisation (roots + steps) */
  int64_t n_poses, n_speed_biases, n_landmarks, n_landmarks_free, n_extrinsics_free;
  int64_t n_observations, n_visits, n_imu, n_imu_samples, n_pose_priors, n_sb_priors, n_relpose;
  int64_t reduced_dim;              /* sum of the reduced (Schur) dimensions                      */
  int64_t s_tiles_nonzero;          /* 64x64 tiles of S the tile-sparse LLT touches (incl. fill)  */
  int64_t s_tiles_dense;            /* lower-triangle tiles of the dense reduced matrices          */
  int64_t n_block_pairs, n_visit_segments, n_partial_blocks;
  int64_t arena_bytes;              /* device memory held by the context                           */
  int64_t cholesky_split_windows;   /* windows whose nested-dissection parts factor independently */
} okvisgpu_problem_stats;
int okvisgpu_get_stats(okvisgpu_ctx* ctx, okvisgpu_problem_stats* stats);

/* Host-only plan of one window's reduced system (no device, no context; for tests and tools): the
 * state order a batch below one window per CU gives it (nested_dissection = 1) or the natural one
 * (0), its tile pattern and the tile-parallel factorisation schedule. Any output may be NULL.
 *   info[8]:        natural reduced dimension, S dimension (64-padded), tiles T, structurally
 *                   non-zero tiles (after fill), launches (roots + updates), split tL, split tS
 *                   (0 0: none), gap rows
 *   tile_nz[T*T]:   the filled lower-triangular tile pattern (row-major, 1 = non-zero)
 *   step_launch[T]: launch of step k's band updates (0: the step has none)
 *   natural[dim]:   natural index of each row of S (-1: gap or padding row), dim = info[1]
 * Pass tile_nz / step_launch / natural sized from a first call with them NULL. */
int okvisgpu_plan_window(const okvisgpu_problem* problem, int32_t nested_dissection, int64_t* info,
                         uint8_t* tile_nz, int32_t* step_launch, int32_t* natural);

/* Host-only digest of a batch's plan on a device of cu_count compute units (no device, no context;
 * development: pins the planner's output bit for bit, tests/test_plan_digest.py). Any output may be
 * NULL.
 *   totals[16]:  f_total, s_total, linv_total, fwd_total, defer_total, max_fpad, max_panels,
 *                n_chol_launches, n_panels, n_band_updates, n_band_updates_diag, any_split, obs_iso,
 *                bytes of the uploaded region, bytes of the scratch region, 0
 *   *n_entries:  device arrays of the arena table; per entry i < min(capacity, *n_entries), in
 *                table order: names[32 * i] (NUL-terminated), region[i] (0 uploaded, 1 scratch),
 *                bytes[i], hash[i] = FNV-1a-64 of the uploaded bytes (0 for scratch)
 * Size the arrays from a first call with capacity 0. */
int okvisgpu_plan_digest(const okvisgpu_problem* problems, int32_t n_windows, int32_t cu_count, int64_t* totals,
                         int32_t capacity, int32_t* n_entries, char* names, int32_t* region, int64_t* bytes,
                         uint64_t* hash);

/* Host-only: the assembly work items of a batch's plan as the records the assembly kernels read,
 * beside what the planner's separate arrays hold for the same items (no device, no context;
 * development, tests/test_assembly_paths.py). Items in kernel order: the heavy pose-pose list, the
 * light pose-pose list, the speed/bias list (pads of the XCD interleave included).
 *   counts[4]:      items of the three lists, records in all
 *   records[12 i]:  window (-1: pad, the rest 0), visit run begin, partial-block run begin, factor run
 *                   begin, end, f-vector index of the row block, of the column block, leading
 *                   dimension of S, S element offset (low, high word), flags (1 diagonal, 2 / 4 the
 *                   row / column block is a speed/bias block), 0
 *   arrays[16 i]:   pair (-1: pad, the rest 0), pair_win, pair_cbegin[pair], pair_runs[pair][0..1],
 *                   pair_cbegin[pair + 1], pair_fi, pair_fj, fb_off[fi], fb_off[fj], fb_kind[fi],
 *                   fb_kind[fj], win_foff, win_fpad, win_soff, 0
 * for i < min(capacity, counts[3]); records / arrays may be NULL. Size them from a first call with
 * capacity 0. */
int okvisgpu_plan_assembly(const okvisgpu_problem* problems, int32_t n_windows, int32_t cu_count, int32_t* counts,
                           int32_t capacity, int32_t* records, int64_t* arrays);

/* Host-only: what the batch size decides about the launches of a solve on a device of cu_count
 * compute units (no device, no context; development, tests/test_launch_regime.py). any_split: a
 * window has a nested-dissection split; persistent_fits / pipe_fits: the persistent / pipelined
 * Cholesky's LDS holds the largest window; cholesky_schedule: options.cholesky_schedule;
 * serial_graph (0 / 1), lin_prep (0) and graph_iters (K) are the measurement overrides
 * OKVISGPU_SERIAL_GRAPH, OKVISGPU_LIN_PREP and OKVISGPU_GRAPH_ITERS, -1 = not set.
 *   regime[7]: few windows, many windows, one-stream graph, GN prep inside the linearisation,
 *              gradient test inside the assembly, iterations per graph, resolved Cholesky schedule */
int okvisgpu_launch_regime(int32_t n_windows, int32_t cu_count, int32_t any_split, int32_t persistent_fits,
                           int32_t pipe_fits, int32_t cholesky_schedule, int32_t serial_graph, int32_t lin_prep,
                           int32_t graph_iters, int32_t* regime);

/* Copy device parameter values back into the caller's host arrays without solving. */
int okvisgpu_get_params(okvisgpu_ctx* ctx);

/* ---------------------------------------------------------------- evaluation entry points
 * (::ceres::Problem::Evaluate / EvaluateResidualBlock analogues; also the parity-test hooks)
 *
 * okvisgpu_evaluate: total cost 1/2 sum rho(|r|^2) of window w at the current device parameters.
 */
int okvisgpu_evaluate(okvisgpu_ctx* ctx, int32_t window, double* cost);

/* Linearise window w at the current parameters and eliminate the landmarks (DENSE_SCHUR):
 *   S   = H_ff - H_fl H_ll^-1 H_lf,   rhs = g_f - H_fl H_ll^-1 g_l,   g = J^T r (Cauchy-corrected)
 * with Jacobi scaling (if jacobi_scaling) and the dogleg LM diagonal D = diag(J^T J)^(1/2)*sqrt(mu)
 * exactly as the solver's first Gauss-Newton solve would form them. Outputs (host, may be NULL):
 *   S   [dim*dim] row-major (full symmetric), rhs [dim], cost [1], dim_out [1].
 * The reduced ordering is: for i = 0 .. max(n_poses, n_speed_biases)-1: pose i (6, if variable)
 * then speed/bias i (9, if variable); then the variable extrinsics in camera order (6 each). */
int okvisgpu_linearize_reduce(okvisgpu_ctx* ctx, int32_t window, int32_t jacobi_scaling, double mu,
                              double* S, double* rhs, double* cost, int32_t* dim_out);

/* Development (a test hook, not part of the drop-in boundary): one Gauss-Newton solution of window w
 * at the current parameters, as the first iteration of a solve forms it. Of `options` (NULL: the
 * defaults) jacobi_scaling, cholesky_schedule, min_lm_diagonal and max_lm_diagonal apply; the rest
 * is ignored. The whole resident batch is linearised at the damping mu, reduced, factorised and
 * back-substituted (GN prep, assembly, Cholesky, landmark back substitution); two vectors of
 * window w come back (host, either may be NULL):
 *   y_f [dim]             the solution of S y_f = rhs, S and rhs being what
 *                         okvisgpu_linearize_reduce(ctx, w, jacobi_scaling, mu, ...) returns with the
 *                         same LM diagonal bounds, in its reduced ordering. y_f is in the
 *                         Jacobi-scaled space; DoglegStrategy's gauss_newton_step_ is -D y_f
 *                         (D = diagonal_, the dogleg scaling).
 *   y_l [3 * n_landmarks] per landmark, in the caller's order, zero for a constant landmark:
 *                         y_l = V'^-1 (s g_l - s W^T s_p y_p), V' the landmark's scaled and damped
 *                         3x3 block, s / s_p the Jacobi scales of the landmark / its poses, W its
 *                         pose-landmark blocks and y_p the poses' (and variable extrinsics') rows of
 *                         y_f; gauss_newton_step_ = -D y_l.
 * dim_out [1] receives the reduced dimension. Returns OKVISGPU_ERR_NUMERICAL when the step of window
 * w failed (a landmark block or a pivot of S not positive definite at this mu: a solve would retry
 * with a larger mu); the outputs are then untouched. Not callable between okvisgpu_solve_begin and
 * okvisgpu_solve_end; the solve state is scratch afterwards, as after okvisgpu_linearize_reduce. */
int okvisgpu_gauss_newton_step(okvisgpu_ctx* ctx, int32_t window, const okvisgpu_options* options,
                               double mu, double* y_f, double* y_l, int32_t* dim_out);

/* Raw per-residual evaluation for parity tests (EvaluateWithMinimalJacobians semantics, no loss):
 *   reprojection: r [n_obs][2], J_pose [n_obs][2][6], J_landmark [n_obs][2][3] (minimal, row-major)
 *   imu:          r [n_imu][15], J [n_imu][15][30] minimal columns (pose0 6, sb0 9, pose1 6, sb1 9)
 * Any output pointer may be NULL. The IMU call updates the factor's preintegration state exactly as
 * ImuError::EvaluateWithMinimalJacobians does (ImuError.cpp:833-859). */
int okvisgpu_eval_reprojection(okvisgpu_ctx* ctx, int32_t window, double* r, double* J_pose,
                               double* J_landmark);
int okvisgpu_eval_imu(okvisgpu_ctx* ctx, int32_t window, int32_t redo_always, double* r, double* J);
/*   relative pose: r [n_relpose][6], J [n_relpose][6][12] minimal (reference pose 6, other pose 6) */
int okvisgpu_eval_relpose(okvisgpu_ctx* ctx, int32_t window, double* r, double* J);
/*   host-evaluated blocks, through the device path (gather, host_evaluate, upload; no loss):
 *   r [n_host][15], J [n_host][15][30] minimal in the IMU column layout (first pose-kind block 0..5,
 *   first speed/bias 6..14, second pose-kind 15..20, second speed/bias 21..29), rows >= dim zero. */
int okvisgpu_eval_host(okvisgpu_ctx* ctx, int32_t window, double* r, double* J);

/* ---------------------------------------------------------------- synthetic windows
 * Host-side generator of the synthetic sliding windows the benchmark is quoted on:
 * EuRoC stereo rig (config/euroc/okvis2.yaml:2-32), smooth sinusoidal 6-DoF trajectory
 * (okvis_ceres/test/TestImuError.cpp:86-185 style), 200 Hz IMU, landmarks in a 2-20 m band,
 * observations with N(0,1px^2) noise and information 64/8^2 = I, perturbed initial states, priors as
 * ViGraph::addStatesInitialise (ViGraph.cpp:347-370), Cauchy(1) on every reprojection.
 * std::mt19937_64(seed). No GPU is touched. */
typedef struct okvisgpu_synth_config {
  int32_t n_keyframes;              /* S10: 10, S50: 50 */
  int32_t n_landmarks;              /* S10: 500, S50: 2000 */
  int32_t n_observations;           /* S10: 4000, S50: 16000 */
  int32_t max_obs_per_landmark;     /* 20 */
  double kf_dt_s;                   /* 0.1 */
  double imu_rate_hz;               /* 200 */
  double pixel_noise;               /* 1.0 */
  double init_sigma_pos, init_sigma_rot, init_sigma_lm, init_sigma_vel; /* 0.05 0.01 0.05 0.02 */
  uint64_t seed;
  /* pose-graph edges (TwoPoseStandardGraphErrorConst) from keyframe i to i + relpose_stride,
   * i = 0, 1, ...: information from sigmas 0.02 m / 0.005 rad (random rotation of the frame),
   * linearisation point = the ground-truth relative pose perturbed at that noise, DeltaX_ small.
   * 0 (default) = none, as in the benchmark windows. */
  int32_t n_relpose;
  int32_t relpose_stride;
  int32_t relpose_kind;             /* 0 pose-graph edges, 1 RelativePoseError, 2 alternating */
  /* online extrinsics calibration (ABI 4): both T_SC blocks variable, initialised at the true T_SC
   * perturbed by N(0, sigma_r^2) / N(0, sigma_alpha^2) and held by a PoseError prior centred on that
   * initial value (ViGraph.cpp:372-382). 0 (default) = constant extrinsics. */
  int32_t do_extrinsics;
  double extrinsics_sigma_r, extrinsics_sigma_alpha;  /* 0.001 m, 0.005 rad (config/hilti22) */
} okvisgpu_synth_config;

typedef struct okvisgpu_synth_window okvisgpu_synth_window;  /* owns all arrays of one problem */

void okvisgpu_synth_default_config(okvisgpu_synth_config* cfg, int32_t n_keyframes,
                                   int32_t n_landmarks, int32_t n_observations, uint64_t seed);
int okvisgpu_synth_create(const okvisgpu_synth_config* cfg, okvisgpu_synth_window** out);
/* The problem view into the window's arrays (valid until destroy). */
const okvisgpu_problem* okvisgpu_synth_problem(okvisgpu_synth_window* w);
/* Ground truth: poses [n_kf][7], landmarks [n_lm][4], speed_biases [n_kf][9] (may be NULL); the
 * true extrinsics are okvisgpu_synth_true_extrinsics [n_cameras][7]. */
int okvisgpu_synth_ground_truth(const okvisgpu_synth_window* w, double* poses, double* landmarks,
                                double* speed_biases);
/* Reset the problem's parameter arrays (and imu_state) to the generated initial estimate. */
int okvisgpu_synth_reset(okvisgpu_synth_window* w);
int okvisgpu_synth_true_extrinsics(const okvisgpu_synth_window* w, double* extrinsics);
void okvisgpu_synth_destroy(okvisgpu_synth_window* w);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* OKVISGPU_H_ */
