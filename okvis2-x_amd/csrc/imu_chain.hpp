// imu_chain.hpp — the IMU integration chain of one trapezoid step, once, for the kernels that walk
// it: k_imu_propagate_lane / k_imu_propagate_group (ImuError::propagation, ImuError.cpp:644-682),
// k_gps_async (GpsErrorAsynchronous::redoPreintegration, GpsErrorAsynchronous.cpp:402-452) and
// k_lidar_chain / k_lidar_points (BatchedLidarPropagator, ViInterface.cpp:696-715). The three
// reference texts are the same recursion. imu_step.hpp below this has the samples and a step's
// inputs, imu_fdelta.hpp F_delta.
//
// The step is a statement, not a function: imu_chain_lane_body.hpp and imu_chain_group_body.hpp are
// included at the place of the step and work on the kernel's own variables, by name. As
// __forceinline__ functions on a state struct they compute other bits (1-ulp differences in most
// outputs on the device, profiles/imu_chain_ab.txt). The compiler optimises a callee on its own before
// it inlines it, and a struct changes the order of the loop's carried values; either changes the order
// in which the operands of commutative FP operations end up, and which product of a sum a*b + c*d
// becomes the FMA follows that order (R[2] and R[7] of qrot came out swapped). Included as text on
// the same variables, the step compiles to the instruction stream it had when it was written out in
// every kernel.
#pragma once

#include "imu_fdelta.hpp"
#include "imu_step.hpp"
#include "okvisgpu_math.hpp"

namespace okg {

// What the chain without Jacobian and covariance carries: Delta_q, acc_integral, acc_doubleintegral.
struct LaneChain {
  Q Dq;
  double ai[3], adi[3];
};

}  // namespace okg
