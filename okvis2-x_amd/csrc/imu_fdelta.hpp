// imu_fdelta.hpp — the block-sparse F_delta of one IMU integration step, its product with a
// 15-vector and the constants of the LDS exchange of P <- F P F^T, shared by the kernels that propagate a 15x15
// covariance column by column in 16-lane groups: k_eval_imu (ImuError::redoPreintegration / append,
// kernels_eval.hip), k_imu_propagate_group (ImuError::propagation, kernels_imu_propagate.hip) and
// k_gps_async (GpsErrorAsynchronous::redoPreintegration, kernels_gps.hip). The recursions have the
// same non-identity blocks (03, 06 = dt I, 09, 012, 39, 63, 69, 612); the entries are the group step's
// (imu_chain_group_body.hpp) and k_eval_imu's own.
#pragma once

#include <hip/hip_runtime.h>

namespace okg {

// F_delta (ImuError.cpp:395-410, :672-682) of one step: non-identity 3x3 blocks
constexpr int kF03 = 0, kF09 = 9, kF012 = 18, kF39 = 27, kF63 = 36, kF69 = 45, kF612 = 54, kFdt = 63;

// Row r of -[w]x times u, the zero entry of the row skipped: the two remaining products in the
// column order of the full row (F03 and F63 are such blocks; their slots hold w only, 3 LDS reads
// per applyF instead of 9).
__device__ __forceinline__ double negSkewRow(const double* w, int r, double u0, double u1, double u2) {
  return r == 0 ? w[2] * u1 + (-w[1]) * u2 : (r == 1 ? (-w[2]) * u0 + w[0] * u2 : w[1] * u0 + (-w[0]) * u1);
}
// out = F v   (block rows: 0 dp, 1 dalpha, 2 dv, 3 bg, 4 ba); F read from LDS (group broadcast)
__device__ __forceinline__ void applyF(const double* F, const double* v, double* out) {
  const double dt = F[kFdt];
  const double w03[3] = {F[kF03], F[kF03 + 1], F[kF03 + 2]}, w63[3] = {F[kF63], F[kF63 + 1], F[kF63 + 2]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double a = v[r];
    a += negSkewRow(w03, r, v[3], v[4], v[5]);
    a += dt * v[6 + r];
    a += F[kF09 + r * 3 + 0] * v[9] + F[kF09 + r * 3 + 1] * v[10] + F[kF09 + r * 3 + 2] * v[11];
    a += F[kF012 + r * 3 + 0] * v[12] + F[kF012 + r * 3 + 1] * v[13] + F[kF012 + r * 3 + 2] * v[14];
    out[r] = a;
    out[3 + r] = v[3 + r] + F[kF39 + r * 3 + 0] * v[9] + F[kF39 + r * 3 + 1] * v[10] + F[kF39 + r * 3 + 2] * v[11];
    double c = negSkewRow(w63, r, v[3], v[4], v[5]);
    c += v[6 + r];
    c += F[kF69 + r * 3 + 0] * v[9] + F[kF69 + r * 3 + 1] * v[10] + F[kF69 + r * 3 + 2] * v[11];
    c += F[kF612 + r * 3 + 0] * v[12] + F[kF612 + r * 3 + 1] * v[13] + F[kF612 + r * 3 + 2] * v[14];
    out[6 + r] = c;
  }
#pragma unroll
  for (int r = 9; r < 15; ++r) out[r] = v[r];
}

__device__ __forceinline__ double groupSum(double v) {  // sum over the 16 lanes of a group
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 1, 64);
  return v;
}

// ---- the column exchange of k_imu_propagate_group and k_gps_async: four groups per wavefront, each
// with a 15 x kColStride tile of LDS
constexpr int kGroupsPerWave = 4;
constexpr int kColStride = 17;  // row stride of the LDS exchange: lanes walking a column hit distinct banks

}  // namespace okg
