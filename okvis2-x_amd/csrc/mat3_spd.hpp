// mat3_spd.hpp — the two 3x3 operations the GPS functors apply to their information and covariance
// matrices (GpsErrorAsynchronous.cpp:87, :185-193; GpsErrorSynchronous.cpp:44-47), for the kernel
// (kernels_gps.hip) and for the host's argument check (okvisgpu_gps_evaluate). Plain C++: no HIP here.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define OKG_M3 __host__ __device__ inline
#else
#define OKG_M3 inline
#endif

namespace okg {

// Eigen's inverse of a fixed 3x3 (cofactors over the determinant); row-major
OKG_M3 void inv3(const double A[9], double o[9]) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c10 = A[5] * A[6] - A[3] * A[8], c20 = A[3] * A[7] - A[4] * A[6];
  const double invdet = 1.0 / (A[0] * c00 + A[1] * c10 + A[2] * c20);
  o[0] = c00 * invdet; o[1] = (A[2] * A[7] - A[1] * A[8]) * invdet; o[2] = (A[1] * A[5] - A[2] * A[4]) * invdet;
  o[3] = c10 * invdet; o[4] = (A[0] * A[8] - A[2] * A[6]) * invdet; o[5] = (A[2] * A[3] - A[0] * A[5]) * invdet;
  o[6] = c20 * invdet; o[7] = (A[1] * A[6] - A[0] * A[7]) * invdet; o[8] = (A[0] * A[4] - A[1] * A[3]) * invdet;
}

// Eigen::LLT<Matrix3d>(A).matrixL().transpose(): the upper factor U with U^T U = A, from A's lower
// triangle; row-major. False when a pivot is not positive (or not a number): U is then unusable.
OKG_M3 bool chol3U(const double A[9], double U[9]) {
  const double d0 = A[0];
  const double l00 = sqrt(d0), l10 = A[3] / l00, l20 = A[6] / l00;
  const double d1 = A[4] - l10 * l10;
  const double l11 = sqrt(d1), l21 = (A[7] - l20 * l10) / l11;
  const double d2 = A[8] - l20 * l20 - l21 * l21;
  const double l22 = sqrt(d2);
  U[0] = l00; U[1] = l10; U[2] = l20;
  U[3] = 0.0; U[4] = l11; U[5] = l21;
  U[6] = 0.0; U[7] = 0.0; U[8] = l22;
  return d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
}

}  // namespace okg
