// match_geometry.hpp — the geometry the descriptor matchers share (kernels_match.hip: Frontend::matchToMap;
// kernels_match_frames.hip: Frontend::matchMotionStereo / matchStereo): 3-vectors, Eigen's normalized(),
// T_WS T_SC, the 48-byte Hamming distance, the wavefront minimum and triangulateFast (also kernels_place.hip:
// Frontend::verifyRecognisedPlace). Device-only, register-resident.
#pragma once

#include "okvisgpu_math.hpp"

namespace okg {

constexpr int kNoDist = 0x7fffffff;

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// Eigen's normalized(): v / |v| for |v|^2 > 0, else v
__device__ __forceinline__ void normalised3(const double v[3], double o[3]) {
  const double z = dot3(v, v);
  if (z > 0.0) {
    const double n = sqrt(z);
    o[0] = v[0] / n; o[1] = v[1] / n; o[2] = v[2] / n;
  } else {
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  }
}
// T_WC = T_WS T_SC: C [9] row-major, r [3]
__device__ __forceinline__ void composeWC(const double* T_WS, const double* T_SC, double C[9], double r[3]) {
  double C_WS[9], C_SC[9];
  qrot(qnormalize(Q{T_WS[3], T_WS[4], T_WS[5], T_WS[6]}), C_WS);
  qrot(qnormalize(Q{T_SC[3], T_SC[4], T_SC[5], T_SC[6]}), C_SC);
  mm3(C_WS, C_SC, C);
  double t[3];
  mv3(C_WS, T_SC, t);
  r[0] = T_WS[0] + t[0]; r[1] = T_WS[1] + t[1]; r[2] = T_WS[2] + t[2];
}
// brisk::Hamming::PopcntofXORed over 48 bytes as 12 dwords
__device__ __forceinline__ int hamming48(const uint32_t a[12], gptr<uint32_t> b) {
  int d = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) d += __popc(a[i] ^ b[i]);
  return d;
}

// the minimum over the wavefront, in every lane
__device__ __forceinline__ int waveMinInt(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
  return v;
}

// triangulateFast (stereo_triangulation.cpp:30-112)
__device__ __forceinline__ void triangulateFast(const double p1[3], const double e1[3], const double p2[3],
                                                const double e2[3], double sigma, double hp[3], bool& valid,
                                                bool& parallel) {
  parallel = false;
  valid = true;
  const double t12[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double b0 = dot3(t12, e1), b1 = dot3(t12, e2);
  const double A00 = dot3(e1, e1), A10 = dot3(e1, e2), A01 = -A10, A11 = -dot3(e2, e2);
  const double det = A00 * A11 - A10 * A01;
  const bool invertible = fabs(det) > 1.0e-12;
  double l0 = 0.0, l1 = 0.0;
  if (invertible) {
    const double invdet = 1.0 / det;
    l0 = (A11 * invdet) * b0 + (-A01 * invdet) * b1;
    l1 = (-A10 * invdet) * b0 + (A00 * invdet) * b1;
  }
  const double c26 = cos(2.6 * sigma);
  double mid[3];
  if (!invertible || l0 < 0.01 || l1 < 0.01) {
    parallel = true;
    const double s = 40.0 * fmax(0.01, sqrt(dot3(t12, t12)));
#pragma unroll
    for (int i = 0; i < 3; ++i) mid[i] = (p1[i] + 0.5 * t12[i]) + s * (e1[i] + e2[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) mid[i] = ((l0 * e1[i] + p1[i]) + (l1 * e2[i] + p2[i])) / 2.0;
  }
  const double m1[3] = {mid[0] - p1[0], mid[1] - p1[1], mid[2] - p1[2]};
  const double m2[3] = {mid[0] - p2[0], mid[1] - p2[1], mid[2] - p2[2]};
  double n1[3], n2[3];
  normalised3(m1, n1);
  normalised3(m2, n2);
  if (dot3(e1, n1) < c26) valid = false;
  if (dot3(e2, n2) < c26) valid = false;
  if (!parallel && dot3(n2, n1) > cos(6.0 * sigma)) parallel = true;
  hp[0] = mid[0]; hp[1] = mid[1]; hp[2] = mid[2];
}

}  // namespace okg
