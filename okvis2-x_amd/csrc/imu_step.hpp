// imu_step.hpp — the sample and step-input layer of the IMU stepping kernels
// (kernels_imu_propagate.hip, kernels_gps.hip, kernels_lidar.hip): one sample as stored with its
// clamped prefetch load, the inputs of one trapezoid step and the step's dq (ImuError.cpp:644-650;
// ViInterface.cpp:696-703 is the same text). The step on them is imu_chain.hpp's.
#pragma once

#include "okvisgpu_math.hpp"

namespace okg {

struct RawSample {  // one sample as stored: stamp, gyro, accelerometer
  int64_t t;
  double ga[6];
};
// Sample min(k, N - 1) of the N > 0 samples that start at sbeg. The loops keep samples k and k + 1 in
// registers and load sample k + 2 at the top of step k, so that a step does not begin by waiting for
// its own loads. (Past the end the last sample stands in: the reference reads nothing it uses there,
// such a step has dt <= 0.)
__device__ __forceinline__ RawSample loadRawSample(const int64_t* ts, const double* ga, int sbeg, int N, int k) {
  const int s = sbeg + min(k, N - 1);
  RawSample r;
  r.t = gmem(ts)[s];
  const auto g = gmem(ga + 6 * (size_t)s);
#pragma unroll
  for (int j = 0; j < 6; ++j) r.ga[j] = g[j];
  return r;
}

// One step's inputs: dt, the bias-corrected mean rates, the step's end and the saturation flags.
struct PropStep {
  double dt, w[3], a[3];  // dt, omega_S_true, acc_S_true (:645, :655)
  bool gyr_sat, acc_sat;
  int64_t nexttime;
};

// One pass of the sample loop up to the integrity check (ImuError.cpp:584-640; the same text at
// GpsErrorAsynchronous.cpp:341-398) for sample k of N whose integration time is `time` and ends at
// t_end: false when the sample is skipped (dt <= 0, :607-609). On true: dt, the (interpolated)
// measurements less the biases, the step's end `nexttime` and the saturation flags against a_max, g_max.
__device__ __forceinline__ bool stepSample(double a_max, double g_max, int N, int64_t t_end, int k, const RawSample& cur,
                                           const RawSample& nxt, int64_t time, bool started, const double* bg,
                                           const double* ba, PropStep& s) {
  const bool last = k + 1 == N;
  double om0[3], ac0[3], om1[3], ac1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    om0[j] = cur.ga[j];
    ac0[j] = cur.ga[3 + j];
    om1[j] = nxt.ga[j];
    ac1[j] = nxt.ga[3 + j];
  }
  const int64_t ts0 = cur.t;
  int64_t nexttime = last ? t_end : nxt.t;
  double dt = durToSec(nexttime - time);
  if (t_end < nexttime) {  // clip to t_end, interpolate the second measurement (:598-605)
    const double interval = durToSec(nexttime - ts0);
    nexttime = t_end;
    dt = durToSec(nexttime - time);
    const double r = dt / interval;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      om1[j] = (1.0 - r) * om0[j] + r * om1[j];
      ac1[j] = (1.0 - r) * ac0[j] + r * ac1[j];
    }
  }
  if (!(dt > 0.0)) return false;
  if (!started) {  // the first integrated step starts at t_start (:612-617)
    const double r = dt / durToSec(nexttime - ts0);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      om0[j] = r * om0[j] + (1.0 - r) * om1[j];
      ac0[j] = r * ac0[j] + (1.0 - r) * ac1[j];
    }
  }
  s.gyr_sat = false;
  s.acc_sat = false;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    s.gyr_sat = s.gyr_sat || fabs(om0[j]) > g_max || fabs(om1[j]) > g_max;
    s.acc_sat = s.acc_sat || fabs(ac0[j]) > a_max || fabs(ac1[j]) > a_max;
    s.w[j] = 0.5 * (om0[j] + om1[j]) - bg[j];
    s.a[j] = 0.5 * (ac0[j] + ac1[j]) - ba[j];
  }
  s.dt = dt;
  s.nexttime = nexttime;
  return true;
}

// dq of one step (:644-650) and sin / cos of theta_half for the right Jacobian
__device__ __forceinline__ Q stepDq(const PropStep& s, double& sh, double& ch) {
  const double theta_half = sqrt(s.w[0] * s.w[0] + s.w[1] * s.w[1] + s.w[2] * s.w[2]) * 0.5 * s.dt;
  sincos(theta_half, &sh, &ch);
  double sincv;  // ode::sinc (ode.hpp:34-46)
  if (fabs(theta_half) > 1.0e-6) {
    sincv = sh / theta_half;
  } else {
    const double x_2 = theta_half * theta_half, x_4 = x_2 * x_2, x_6 = x_2 * x_2 * x_2;
    sincv = 1.0 - (1.0 / 6.0) * x_2 + (1.0 / 120.0) * x_4 - (1.0 / 5040.0) * x_6;
  }
  const double sth = sincv * 0.5 * s.dt;
  return Q{sth * s.w[0], sth * s.w[1], sth * s.w[2], ch};
}

}  // namespace okg
