// loss.hpp — robust losses (okvisgpu.h "robust losses"): ::ceres::LossFunction::Evaluate
// of the Ceres loss family (ceres-solver >= 2.1 loss_function.cc, restated: CauchyLoss, TukeyLoss,
// HuberLoss, SoftLOneLoss, ArctanLoss, TolerantLoss), rho[0..2] = rho(s), rho'(s), rho''(s). Used by
// the planner's validation (plan.cpp), by the host-evaluated factors' corrector (runtime.cpp) and, on
// the device, by the place refinement's corrector (kernels_place.hip).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "../../include/okvisgpu.h"

// (plan.cpp is also compiled by a plain host compiler, without HIP)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define OKG_LOSS_HD __host__ __device__ inline
#else
#define OKG_LOSS_HD inline
#endif

namespace okg {

inline bool lossValid(const okvisgpu_loss& L) {
  switch (L.kind) {
    case OKVISGPU_LOSS_NONE: return true;
    case OKVISGPU_LOSS_TOLERANT: return L.a >= 0.0 && L.b > 0.0 && std::isfinite(L.a) && std::isfinite(L.b);
    case OKVISGPU_LOSS_CAUCHY: case OKVISGPU_LOSS_TUKEY: case OKVISGPU_LOSS_HUBER: case OKVISGPU_LOSS_SOFTLONE:
    case OKVISGPU_LOSS_ARCTAN: return L.a > 0.0 && std::isfinite(L.a);
  }
  return false;
}

OKG_LOSS_HD void lossRho(const okvisgpu_loss& L, double s, double* rho) {
  const double a = L.a;
  switch (L.kind) {
    case OKVISGPU_LOSS_CAUCHY: {
      const double b = a * a, c = 1.0 / b;
      const double sum = 1.0 + s * c, inv = 1.0 / sum;
      rho[0] = b * std::log(sum);
      rho[1] = std::max(DBL_MIN, inv);
      rho[2] = -c * (inv * inv);
      return;
    }
    case OKVISGPU_LOSS_TUKEY: {
      const double a2 = a * a;
      if (s <= a2) {  // inlier region
        const double v = 1.0 - s / a2, v2 = v * v;
        rho[0] = a2 / 3.0 * (1.0 - v2 * v);
        rho[1] = v2;
        rho[2] = -2.0 / a2 * v;
      } else {  // outlier region: constant cost, no gradient
        rho[0] = a2 / 3.0;
        rho[1] = 0.0;
        rho[2] = 0.0;
      }
      return;
    }
    case OKVISGPU_LOSS_HUBER: {
      const double b = a * a;
      if (s > b) {
        const double r = std::sqrt(s);
        rho[0] = 2.0 * a * r - b;
        rho[1] = std::max(DBL_MIN, a / r);
        rho[2] = -rho[1] / (2.0 * s);
      } else {
        rho[0] = s;
        rho[1] = 1.0;
        rho[2] = 0.0;
      }
      return;
    }
    case OKVISGPU_LOSS_SOFTLONE: {
      const double b = a * a, c = 1.0 / b;
      const double sum = 1.0 + s * c, t = std::sqrt(sum);
      rho[0] = 2.0 * b * (t - 1.0);
      rho[1] = std::max(DBL_MIN, 1.0 / t);
      rho[2] = -(c * rho[1]) / (2.0 * sum);
      return;
    }
    case OKVISGPU_LOSS_ARCTAN: {
      const double b = 1.0 / (a * a);
      const double sum = 1.0 + s * s * b, inv = 1.0 / sum;
      rho[0] = a * std::atan2(s, a);
      rho[1] = std::max(DBL_MIN, inv);
      rho[2] = -2.0 * s * b * (inv * inv);
      return;
    }
    case OKVISGPU_LOSS_TOLERANT: {
      const double b = L.b, c = b * std::log(1.0 + std::exp(-a / b));
      const double x = (s - a) / b;
      if (x > 36.7) {  // 1 + e^x == e^x in double beyond ln(2^53)
        rho[0] = s - a - c;
        rho[1] = 1.0;
        rho[2] = 0.0;
      } else {
        const double ex = std::exp(x);
        rho[0] = b * std::log(1.0 + ex) - c;
        rho[1] = std::max(DBL_MIN, ex / (1.0 + ex));
        rho[2] = 0.5 / (b * (1.0 + std::cosh(x)));
      }
      return;
    }
    default:
      rho[0] = s;
      rho[1] = 1.0;
      rho[2] = 0.0;
  }
}

// the loss of host factor h: host_loss (ABI 6), else CauchyLoss(1) where host_cauchy is set
inline okvisgpu_loss hostLoss(const okvisgpu_problem* p, int h) {
  if (p->host_loss) return p->host_loss[h];
  okvisgpu_loss L{OKVISGPU_LOSS_NONE, 0, 1.0, 0.0};
  if (p->host_cauchy && p->host_cauchy[h]) L.kind = OKVISGPU_LOSS_CAUCHY;
  return L;
}

}  // namespace okg
