// window_export.hpp — the host loops that hand one window's numbers back in the caller's layout
// (resident_calls.cpp): linearisation records split into residuals and Jacobians, and reduced
// vectors and matrices exported in the natural order (pose i, speed/bias i, ..., extrinsics),
// whatever order the window's reduced system is held in (nested dissection: permuted slots and gap
// rows, nat[r] < 0). No HIP here: the sources are staged host bytes, the copies are the caller's.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace okg {

// n records of K values each: the first R of a record to r[n][R], the rest to J[n][K - R]. Either
// output may be null; n == 0 reads nothing.
inline void splitRecords(const double* rec, size_t n, int K, int R, double* r, double* J) {
  for (size_t f = 0; f < n; ++f, rec += K) {
    if (r) std::copy(rec, rec + R, r + f * (size_t)R);
    if (J) std::copy(rec + R, rec + K, J + f * (size_t)(K - R));
  }
}

// out[nat[r]] = v[r] for the fdim rows of v that are no gap rows.
inline void scatterNatural(const double* v, const int32_t* nat, int fdim, double* out) {
  for (int r = 0; r < fdim; ++r)
    if (nat[r] >= 0) out[nat[r]] = v[r];
}

// The lower triangle of the first fdim rows of M (row stride fpad) into both triangles of out (row
// stride dn), gap rows and columns left out. M's upper triangle and padding are not read.
inline void scatterNaturalSym(const double* M, const int32_t* nat, int fdim, int fpad, int dn, double* out) {
  for (int r = 0; r < fdim; ++r)
    for (int q = 0; q <= r; ++q) {
      const int a = nat[r], b = nat[q];
      if (a < 0 || b < 0) continue;
      out[(size_t)a * dn + b] = M[(size_t)r * fpad + q];
      out[(size_t)b * dn + a] = M[(size_t)r * fpad + q];
    }
}

}  // namespace okg
