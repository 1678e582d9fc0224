// launch_regime_check — okvisgpu_launch_regime (okvis2-x_amd/csrc/plan.cpp, compiled into this
// program for the host with -fsanitize=address,undefined) against a table on stdin: one case per
// line, the nine inputs then the seven expected outputs (tests/test_launch_regime.py writes its own
// table). Exit status 0 and "launch_regime_check ok: N cases" when every case matches.
#include <cstdio>

#include "okvisgpu.h"

int main() {
  int n = 0, bad = 0;
  for (;; ++n) {
    int v[16], got = 0;
    while (got < 16 && std::scanf("%d", &v[got]) == 1) ++got;
    if (got == 0) break;
    int32_t r[7];
    if (got != 16 || okvisgpu_launch_regime(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], r) != OKVISGPU_OK) {
      std::fprintf(stderr, "case %d: %d of 16 numbers, or the call failed\n", n, got);
      return 2;
    }
    for (int i = 0; i < 7; ++i)
      if (r[i] != v[9 + i]) {
        std::fprintf(stderr, "case %d: output %d is %d, expected %d\n", n, i, (int)r[i], v[9 + i]);
        ++bad;
      }
  }
  if (bad || n == 0) return 1;
  std::printf("launch_regime_check ok: %d cases\n", n);
  return 0;
}
