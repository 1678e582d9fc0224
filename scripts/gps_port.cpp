// gps_port.cpp — a stand-alone single-thread C++ port of tests/_gps_error.py (GpsErrorAsynchronous with
// a fresh functor: the pre-integration with four dense 15x15 dPdsigma matrices, as the reference carries
// them, then the residual, sqrt_info and the three minimal Jacobians), the CPU figure of
// scripts/gps_timing.py on the inputs that script writes: the port on this host, not the reference (which
// needs Eigen and is not buildable here). Own small-matrix arithmetic, no dependency.
//   g++ -O2 -std=c++17 scripts/gps_port.cpp -o scripts/gps_port        (timing)
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 scripts/gps_port.cpp -o gps_port_san  (checks)
// Usage: gps_port <input file> [reps]   -> one JSON line
// Input (native endianness): int64 n, int64 n_samples, double par[7], double r_SA[3], then poses [n][7],
// speed_biases [n][9], T_GW [n][7], measurement [n][3], information [n][9], int64 t_k [n], t_g [n],
// int64 sample_begin [n+1], int64 sample_t [n_samples], double sample_gyr_acc [n_samples][6].
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

void mul(const double* A, const double* B, double* C, int R, int K, int N) {  // C = A B
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < N; ++c) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += A[r * K + k] * B[k * N + c];
      C[r * N + c] = s;
    }
}
void mulT(const double* A, const double* B, double* C, int R, int K, int N) {  // C = A B^T, B [N x K]
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < N; ++c) {
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += A[r * K + k] * B[c * K + k];
      C[r * N + c] = s;
    }
}
void crossMx(const double* v, double* C) {
  C[0] = 0; C[1] = -v[2]; C[2] = v[1];
  C[3] = v[2]; C[4] = 0; C[5] = -v[0];
  C[6] = -v[1]; C[7] = v[0]; C[8] = 0;
}
void qmul(const double* a, const double* b, double* o) {
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = x; o[1] = y; o[2] = z; o[3] = w;
}
void qrot(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
void qnormalize(double* q) {
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= n;
}
double sinc(double x) {
  if (std::fabs(x) > 1e-6) return std::sin(x) / x;
  const double x2 = x * x;
  return 1.0 - x2 / 6.0 + x2 * x2 / 120.0 - x2 * x2 * x2 / 5040.0;
}
void rightJacobian(const double* p, double* J) {
  const double phi = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  double X[9], X2[9];
  crossMx(p, X);
  mul(X, X, X2, 3, 3, 3);
  double a = -0.5, b = 1.0 / 6.0;
  if (phi >= 1e-4) {
    a = -(1.0 - std::cos(phi)) / (phi * phi);
    b = (phi - std::sin(phi)) / (phi * phi * phi);
  }
  for (int i = 0; i < 9; ++i) J[i] = a * X[i] + b * X2[i];
  J[0] += 1; J[4] += 1; J[8] += 1;
}
double toSec(int64_t dns) {
  int64_t sec = dns / 1000000000LL, nsec = dns % 1000000000LL;
  if (nsec < 0) { nsec += 1000000000LL; sec -= 1; }
  return (double)sec + 1e-9 * (double)nsec;
}
void inv3(const double* A, double* o) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c10 = A[5] * A[6] - A[3] * A[8], c20 = A[3] * A[7] - A[4] * A[6];
  const double d = 1.0 / (A[0] * c00 + A[1] * c10 + A[2] * c20);
  o[0] = c00 * d; o[1] = (A[2] * A[7] - A[1] * A[8]) * d; o[2] = (A[1] * A[5] - A[2] * A[4]) * d;
  o[3] = c10 * d; o[4] = (A[0] * A[8] - A[2] * A[6]) * d; o[5] = (A[2] * A[3] - A[0] * A[5]) * d;
  o[6] = c20 * d; o[7] = (A[1] * A[6] - A[0] * A[7]) * d; o[8] = (A[0] * A[4] - A[1] * A[3]) * d;
}
void cholU(const double* A, double* U) {
  const double l00 = std::sqrt(A[0]), l10 = A[3] / l00, l20 = A[6] / l00;
  const double l11 = std::sqrt(A[4] - l10 * l10), l21 = (A[7] - l20 * l10) / l11;
  const double l22 = std::sqrt(A[8] - l20 * l20 - l21 * l21);
  U[0] = l00; U[1] = l10; U[2] = l20; U[3] = 0; U[4] = l11; U[5] = l21; U[6] = 0; U[7] = 0; U[8] = l22;
}
void setBlock(double* M, int ld, int r0, int c0, const double* B, double s) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[(r0 + r) * ld + c0 + c] = s * B[r * 3 + c];
}

struct Inputs {
  int64_t n = 0, ns = 0;
  double par[7], r_SA[3];
  std::vector<double> poses, sb, gw, z, info, ga;
  std::vector<int64_t> t_k, t_g, begin, ts;
};

// one factor: returns r [3], Jp [18], Jsb [27], Jg [18] in out [66]
void evaluate(const Inputs& I, int64_t i, double* out) {
  const double *pose = &I.poses[7 * i], *sb = &I.sb[9 * i], *G = &I.gw[7 * i];
  const int64_t t_k = I.t_k[i], t_g = I.t_g[i], s0 = I.begin[i], N = I.begin[i + 1] - s0;
  double Dq[4] = {0, 0, 0, 1}, Ci[9] = {0}, Cdi[9] = {0}, ai[3] = {0}, adi[3] = {0}, cross[9] = {0};
  double dadbg[9] = {0}, dvdbg[9] = {0}, dpdbg[9] = {0};
  static thread_local double dP[4][225], F[225], T1[225], K[4][15];
  for (auto& m : dP) std::fill(m, m + 225, 0.0);
  int64_t time = t_k;
  bool started = false;
  for (int64_t k = 0; k < N; ++k) {
    double om0[3], ac0[3], om1[3], ac1[3];
    const double *g0 = &I.ga[6 * (s0 + k)], *g1 = &I.ga[6 * (s0 + std::min(k + 1, N - 1))];
    for (int j = 0; j < 3; ++j) { om0[j] = g0[j]; ac0[j] = g0[3 + j]; om1[j] = g1[j]; ac1[j] = g1[3 + j]; }
    int64_t nexttime = k + 1 == N ? t_g : I.ts[s0 + k + 1];
    double dt = toSec(nexttime - time);
    if (t_g < nexttime) {
      const double interval = toSec(nexttime - I.ts[s0 + k]);
      nexttime = t_g;
      dt = toSec(nexttime - time);
      const double r = dt / interval;
      for (int j = 0; j < 3; ++j) { om1[j] = (1 - r) * om0[j] + r * om1[j]; ac1[j] = (1 - r) * ac0[j] + r * ac1[j]; }
    }
    if (dt <= 0.0) continue;
    if (!started) {
      started = true;
      const double r = dt / toSec(nexttime - I.ts[s0 + k]);
      for (int j = 0; j < 3; ++j) { om0[j] = r * om0[j] + (1 - r) * om1[j]; ac0[j] = r * ac0[j] + (1 - r) * ac1[j]; }
    }
    double gm = 1, am = 1, w[3], a[3];
    for (int j = 0; j < 3; ++j) {
      if (std::fabs(om0[j]) > I.par[1] || std::fabs(om1[j]) > I.par[1]) gm = 100;
      if (std::fabs(ac0[j]) > I.par[0] || std::fabs(ac1[j]) > I.par[0]) am = 100;
      w[j] = 0.5 * (om0[j] + om1[j]) - sb[3 + j];
      a[j] = 0.5 * (ac0[j] + ac1[j]) - sb[6 + j];
    }
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * 0.5 * dt, sc = sinc(th) * 0.5 * dt;
    const double dq[4] = {sc * w[0], sc * w[1], sc * w[2], std::cos(th)};
    double Dq1[4], C[9], C1[9], CC[9], CCa[3];
    qmul(Dq, dq, Dq1);
    qrot(Dq, C);
    qrot(Dq1, C1);
    for (int e = 0; e < 9; ++e) CC[e] = C[e] + C1[e];
    mul(CC, a, CCa, 3, 3, 1);
    double dp[3], F012[9];
    for (int j = 0; j < 3; ++j) dp[j] = ai[j] * dt + 0.25 * CCa[j] * dt * dt;
    for (int e = 0; e < 9; ++e) F012[e] = -Ci[e] * dt + 0.25 * CC[e] * dt * dt;
    const double wdt[3] = {w[0] * dt, w[1] * dt, w[2] * dt};
    double Jr[9], C1Jr[9], Rinv[9], cross1[9], ax[9], t0[9], X[9], t1[9];
    rightJacobian(wdt, Jr);
    mul(C1, Jr, C1Jr, 3, 3, 3);
    const double n2 = dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3];
    const double dqi[4] = {-dq[0] / n2, -dq[1] / n2, -dq[2] / n2, dq[3] / n2};
    qrot(dqi, Rinv);
    mul(Rinv, cross, cross1, 3, 3, 3);
    for (int e = 0; e < 9; ++e) cross1[e] += Jr[e] * dt;
    crossMx(a, ax);
    mul(C, ax, t0, 3, 3, 3);
    mul(t0, cross, X, 3, 3, 3);
    mul(C1, ax, t0, 3, 3, 3);
    mul(t0, cross1, t1, 3, 3, 3);
    for (int e = 0; e < 9; ++e) X[e] += t1[e];
    double dpg[9];
    for (int e = 0; e < 9; ++e) dpg[e] = dt * dvdbg[e] + 0.25 * dt * dt * X[e];
    {  // F_delta and the four recursions
      std::fill(F, F + 225, 0.0);
      for (int d = 0; d < 15; ++d) F[d * 15 + d] = 1.0;
      double cx[9], half[3] = {0.5 * CCa[0] * dt, 0.5 * CCa[1] * dt, 0.5 * CCa[2] * dt};
      const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      crossMx(dp, cx);
      setBlock(F, 15, 0, 3, cx, -1.0);
      setBlock(F, 15, 0, 6, I3, dt);
      setBlock(F, 15, 0, 9, dpg, 1.0);
      setBlock(F, 15, 0, 12, F012, 1.0);
      setBlock(F, 15, 3, 9, C1, -dt);
      crossMx(half, cx);
      setBlock(F, 15, 6, 3, cx, -1.0);
      setBlock(F, 15, 6, 9, X, 0.5 * dt);
      setBlock(F, 15, 6, 12, CC, -0.5 * dt);
      for (auto& kd : K) std::fill(kd, kd + 15, 0.0);
      for (int d = 0; d < 3; ++d) {
        K[0][3 + d] = gm * dt;
        K[1][d] = 0.5 * dt * dt * dt * am * am * am;
        K[1][6 + d] = am * dt;
        K[2][9 + d] = dt;
        K[3][12 + d] = dt;
      }
      for (int j = 0; j < 4; ++j) {
        mul(F, dP[j], T1, 15, 15, 15);
        mulT(T1, F, dP[j], 15, 15, 15);
        for (int d = 0; d < 15; ++d) dP[j][d * 15 + d] += K[j][d];
      }
    }
    for (int e = 0; e < 9; ++e) {
      Cdi[e] += Ci[e] * dt + 0.25 * CC[e] * dt * dt;
      Ci[e] += 0.5 * CC[e] * dt;
      dadbg[e] += C1Jr[e] * dt;
      dpdbg[e] += dpg[e];
      dvdbg[e] += 0.5 * dt * X[e];
      cross[e] = cross1[e];
    }
    for (int j = 0; j < 3; ++j) { adi[j] += dp[j]; ai[j] += 0.5 * CCa[j] * dt; }
    for (int j = 0; j < 4; ++j) Dq[j] = Dq1[j];
    time = nexttime;
    if (nexttime == t_g) break;
  }
  double P[225];
  const double s2[4] = {I.par[2] * I.par[2], I.par[3] * I.par[3], I.par[4] * I.par[4], I.par[5] * I.par[5]};
  for (int r = 0; r < 15; ++r)
    for (int c = 0; c < 15; ++c) {
      double p = 0.0;
      for (int j = 0; j < 4; ++j) p += (0.5 * dP[j][r * 15 + c] + 0.5 * dP[j][c * 15 + r]) * s2[j];
      P[r * 15 + c] = p;
    }
  // the residual stage (Delta_b = 0 after the redo)
  double q0[4] = {pose[3], pose[4], pose[5], pose[6]}, C0[9], CGW[9], qt[4], Ctg[9];
  qnormalize(q0);
  qrot(q0, C0);
  qrot(G + 3, CGW);
  const double Dt = toSec(t_g - t_k);
  double Cadi[3], rtg[3], aW[3], a0[3];
  mul(C0, adi, Cadi, 3, 3, 1);
  for (int j = 0; j < 3; ++j) rtg[j] = pose[j] + sb[j] * Dt - (j == 2 ? 0.5 * I.par[6] * Dt * Dt : 0.0) + Cadi[j];
  qmul(q0, Dq, qt);
  qnormalize(qt);
  qrot(qt, Ctg);
  mul(Ctg, I.r_SA, aW, 3, 3, 1);
  mul(C0, I.r_SA, a0, 3, 3, 1);
  double Tm[225], TP[225], Pw[225];
  std::fill(Tm, Tm + 225, 0.0);
  for (int d = 0; d < 15; ++d) Tm[d * 15 + d] = 1.0;
  setBlock(Tm, 15, 0, 0, C0, 1.0);
  setBlock(Tm, 15, 3, 3, C0, 1.0);
  setBlock(Tm, 15, 6, 6, C0, 1.0);
  mul(Tm, P, TP, 15, 15, 15);
  mulT(TP, Tm, Pw, 15, 15, 15);
  double Jws[18], X0[9], E0[9], P6[36], JP[18], JPJ[9], Ginv[9], cov[9], W[9], S[9];
  crossMx(a0, X0);
  mul(CGW, X0, E0, 3, 3, 3);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { Jws[r * 6 + c] = CGW[r * 3 + c]; Jws[r * 6 + 3 + c] = -E0[r * 3 + c]; }
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) P6[r * 6 + c] = Pw[r * 15 + c];
  mul(Jws, P6, JP, 3, 6, 6);
  mulT(JP, Jws, JPJ, 3, 6, 3);
  inv3(&I.info[9 * i], Ginv);
  for (int e = 0; e < 9; ++e) cov[e] = Ginv[e] + JPJ[e];
  inv3(cov, W);
  cholU(W, S);
  double pW[3], pG[3], err[3];
  for (int j = 0; j < 3; ++j) pW[j] = rtg[j] + aW[j];
  mul(CGW, pW, pG, 3, 3, 1);
  for (int j = 0; j < 3; ++j) err[j] = I.z[3 * i + j] - (pG[j] + G[j]);
  mul(S, err, out, 3, 3, 1);
  // Jprop and the Jacobians
  double Jprop[225], B[9], cx[9];
  std::fill(Jprop, Jprop + 225, 0.0);
  for (int d = 0; d < 15; ++d) Jprop[d * 15 + d] = 1.0;
  const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  crossMx(Cadi, cx);
  setBlock(Jprop, 15, 0, 3, cx, -1.0);
  setBlock(Jprop, 15, 0, 6, I3, Dt);
  mul(C0, dpdbg, B, 3, 3, 3);
  setBlock(Jprop, 15, 0, 9, B, 1.0);
  mul(C0, Cdi, B, 3, 3, 3);
  setBlock(Jprop, 15, 0, 12, B, -1.0);
  mul(C0, dadbg, B, 3, 3, 3);
  setBlock(Jprop, 15, 3, 9, B, -1.0);
  double Jtg[18], Xa[9], E[9], J66[36], J69[54], Jp[18], Jsb[27], J2[18];
  crossMx(aW, Xa);
  mul(CGW, Xa, E, 3, 3, 3);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { Jtg[r * 6 + c] = -CGW[r * 3 + c]; Jtg[r * 6 + 3 + c] = E[r * 3 + c]; }
  for (int r = 0; r < 6; ++r) {
    for (int c = 0; c < 6; ++c) J66[r * 6 + c] = Jprop[r * 15 + c];
    for (int c = 0; c < 9; ++c) J69[r * 9 + c] = Jprop[r * 15 + 6 + c];
  }
  mul(Jtg, J66, Jp, 3, 6, 6);
  mul(Jtg, J69, Jsb, 3, 6, 9);
  crossMx(pG, cx);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { J2[r * 6 + c] = r == c ? -1.0 : 0.0; J2[r * 6 + 3 + c] = cx[r * 3 + c]; }
  mul(S, Jp, out + 3, 3, 3, 6);
  mul(S, Jsb, out + 21, 3, 3, 9);
  mul(S, J2, out + 48, 3, 3, 6);
}

template <class T>
void readInto(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "gps_port: short input\n"); std::exit(1); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: gps_port <input file> [reps]\n"); return 1; }
  const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "gps_port: cannot open %s\n", argv[1]); return 1; }
  Inputs I;
  std::vector<int64_t> head;
  std::vector<double> par;
  readInto(f, head, 2);
  I.n = head[0];
  I.ns = head[1];
  if (I.n < 0 || I.ns < 0) { std::fprintf(stderr, "gps_port: bad header\n"); return 1; }
  readInto(f, par, 10);
  std::copy(par.begin(), par.begin() + 7, I.par);
  std::copy(par.begin() + 7, par.end(), I.r_SA);
  const size_t n = (size_t)I.n, ns = (size_t)I.ns;
  readInto(f, I.poses, 7 * n);
  readInto(f, I.sb, 9 * n);
  readInto(f, I.gw, 7 * n);
  readInto(f, I.z, 3 * n);
  readInto(f, I.info, 9 * n);
  readInto(f, I.t_k, n);
  readInto(f, I.t_g, n);
  readInto(f, I.begin, n + 1);
  readInto(f, I.ts, ns);
  readInto(f, I.ga, 6 * ns);
  std::fclose(f);
  for (size_t i = 0; i < n; ++i)
    if (I.begin[i] < 0 || I.begin[i + 1] <= I.begin[i] || (size_t)I.begin[i + 1] > ns) {
      std::fprintf(stderr, "gps_port: bad sample_begin\n");
      return 1;
    }
  std::vector<double> out(66 * n), ms;
  for (int r = 0; r < reps; ++r) {
    const auto a = std::chrono::steady_clock::now();
    for (size_t i = 0; i < n; ++i) evaluate(I, (int64_t)i, &out[66 * i]);
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count());
  }
  std::sort(ms.begin(), ms.end());
  double sum_r = 0.0, sum_J = 0.0;
  for (size_t i = 0; i < n; ++i) {
    for (int e = 0; e < 3; ++e) sum_r += out[66 * i + e];
    for (int e = 3; e < 66; ++e) sum_J += out[66 * i + e];
  }
  std::printf("{\"port\": \"single-thread C++ port of tests/_gps_error.py (not the reference)\", \"n\": %lld, \"reps\": %d, "
              "\"ms_median\": %.4f, \"ms_min\": %.4f, \"sum_r\": %.9f, \"sum_J\": %.9f}\n",
              (long long)I.n, reps, ms[ms.size() / 2], ms[0], sum_r, sum_J);
  return 0;
}
