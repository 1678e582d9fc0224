// lidar_port.cpp — a stand-alone single-thread C++ port of the serial LiDAR pre-processing that
// okvisgpu_lidar_deskew and okvisgpu_voxel_downsample replace: one propagator per scan with a persistent
// sample cursor, advanced point by point, carrying the attitude increment, both acceleration integrals
// and the bias-sensitivity matrices (which the serial loop computes for every point although the
// deskewing multiplies them by a zero bias change), then the transform of each ray into the live
// frame; and a first-point-per-voxel filter over a hash map. It is the CPU figure of
// scripts/lidar_timing.py: the port on this host, not the reference (which needs Eigen and is not
// buildable here). Own 3x3 arithmetic, no dependency.
//   g++ -O3 -std=c++17 scripts/lidar_port.cpp -o scripts/lidar_port        (timing)
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 scripts/lidar_port.cpp -o lidar_port_san  (checks)
// Usage: lidar_port [queries [samples [reps]]]   -> one JSON line
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

namespace {

struct V3 {
  double x, y, z;
};
struct M3 {
  double m[9];
};
struct Quat {
  double x, y, z, w;
};
struct Pose {
  V3 r;
  Quat q;
};

V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
double norm(V3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
M3 zero3() { return M3{{0, 0, 0, 0, 0, 0, 0, 0, 0}}; }
M3 operator+(const M3& a, const M3& b) {
  M3 c;
  for (int i = 0; i < 9; ++i) c.m[i] = a.m[i] + b.m[i];
  return c;
}
M3 operator*(double s, const M3& a) {
  M3 c;
  for (int i = 0; i < 9; ++i) c.m[i] = s * a.m[i];
  return c;
}
M3 operator*(const M3& a, const M3& b) {
  M3 c;
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) c.m[3 * r + k] = a.m[3 * r] * b.m[k] + a.m[3 * r + 1] * b.m[3 + k] + a.m[3 * r + 2] * b.m[6 + k];
  return c;
}
V3 operator*(const M3& a, V3 v) {
  return {a.m[0] * v.x + a.m[1] * v.y + a.m[2] * v.z, a.m[3] * v.x + a.m[4] * v.y + a.m[5] * v.z,
          a.m[6] * v.x + a.m[7] * v.y + a.m[8] * v.z};
}
M3 transpose(const M3& a) { return M3{{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}}; }
M3 skew(V3 v) { return M3{{0, -v.z, v.y, v.z, 0, -v.x, -v.y, v.x, 0}}; }
Quat operator*(Quat a, Quat b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
          a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
Quat unit(Quat q) {
  const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return {q.x / n, q.y / n, q.z / n, q.w / n};
}
M3 rotation(Quat q) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  return M3{{1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
             1 - (txx + tyy)}};
}
double sincSeries(double x) {
  if (std::fabs(x) > 1e-6) return std::sin(x) / x;
  const double x2 = x * x;
  return 1.0 - x2 / 6.0 + x2 * x2 / 120.0 - x2 * x2 * x2 / 5040.0;
}
M3 rightJacobian(V3 p) {
  const double phi = norm(p);
  const M3 X = skew(p), X2 = X * X;
  double a = -0.5, b = 1.0 / 6.0;
  if (phi >= 1e-4) {
    a = -(1.0 - std::cos(phi)) / (phi * phi);
    b = (phi - std::sin(phi)) / (phi * phi * phi);
  }
  M3 J = a * X + b * X2;
  J.m[0] += 1.0; J.m[4] += 1.0; J.m[8] += 1.0;
  return J;
}
double seconds(int64_t ns) {
  int64_t s = ns / 1000000000LL, n = ns % 1000000000LL;
  if (n < 0) { n += 1000000000LL; s -= 1; }
  return (double)s + 1e-9 * (double)n;
}

struct Sample {
  int64_t t;
  V3 gyr, acc;
};

// The serial propagator: the committed state, the state interpolated to the last query, the cursor.
struct Propagator {
  struct State {
    Quat dq{0, 0, 0, 1};
    M3 Ci = zero3(), Cdi = zero3(), cross = zero3(), dalpha = zero3(), dv = zero3(), dp = zero3();
    V3 ai{0, 0, 0}, adi{0, 0, 0}, omega{0, 0, 0};
  };
  State done, at;
  const std::vector<Sample>& imu;
  size_t cursor = 0;
  int64_t tStart, tDone;
  double span = 0.0;
  Propagator(int64_t t0, const std::vector<Sample>& s) : imu(s), tStart(t0), tDone(t0) {}

  bool advanceTo(V3 bg, V3 ba, int64_t T) {
    if (!(imu.back().t >= T)) return false;
    int64_t time = tDone;
    bool started = false;
    for (; cursor + 1 < imu.size(); ++cursor) {
      const Sample &s0 = imu[cursor], &s1 = imu[cursor + 1];
      V3 w0 = s0.gyr, a0 = s0.acc, w1 = s1.gyr, a1 = s1.acc;
      int64_t next = s1.t;
      double dt = seconds(next - time);
      if (T < next) {
        const double interval = seconds(next - s0.t);
        next = T;
        dt = seconds(next - time);
        const double r = dt / interval;
        w1 = (1.0 - r) * w0 + r * w1;
        a1 = (1.0 - r) * a0 + r * a1;
      }
      if (dt <= 0.0) continue;
      if (!started) {
        started = true;
        const double r = dt / seconds(next - s0.t);
        w0 = r * w0 + (1.0 - r) * w1;
        a0 = r * a0 + (1.0 - r) * a1;
      }
      const V3 w = 0.5 * (w0 + w1) - bg, a = 0.5 * (a0 + a1) - ba;
      const double half = norm(w) * 0.5 * dt;
      const V3 v = (sincSeries(half) * 0.5 * dt) * w;
      const Quat step{v.x, v.y, v.z, std::cos(half)};
      State n;
      n.dq = done.dq * step;
      const M3 C = rotation(done.dq), C1 = rotation(n.dq), CC = C + C1;
      n.Ci = done.Ci + (0.5 * dt) * CC;
      n.ai = done.ai + (0.5 * dt) * (CC * a);
      n.Cdi = done.Cdi + dt * done.Ci + (0.25 * dt * dt) * CC;
      n.adi = done.adi + dt * done.ai + (0.25 * dt * dt) * (CC * a);
      n.dalpha = done.dalpha + dt * C1;
      n.cross = transpose(rotation(step)) * done.cross + dt * rightJacobian(dt * w);
      const M3 ax = skew(a), X = C * ax * done.cross + C1 * ax * n.cross;
      n.dv = done.dv + (0.5 * dt) * X;
      n.dp = done.dp + dt * done.dv + (0.25 * dt * dt) * X;
      n.omega = w;
      if (next == T) {
        at = n;
        break;
      }
      done = n;
      time = next;
      tDone = next;
    }
    span = seconds(T - tStart);
    return true;
  }

  // pose, speed and rate at the last query; db = the bias change since the reference biases (zero here)
  void state(const Pose& T0, V3 v0, V3 dbg, V3 dba, double g, Pose& T1, V3& v1, V3& omega) const {
    const V3 gW{0, 0, g};
    const Quat q0 = unit(T0.q);
    const M3 C0 = rotation(q0);
    const V3 corr = (-1.0) * (at.dalpha * dbg);
    const double h = 0.5 * norm(corr);
    const V3 cv = (sincSeries(h) * 0.5) * corr;
    const Quat dq = Quat{cv.x, cv.y, cv.z, std::cos(h)} * at.dq;
    T1.r = (T0.r + span * v0 - (0.5 * span * span) * gW) + C0 * (at.adi + at.dp * dbg - at.Cdi * dba);
    T1.q = unit(q0 * dq);
    v1 = (v0 - span * gW) + C0 * (at.ai + at.dv * dbg - at.Ci * dba);
    omega = at.omega;
  }
};

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
  double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct VoxelKey {
  int32_t x, y, z;
  bool operator==(const VoxelKey& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct VoxelKeyHash {
  size_t operator()(const VoxelKey& k) const {
    return (size_t)((uint32_t)k.x * 73856093u ^ (uint32_t)k.y * 19349669u ^ (uint32_t)k.z * 83492791u);
  }
};

double medianMs(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

}  // namespace

int main(int argc, char** argv) {
  const int nq = argc > 1 ? std::atoi(argv[1]) : 65536, ns = argc > 2 ? std::atoi(argv[2]) : 41;
  const int reps = argc > 3 ? std::atoi(argv[3]) : 11;
  if (nq < 1 || ns < 2 || reps < 1) return 2;
  Rng rng{20261020};
  const int64_t rate = 5000000, base = 1000000000;
  std::vector<Sample> imu((size_t)ns);
  for (int k = 0; k < ns; ++k)
    imu[(size_t)k] = {base + k * rate,
                      {rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1)},
                      {rng.uniform(-2, 2), rng.uniform(-2, 2), 9.81 + rng.uniform(-2, 2)}};
  const int64_t t0 = base + 777, span = (ns - 1) * rate - 777;
  std::vector<int64_t> qt((size_t)nq);
  std::vector<V3> ray((size_t)nq);
  for (int i = 0; i < nq; ++i) {
    qt[(size_t)i] = t0 + 1 + (int64_t)((double)(span - 1) * (double)i / (double)nq);
    ray[(size_t)i] = {rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-50, 50)};
  }
  auto pose = [&](double reach) {
    return Pose{{rng.uniform(-reach, reach), rng.uniform(-reach, reach), rng.uniform(-reach, reach)},
                unit({rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.1, 1)})};
  };
  const Pose T0 = pose(300), live = pose(300), TSL = pose(0.5);
  const V3 v0{rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-2, 2)};
  const V3 bg{0.01, -0.02, 0.005}, ba{0.05, -0.02, 0.1};

  std::vector<float> cloud(3 * (size_t)nq);
  std::vector<double> deskewMs, voxelMs;
  double checksum = 0.0;
  size_t kept = 0;
  for (int rep = 0; rep < reps; ++rep) {
    auto a = std::chrono::steady_clock::now();
    {
      Propagator p(t0, imu);
      const M3 Clive = transpose(rotation(unit(live.q))), CSL = rotation(unit(TSL.q));
      for (int i = 0; i < nq; ++i) {
        if (!p.advanceTo(bg, ba, qt[(size_t)i])) continue;
        Pose T1;
        V3 v1, om;
        p.state(T0, v0, {0, 0, 0}, {0, 0, 0}, 9.81, T1, v1, om);
        const V3 pS = CSL * ray[(size_t)i] + TSL.r, pW = rotation(T1.q) * pS + T1.r, pl = Clive * (pW - live.r);
        cloud[3 * (size_t)i] = (float)pl.x;
        cloud[3 * (size_t)i + 1] = (float)pl.y;
        cloud[3 * (size_t)i + 2] = (float)pl.z;
      }
    }
    auto b = std::chrono::steady_clock::now();
    {
      const float vs = (float)0.05;
      std::unordered_map<VoxelKey, int32_t, VoxelKeyHash> grid;
      grid.reserve((size_t)nq);
      for (int i = 0; i < nq; ++i) {
        const float qx = cloud[3 * (size_t)i] / vs, qy = cloud[3 * (size_t)i + 1] / vs, qz = cloud[3 * (size_t)i + 2] / vs;
        auto in = [](float q) { return q >= -2147483648.0f && q < 2147483648.0f; };
        if (!(in(qx) && in(qy) && in(qz))) continue;
        grid.emplace(VoxelKey{(int32_t)qx, (int32_t)qy, (int32_t)qz}, i);
      }
      kept = grid.size();
    }
    auto c = std::chrono::steady_clock::now();
    deskewMs.push_back(std::chrono::duration<double, std::milli>(b - a).count());
    voxelMs.push_back(std::chrono::duration<double, std::milli>(c - b).count());
    checksum += cloud[0] + cloud[3 * (size_t)nq - 1];
  }
  std::printf("{\"port\": \"single-thread C++ port of the serial loop (not the reference)\", \"queries\": %d, "
              "\"samples\": %d, \"reps\": %d, \"deskew_ms_median\": %.4f, \"voxel_ms_median\": %.4f, \"kept\": %zu, "
              "\"checksum\": %.6f}\n",
              nq, ns, reps, medianMs(deskewMs), medianMs(voxelMs), kept, checksum);
  return 0;
}
