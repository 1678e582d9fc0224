// imu_chain_lane_body.hpp — one step of the lane chain (ImuError.cpp:644-659; ViInterface.cpp:696-715
// is the same text). Not a header: the statement imu_chain.hpp describes, included where it runs, with
// these names in scope:
//   Q Dq, double ai[3], adi[3]   the carried Delta_q, acc_integral, acc_doubleintegral
//   double C[9]                  R(Delta_q): before the step on entry, after it on leaving
//   PropStep s                   the step's inputs
{
  const double dt = s.dt;
  double sh, ch;
  Dq = qmul(Dq, stepDq(s, sh, ch));
  double C1[9], CCa[3];
  qrot(Dq, C1);
#pragma unroll
  for (int e = 0; e < 9; ++e) C[e] += C1[e];
  mv3(C, s.a, CCa);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    adi[j] += ai[j] * dt + 0.25 * CCa[j] * dt * dt;
    ai[j] += 0.5 * CCa[j] * dt;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) C[e] = C1[e];
}
