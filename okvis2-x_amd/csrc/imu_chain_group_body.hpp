// imu_chain_group_body.hpp — one step of the group chain (ImuError.cpp:644-682;
// GpsErrorAsynchronous.cpp:402-452 is the same text but for dalpha_db_g). Not a header: the statement
// imu_chain.hpp describes, included where it runs, with these names in scope:
//   Q Dq, double C[9], Ci[9], Cdi[9], cross[9], dadbg[9], dvdbg[9], dpdbg[9], ai[3], adi[3], Dt
//                      the carried state: Delta_q, R(Delta_q), C_integral, C_doubleintegral, cross,
//                      dalpha_db_g, dv_db_g, dp_db_g, acc_integral, acc_doubleintegral, Delta_t
//   PropStep s         the step's inputs
//   double F[kFdt + 1] with COV, receives the step's F_delta (imu_fdelta.hpp), from the sums before the step
//   constexpr bool COV, JR
// JR: dalpha_db_g += C_1 rightJacobian(w dt) dt as redoPreintegration has it
// (GpsErrorAsynchronous.cpp:425); without, dalpha_db_g += dt C_1 as ImuError::propagation has it
// (ImuError.cpp:663).
{
  const double dt = s.dt;
  Dt += dt;
  double sh, ch;
  const Q dq = stepDq(s, sh, ch);
  Dq = qmul(Dq, dq);
  double C1[9], CC[9], CCa[3];
  qrot(Dq, C1);
#pragma unroll
  for (int e = 0; e < 9; ++e) CC[e] = C[e] + C1[e];
  mv3(CC, s.a, CCa);
  // Jacobian parts (:663-668): cross_1 = R(dq)^T cross + rightJacobian(w dt) dt,
  // X = C [a]x cross + C_1 [a]x cross_1
  double X[9], C1Jr[9];
  {
    const double wdt[3] = {s.w[0] * dt, s.w[1] * dt, s.w[2] * dt};
    double Jr[9], Rdqi[9], ax[9], t0[9], t1[9], cross1[9];
    rightJacobianHalf(wdt, sh, ch, Jr);
    if (JR) mm3(C1, Jr, C1Jr);
    qrot(qinv(dq), Rdqi);
    crossMx(s.a, ax);
    mm3(C, ax, t0);
    mm3(t0, cross, X);
    mm3(Rdqi, cross, cross1);
#pragma unroll
    for (int e = 0; e < 9; ++e) cross[e] = cross1[e] + Jr[e] * dt;
    mm3(C1, ax, t0);
    mm3(t0, cross, t1);
#pragma unroll
    for (int e = 0; e < 9; ++e) X[e] += t1[e];
  }
  const double qdt2 = 0.25 * dt * dt;
  // F_delta (:672-682) from the sums before the step, then the sums (:656-668)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double v = ai[j] * dt + qdt2 * CCa[j];
    if (COV) {
      F[kF03 + j] = v;                  // F03 = -[acc_integral dt + dt^2/4 (C + C_1) a]x, held as its vector
      F[kF63 + j] = 0.5 * dt * CCa[j];  // F63 = -[dt/2 (C + C_1) a]x
    }
    adi[j] += v;
    ai[j] += 0.5 * CCa[j] * dt;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const double p = dt * dvdbg[e] + qdt2 * X[e];
    if (COV) {
      F[kF09 + e] = p;
      F[kF012 + e] = -Ci[e] * dt + qdt2 * CC[e];
      F[kF39 + e] = -dt * C1[e];
      F[kF69 + e] = 0.5 * dt * X[e];
      F[kF612 + e] = -0.5 * dt * CC[e];
    }
    Cdi[e] += Ci[e] * dt + qdt2 * CC[e];
    Ci[e] += 0.5 * dt * CC[e];
    if (JR) dadbg[e] += C1Jr[e] * dt;
    else dadbg[e] += dt * C1[e];
    dpdbg[e] += p;
    dvdbg[e] += 0.5 * dt * X[e];
    C[e] = C1[e];
  }
  if (COV) F[kFdt] = dt;
}
