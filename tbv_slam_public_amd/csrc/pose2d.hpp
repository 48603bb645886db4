// pose2d.hpp -- the planar pose algebra of the registration family (matcher.hip, tieaudit.hip, coral.hip, verify.hip,
// odometry.hip), once: Eigen's Affine product and inverse on a 2 x 2 linear part and a translation, and the same on
// (x, y, theta).  Host and device; plain C++ without __HIPCC__ (tests/cpp/registration_check.cpp).
//
// Every routine has ONE operation order, kept by -ffp-contract=off: the tie audit replays the matcher's transforms bit for
// bit, so both take them from here.  The angle's sine and cosine come from libm -- sincos on the device, std::cos and
// std::sin on the host; a caller with a rotation of its own (the matcher's polynomial sincos) goes through aff_from_cs.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define POSE2D_FN __host__ __device__ __forceinline__
#else
#define POSE2D_FN inline
#endif

struct Aff2 { double l0, l1, l2, l3, t0, t1; };   // [l0 l1; l2 l3] x + (t0, t1)

POSE2D_FN void pose2d_sincos(double th, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(th, s, c);
#else
  *c = std::cos(th); *s = std::sin(th);
#endif
}

POSE2D_FN Aff2 aff_identity() { return Aff2{1, 0, 0, 1, 0, 0}; }
POSE2D_FN Aff2 aff_from_cs(double c, double s, double x, double y) { return Aff2{c, -s, s, c, x, y}; }
// registration.cpp:128-135 vectorToAffine3d + n_scan_normal.cpp:350-351
POSE2D_FN Aff2 aff_from_xyt(const double* p) {
  double s, c;
  pose2d_sincos(p[2], &s, &c);
  return aff_from_cs(c, s, p[0], p[1]);
}
POSE2D_FN Aff2 aff_mul(const Aff2& a, const Aff2& b) {     // Eigen Transform * Transform
  Aff2 r;
  r.l0 = a.l0 * b.l0 + a.l1 * b.l2;
  r.l1 = a.l0 * b.l1 + a.l1 * b.l3;
  r.l2 = a.l2 * b.l0 + a.l3 * b.l2;
  r.l3 = a.l2 * b.l1 + a.l3 * b.l3;
  r.t0 = a.l0 * b.t0 + a.l1 * b.t1 + a.t0;
  r.t1 = a.l2 * b.t0 + a.l3 * b.t1 + a.t1;
  return r;
}
POSE2D_FN Aff2 aff_inv(const Aff2& a) {                    // Eigen Affine inverse: adjugate / det
  const double det = a.l0 * a.l3 - a.l2 * a.l1;
  const double invdet = 1.0 / det;
  Aff2 r;
  r.l0 = a.l3 * invdet; r.l1 = -a.l1 * invdet; r.l2 = -a.l2 * invdet; r.l3 = a.l0 * invdet;
  r.t0 = -(r.l0 * a.t0 + r.l1 * a.t1);
  r.t1 = -(r.l2 * a.t0 + r.l3 * a.t1);
  return r;
}
POSE2D_FN void aff_to_xyt(const Aff2& a, double p[3]) {    // utils.cpp:115-122 Affine3dToVectorXYeZ
  p[0] = a.t0; p[1] = a.t1; p[2] = std::atan2(a.l2, a.l3);
}

// the same algebra on (x, y, theta); o may be a or b
POSE2D_FN void xyt_compose(const double a[3], const double b[3], double o[3]) {      // a * b
  double s, c;
  pose2d_sincos(a[2], &s, &c);
  const double x = c * b[0] - s * b[1] + a[0], y = s * b[0] + c * b[1] + a[1];
  o[0] = x; o[1] = y; o[2] = a[2] + b[2];
}
POSE2D_FN void xyt_inverse(const double a[3], double o[3]) {                         // a^-1
  double s, c;
  pose2d_sincos(a[2], &s, &c);
  const double x = -(c * a[0] + s * a[1]), y = s * a[0] - c * a[1];
  o[0] = x; o[1] = y; o[2] = -a[2];
}

#if defined(__HIPCC__)
// loopclosure::VerifyByOdometry (loopclosure.cpp:783-795) on the device, for closure_odom_kernel (closure.hip) and
// verify_fill_kernel (verify.hip): the motions rel[begin .. end) ([k][3], RelativeMotion(k, k + 1)) composed in order, in
// the arithmetic and order of cfear_verify_by_odometry (verify.hip).  two_sigma2 = 2 sigma^2.
__device__ __forceinline__ double odom_chain_similarity(const double* rel, int begin, int end, double two_sigma2) {
  double T0 = 0.0, T1 = 0.0, T2 = 0.0, trav = 0.0;
  for (int k = begin; k < end; k++) {
    const double d0 = rel[3 * (size_t)k], d1 = rel[3 * (size_t)k + 1], d2 = rel[3 * (size_t)k + 2];
    trav += sqrt(d0 * d0 + d1 * d1);
    const double cs = cos(T2), sn = sin(T2);
    const double x = cs * d0 - sn * d1 + T0, y = sn * d0 + cs * d1 + T1;
    T0 = x; T1 = y; T2 = T2 + d2;
  }
  const double est = sqrt(T0 * T0 + T1 * T1);
  const double over = est - 5.0;
  const double error = over < 0.0 ? 0.0 : over;                 // std::max(over, 0.0): a NaN stays a NaN
  const double r = error / trav;
  return 1.0 - exp(-r * r / two_sigma2);
}
#endif

// AccelerationVelocitySanityCheck (odometrykeyframefuser.cpp:76-94): 4 Hz, 200 m/s and 200 m/s^2, strict comparisons,
// acceleration tested first; only the translations of the two motions enter.  1 = sane, 0 = use the guess (:198-199).
POSE2D_FN int pose2d_acc_vel_sane(const double tmot_prev_xy[2], const double tmot_curr_xy[2]) {
  const double dt = 0.25, vel_limit = 200, acc_limit = 200;
  const double vel = sqrt((tmot_curr_xy[0] / dt) * (tmot_curr_xy[0] / dt) + (tmot_curr_xy[1] / dt) * (tmot_curr_xy[1] / dt));
  const double ax = (tmot_curr_xy[0] - tmot_prev_xy[0]) / (dt * dt), ay = (tmot_curr_xy[1] - tmot_prev_xy[1]) / (dt * dt);
  const double acc = sqrt(ax * ax + ay * ay);
  if (acc > acc_limit) return 0;
  else if (vel > vel_limit) return 0;
  return 1;
}
