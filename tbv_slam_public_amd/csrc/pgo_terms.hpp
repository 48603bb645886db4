// pgo_terms.hpp -- the arithmetic one pose-graph constraint needs, shared by the host solver (pgo.hip) and the batched
// device solver (pgo_batch.hip): PoseGraph3dErrorTerm (tbv_slam/include/tbv_slam/ceresoptimizer.h:62-97) over doubles or
// forward-mode jets, ceres::CauchyLoss, ceres::EigenQuaternionParameterization, and the 6 x 6 Cholesky factor of the scaled
// information.  Every function evaluates the same expressions in the same order on both sides (the library is built with
// -ffp-contract=off), so host and device differ only where a sum is split over lanes and in the last bit of libm calls.
#pragma once
#include <cmath>
#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/cfear_hip.h"

#if defined(__HIPCC__)
#define PGO_HD __host__ __device__
#else
#define PGO_HD
#endif

namespace pgo {

// ---- forward-mode automatic differentiation over N parameters, like ceres::Jet -----------------------------------------
// A derivative component depends only on the same component of the operands, so the 14 derivatives of a residual block
// (p_a 3, q_a 4, p_b 3, q_b 4) may be taken in one pass of JetT<14> or in two of JetT<7>: the values are the same bit for bit.
template <int N> struct JetT {
  double a;
  double v[N];
  PGO_HD JetT() : a(0) { for (int i = 0; i < N; i++) v[i] = 0; }
  PGO_HD JetT(double x) : a(x) { for (int i = 0; i < N; i++) v[i] = 0; }
  PGO_HD JetT(double x, int k) : a(x) { for (int i = 0; i < N; i++) v[i] = i == k ? 1.0 : 0.0; }
};
template <int N> PGO_HD inline JetT<N> operator+(const JetT<N>& x, const JetT<N>& y) { JetT<N> r; r.a = x.a + y.a; for (int i = 0; i < N; i++) r.v[i] = x.v[i] + y.v[i]; return r; }
template <int N> PGO_HD inline JetT<N> operator-(const JetT<N>& x, const JetT<N>& y) { JetT<N> r; r.a = x.a - y.a; for (int i = 0; i < N; i++) r.v[i] = x.v[i] - y.v[i]; return r; }
template <int N> PGO_HD inline JetT<N> operator-(const JetT<N>& x) { JetT<N> r; r.a = -x.a; for (int i = 0; i < N; i++) r.v[i] = -x.v[i]; return r; }
template <int N> PGO_HD inline JetT<N> operator*(const JetT<N>& x, const JetT<N>& y) { JetT<N> r; r.a = x.a * y.a; for (int i = 0; i < N; i++) r.v[i] = x.a * y.v[i] + x.v[i] * y.a; return r; }

template <typename T> struct Quat { T x, y, z, w; };
template <typename T> PGO_HD inline Quat<T> qmul(const Quat<T>& a, const Quat<T>& b) {       // Eigen::Quaternion operator*
  return Quat<T>{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                 a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
template <typename T> PGO_HD inline Quat<T> qconj(const Quat<T>& a) { return Quat<T>{-a.x, -a.y, -a.z, a.w}; }
// Eigen::Quaternion * Vector3: v + 2 w (u x v) + 2 u x (u x v), evaluated as Eigen's _transformVector does
template <typename T> PGO_HD inline void qrot(const Quat<T>& q, const T v[3], T out[3]) {
  const T ux = q.y * v[2] - q.z * v[1], uy = q.z * v[0] - q.x * v[2], uz = q.x * v[1] - q.y * v[0];
  const T two(2.0);
  const T tx = two * ux, ty = two * uy, tz = two * uz;
  out[0] = v[0] + q.w * tx + (q.y * tz - q.z * ty);
  out[1] = v[1] + q.w * ty + (q.z * tx - q.x * tz);
  out[2] = v[2] + q.w * tz + (q.x * ty - q.y * tx);
}

// PoseGraph3dErrorTerm::operator() (ceresoptimizer.h:62-97): residual = L * [p_ab_est - p_ab_meas; 2 vec(q_meas * q_ab_est^-1)]
template <typename T>
PGO_HD inline void error_term(const T pa[3], const Quat<T>& qa, const T pb[3], const Quat<T>& qb, const cfear_pose3d& meas, const double L[36], T r[6]) {
  const Quat<T> qa_inv = qconj(qa);
  const Quat<T> q_ab = qmul(qa_inv, qb);
  const T d[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
  T p_ab[3];
  qrot(qa_inv, d, p_ab);
  const Quat<T> qm{T(meas.q[0]), T(meas.q[1]), T(meas.q[2]), T(meas.q[3])};
  const Quat<T> dq = qmul(qm, qconj(q_ab));
  T e[6] = {p_ab[0] - T(meas.p[0]), p_ab[1] - T(meas.p[1]), p_ab[2] - T(meas.p[2]), T(2.0) * dq.x, T(2.0) * dq.y, T(2.0) * dq.z};
  for (int i = 0; i < 6; i++) {                                  // residuals.applyOnTheLeft(sqrt_information)
    T s(0.0);
    for (int k = 0; k < 6; k++) s = s + T(L[i * 6 + k]) * e[k];
    r[i] = s;
  }
}

// ceres::CauchyLoss(a) at s = |r|^2 (rho, rho'); no loss: (s, 1)
PGO_HD inline void loss(bool cauchy, double cauchy_a, double s, double& rho0, double& rho1) {
  if (!cauchy) { rho0 = s; rho1 = 1.0; return; }
  const double b = cauchy_a * cauchy_a, cc = 1.0 / b, sum = 1.0 + s * cc, inv = 1.0 / sum;
  const double tiny = std::numeric_limits<double>::min();
  rho0 = b * std::log(sum);
  rho1 = tiny < inv ? inv : tiny;                                // std::max(min, inv)
}

// EigenQuaternionParameterization::ComputeJacobian (4 x 3, Eigen coefficient order x, y, z, w)
PGO_HD inline void local_jacobian(const double q[4], double G[12]) {
  G[0] = q[3];  G[1] = q[2];  G[2] = -q[1];
  G[3] = -q[2]; G[4] = q[3];  G[5] = q[0];
  G[6] = q[1];  G[7] = -q[0]; G[8] = q[3];
  G[9] = -q[0]; G[10] = -q[1]; G[11] = -q[2];
}

// x_plus_delta: p += dp; q = exp(dq) * q (ceres::EigenQuaternionParameterization::Plus)
PGO_HD inline void plus(const cfear_pose3d& x, const double d[6], cfear_pose3d& out) {
  for (int k = 0; k < 3; k++) out.p[k] = x.p[k] + d[k];
  const double nd = std::sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
  if (nd > 0.0) {
    const double s = std::sin(nd) / nd;
    const Quat<double> dq{s * d[3], s * d[4], s * d[5], std::cos(nd)}, q{x.q[0], x.q[1], x.q[2], x.q[3]};
    const Quat<double> r = qmul(dq, q);
    out.q[0] = r.x; out.q[1] = r.y; out.q[2] = r.z; out.q[3] = r.w;
  } else {
    for (int k = 0; k < 4; k++) out.q[k] = x.q[k];
  }
}

// lower Cholesky factor of a row-major 6 x 6 matrix; false if a pivot is not positive
PGO_HD inline bool llt6(const double A[36], double L[36]) {
  for (int i = 0; i < 36; i++) L[i] = 0.0;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[i * 6 + j];
      for (int k = 0; k < j; k++) s -= L[i * 6 + k] * L[j * 6 + k];
      if (i == j) { if (!(s > 0.0)) return false; L[i * 6 + i] = std::sqrt(s); }
      else L[i * 6 + j] = s / L[j * 6 + j];
    }
  return true;
}

// ---- host: the residual blocks of one graph ---------------------------------------------------------------------------
// CeresLeastSquares::BuildOptimizationProblem (ceresoptimizer.cpp:64-113): AddConstraintType(odometry), then
// (loop_appearance); mini_loop / candidate constraints are not optimised.  Both solvers take their problem from here, so
// they refuse the same inputs: ids that do not ascend, a constraint on an unknown node, information that is not positive
// definite, and a graph without a residual block (CFEAR_ERR_INVALID_ARGUMENT each).
struct Term {
  int a, b;                              // node indices (0 = the fixed first node)
  int j;                                 // the constraint: constraints[j]
  int l;                                 // its sqrt_information: factors[l]
  bool cauchy;
};
struct Factor { double L[36]; };         // sqrt_information = I_scaled.llt().matrixL(), row-major
// I_scaled of a block of type `pass` (0 odometry, 1 loop_appearance) and its factor; false if it is not positive definite
inline bool scaled_factor(const cfear_pgo_params* par, const cfear_graph_constraint& c, int pass, Factor& f) {
  const double loop_scale_factor = pass == 1 ? 1.0 / par->loop_scaling : 1.0;         // :85
  double I[36] = {0};
  if (par->replace_cov_by_identity) {                                    // :86-88: the odom_* variances scale BOTH types
    const double d[6] = {1.0 / par->odom_vxx, 1.0 / par->odom_vyy, 1, 1, 1, 1.0 / par->odom_vtt};
    for (int t = 0; t < 6; t++) I[t * 7] = d[t] * loop_scale_factor;
  } else {
    for (int t = 0; t < 36; t++) I[t] = c.information[t] * loop_scale_factor;
  }
  return llt6(I, f.L);
}
// With replace_cov_by_identity every odometry block shares factors[0] and every loop block factors[1] (either may be
// absent); otherwise each block has its own.
inline int collect_terms(const uint64_t* ids, int n, const cfear_graph_constraint* constraints, int m, const cfear_pgo_params* par,
                         std::vector<Term>& out, std::vector<Factor>& factors) {
  out.clear();
  factors.clear();
  for (int i = 1; i < n; i++) if (!(ids[i - 1] < ids[i])) return CFEAR_ERR_INVALID_ARGUMENT;   // the node map is ordered by id
  auto find = [&](uint64_t id) { const uint64_t* p = std::lower_bound(ids, ids + n, id); return (p != ids + n && *p == id) ? (int)(p - ids) : -1; };
  for (int pass = 0; pass < 2; pass++) {
    int shared = -1;
    for (int j = 0; j < m; j++) {
      const cfear_graph_constraint& c = constraints[j];
      if (c.type != pass) continue;
      Term k;
      k.a = find(c.id_begin); k.b = find(c.id_end);
      if (k.a < 0 || k.b < 0) return CFEAR_ERR_INVALID_ARGUMENT;         // "Nodes doesn't exist" (:74-75)
      k.j = j;
      k.cauchy = pass == 1;
      if (shared < 0) {
        Factor f;
        if (!scaled_factor(par, c, pass, f)) return CFEAR_ERR_INVALID_ARGUMENT;   // Eigen's llt() of a non-SPD matrix is garbage; refuse
        factors.push_back(f);
        if (par->replace_cov_by_identity) shared = (int)factors.size() - 1;
      }
      k.l = shared >= 0 ? shared : (int)factors.size() - 1;
      out.push_back(k);
    }
  }
  return out.empty() ? CFEAR_ERR_INVALID_ARGUMENT : CFEAR_OK;
}

}  // namespace pgo
