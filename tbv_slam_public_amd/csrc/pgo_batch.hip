// pgo_batch.hip -- cfear_pgo_solve_batch: many independent pose graphs, one wavefront each (gfx950, wave64, fp64).
//
// One solve is a serial chain (pgo.hip); a batch of them is not.  pgo_batch_kernel runs the WHOLE Levenberg-Marquardt loop of
// cfear_pgo_solve for one graph in one wavefront, the way matcher_kernel runs a registration: every decision of the host
// solver (trust-region bookkeeping, the three tolerances, the invalid-step counter, the chain preconditioner with its
// block-diagonal fall-back, the conjugate-gradient exit tests) is restated here statement for statement, and the scalars
// that steer it are uniform across the wavefront.  What the lanes share:
//   * residual blocks: one constraint per lane and pass; Jacobians by the jets of pgo_terms.hpp, seven derivatives at a time;
//   * node sums (gradient, column norms, J^T (J v), the 6 x 6 blocks of the normal equations): one node per lane, gathered
//     through a node -> (constraint, side) index the host builds once, in constraint order -- the host solver's order;
//   * the chain preconditioner: lanes 0 .. 5 hold one row (column, on the way back) of each 6 x 6 step, the values that
//     cross lanes travel by v_readlane, and the next node's blocks are loaded while this node's are used;
//   * scalars (cost, dot products, norms): per-lane partial sums over a lane-strided index, then a 6-step xor butterfly.
// No atomics anywhere: every sum has an order fixed by the graph alone, so a graph's result does not depend on its
// position in the batch, on the other graphs, or on the chunking.
//
// Per-constraint state (6 x 12 Jacobian, residuals, J v) is stored constraint-minor ([row][column][constraint]) so that
// the lanes of a pass touch neighbouring addresses.  At ~1.9 KB per node a batch does not fit at once: the host walks
// the graphs in chunks under kPgoBudget bytes (CFEAR_OPT_PGO_GRAPH_CHUNK caps a chunk's graphs for the tests).
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "pgo_terms.hpp"

namespace {

constexpr int kPgoThreads = CFEAR_WAVE;                  // one wavefront per graph
constexpr size_t kPgoBudget = (size_t)8 << 30;           // device bytes one chunk may take

struct PgoGraph {
  int64_t node0, con0;       // first node / first residual block of the graph in the chunk's arrays
  int64_t ptr0;              // first entry of its node -> block index table (n + 1 entries)
  int32_t n, m;              // nodes; residual blocks (odometry first, then loops)
  int32_t n_odom, pad;       // blocks [n_odom, m) carry the Cauchy loss
};

struct PgoArgs {
  const PgoGraph* graphs;
  cfear_pose3d* x;           // [nodes] in: the initial poses; out: the solution
  cfear_pose3d* cand;        // [nodes]
  const int32_t *ca, *cb, *lidx;   // [blocks] node a, node b, row of `factors`
  const cfear_pose3d* meas;        // [blocks]
  const double* factors;           // [][36] sqrt_information
  const int32_t* nc_ptr;           // per graph [n + 1]: node i's entries are nc_idx[2 con0 + nc_ptr[i] .. nc_ptr[i + 1])
  const int32_t* nc_idx;           // [2 blocks] block << 1 | side (0 = the node is the block's a, 1 = its b), ascending
  double *res, *J, *t;             // [6][m], [6][12][m], [6][m] per graph, at 6 con0, 72 con0, 6 con0
  double *scale, *diag, *gs, *y, *r, *z, *p, *Ap;   // [nodes][6]
  double *Ld, *Lo;                 // [nodes][36] diagonal and sub-diagonal blocks: H, then its Cholesky factor
  cfear_pgo_summary* summaries;    // [graphs of the chunk]
  double cauchy_a;
  int32_t max_iter, pad;
};

// ---- wavefront helpers (a lane's value, uniform: readlane_f64, common.hpp) ---------------------------------------------
// Not common.hpp's wave_sum_f64 nor logreg.hip's sum: the order of the additions differs, so the rounding does.
__device__ inline double wave_sum_xor32_to_1(double v) {         // the same bits in every lane: a + b == b + a at every level
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ inline double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// the wavefront's view of its graph
struct G {
  int n, m, n_odom, lane;
  cfear_pose3d *x, *cand;
  const int32_t *ca, *cb, *lidx, *nc_ptr, *nc_idx;
  const cfear_pose3d* meas;
  const double* factors;
  double *res, *J, *t, *scale, *diag, *gs, *y, *r, *z, *p, *Ap, *Ld, *Lo;
  double cauchy_a;
  __device__ double& Jat(int c, int i, int k) const { return J[(size_t)(i * 12 + k) * m + c]; }
};

// derivatives of one block's residuals with respect to the seven parameters of node a (SIDE 0) or node b (SIDE 1)
template <int SIDE>
__device__ inline void block_half(const cfear_pose3d& A, const cfear_pose3d& B, const cfear_pose3d& meas, const double* L, double val[6],
                                  double d[6][6]) {
  using Jet = pgo::JetT<7>;
  const cfear_pose3d& V = SIDE == 0 ? A : B;
  const Jet vp[3] = {Jet(V.p[0], 0), Jet(V.p[1], 1), Jet(V.p[2], 2)};
  const pgo::Quat<Jet> vq{Jet(V.q[0], 3), Jet(V.q[1], 4), Jet(V.q[2], 5), Jet(V.q[3], 6)};
  const cfear_pose3d& C = SIDE == 0 ? B : A;
  const Jet cp[3] = {Jet(C.p[0]), Jet(C.p[1]), Jet(C.p[2])};
  const pgo::Quat<Jet> cq{Jet(C.q[0]), Jet(C.q[1]), Jet(C.q[2]), Jet(C.q[3])};
  Jet r[6];
  if (SIDE == 0) pgo::error_term<Jet>(vp, vq, cp, cq, meas, L, r);
  else pgo::error_term<Jet>(cp, cq, vp, vq, meas, L, r);
  double Gm[12];
  pgo::local_jacobian(V.q, Gm);
  for (int i = 0; i < 6; i++) {
    val[i] = r[i].a;
    for (int k = 0; k < 3; k++) d[i][k] = r[i].v[k];
    for (int k = 0; k < 3; k++) {
      double s = 0;
      for (int t = 0; t < 4; t++) s += r[i].v[3 + t] * Gm[t * 3 + k];
      d[i][3 + k] = s;
    }
  }
}

// Problem::evaluate: the cost at pts; with_jac: also the robustified residuals and the (unscaled) Jacobians
__device__ double evaluate(const G& g, const cfear_pose3d* pts, bool with_jac) {
  double cost = 0.0;
  for (int c = g.lane; c < g.m; c += kPgoThreads) {
    const cfear_pose3d A = pts[g.ca[c]], B = pts[g.cb[c]], meas = g.meas[c];
    const double* L = g.factors + (size_t)36 * g.lidx[c];
    const bool cauchy = c >= g.n_odom;
    double rho0, rho1;
    if (!with_jac) {
      const pgo::Quat<double> qa{A.q[0], A.q[1], A.q[2], A.q[3]}, qb{B.q[0], B.q[1], B.q[2], B.q[3]};
      double r[6];
      pgo::error_term<double>(A.p, qa, B.p, qb, meas, L, r);
      double s = 0;
      for (int i = 0; i < 6; i++) s += r[i] * r[i];
      pgo::loss(cauchy, g.cauchy_a, s, rho0, rho1);
      cost += 0.5 * rho0;
      continue;
    }
    double val[6], d[6][6];
    block_half<0>(A, B, meas, L, val, d);
    double s = 0;
    for (int i = 0; i < 6; i++) s += val[i] * val[i];
    pgo::loss(cauchy, g.cauchy_a, s, rho0, rho1);
    cost += 0.5 * rho0;
    const double sr = std::sqrt(rho1);                           // Corrector, alpha = 0 (rho'' <= 0 for Cauchy)
    for (int i = 0; i < 6; i++) {
      g.res[(size_t)i * g.m + c] = val[i] * sr;
      for (int k = 0; k < 6; k++) g.Jat(c, i, k) = d[i][k] * sr;
    }
    block_half<1>(A, B, meas, L, val, d);
    for (int i = 0; i < 6; i++)
      for (int k = 0; k < 6; k++) g.Jat(c, i, 6 + k) = d[i][k] * sr;
  }
  __syncthreads();
  return wave_sum_xor32_to_1(cost);
}

// out[node][k] = sum over the node's blocks of sum_i J[i][side 6 + k] * w_i, w = J itself (column norms) or the residuals
template <bool NORMS>
__device__ void node_sums(const G& g, double* out) {
  for (int nd = g.lane; nd < g.n; nd += kPgoThreads) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int e = g.nc_ptr[nd]; e < g.nc_ptr[nd + 1]; e++) {
      const int c = g.nc_idx[e] >> 1, off = (g.nc_idx[e] & 1) * 6;
      for (int i = 0; i < 6; i++) {
        const double w = NORMS ? 0.0 : g.res[(size_t)i * g.m + c];
        for (int k = 0; k < 6; k++) { const double j = g.Jat(c, i, off + k); acc[k] += j * (NORMS ? j : w); }
      }
    }
    for (int k = 0; k < 6; k++) out[(size_t)6 * nd + k] = acc[k];
  }
  __syncthreads();
}
__device__ void gradient(const G& g, double* out) {              // J^T r, the constant first node zeroed
  node_sums<false>(g, out);
  if (g.lane < 6) out[g.lane] = 0.0;
  __syncthreads();
}
__device__ void scale_columns(const G& g) {
  for (int c = g.lane; c < g.m; c += kPgoThreads) {
    const int a = g.ca[c], b = g.cb[c];
    for (int k = 0; k < 6; k++) {
      const double sa = a == 0 ? 0.0 : g.scale[(size_t)6 * a + k], sb = b == 0 ? 0.0 : g.scale[(size_t)6 * b + k];
      for (int i = 0; i < 6; i++) { g.Jat(c, i, k) *= sa; g.Jat(c, i, 6 + k) *= sb; }
    }
  }
  __syncthreads();
}
// t = J (sign v)
__device__ void Jv(const G& g, const double* v, double sign) {
  for (int c = g.lane; c < g.m; c += kPgoThreads) {
    const int a = g.ca[c], b = g.cb[c];
    double va[6], vb[6];
    for (int k = 0; k < 6; k++) { va[k] = sign * v[(size_t)6 * a + k]; vb[k] = sign * v[(size_t)6 * b + k]; }
    for (int i = 0; i < 6; i++) {
      double s = 0;
      for (int k = 0; k < 6; k++) s += g.Jat(c, i, k) * va[k] + g.Jat(c, i, 6 + k) * vb[k];
      g.t[(size_t)i * g.m + c] = s;
    }
  }
  __syncthreads();
}
// out = (J^T J + D^2) v on nodes 1 .. n-1
__device__ void JtJv(const G& g, const double* v, double radius, double* out) {
  Jv(g, v, 1.0);
  for (int nd = g.lane; nd < g.n; nd += kPgoThreads) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int e = g.nc_ptr[nd]; e < g.nc_ptr[nd + 1]; e++) {
      const int c = g.nc_idx[e] >> 1, off = (g.nc_idx[e] & 1) * 6;
      for (int i = 0; i < 6; i++) {
        const double w = g.t[(size_t)i * g.m + c];
        for (int k = 0; k < 6; k++) acc[k] += g.Jat(c, i, off + k) * w;
      }
    }
    for (int k = 0; k < 6; k++) {
      const size_t q = (size_t)6 * nd + k;
      out[q] = nd == 0 ? 0.0 : acc[k] + g.diag[q] / radius * v[q];
    }
  }
  __syncthreads();
}
__device__ double dot(const G& g, const double* a, const double* b) {
  double s = 0;
  for (int k = g.lane; k < 6 * g.n; k += kPgoThreads) s += a[k] * b[k];
  return wave_sum_xor32_to_1(s);
}

// ChainPrecond::build, first half: H(i, i) into Ld and H(i, i-1) into Lo, node by node
__device__ void assemble_blocks(const G& g, double radius, bool with_chain) {
  for (int nd = 1 + g.lane; nd < g.n; nd += kPgoThreads) {
    double D[36], E[36];
    for (int q = 0; q < 36; q++) { D[q] = 0.0; E[q] = 0.0; }
    for (int e = g.nc_ptr[nd]; e < g.nc_ptr[nd + 1]; e++) {
      const int c = g.nc_idx[e] >> 1, side = g.nc_idx[e] & 1, off = side * 6;
      const int other = side ? g.ca[c] : g.cb[c];
      const bool chain = with_chain && other == nd - 1;
      double Jn[6][6], Jo[6][6];                                   // the block's columns of this node and of the other one
      for (int i = 0; i < 6; i++)
        for (int k = 0; k < 6; k++) { Jn[i][k] = g.Jat(c, i, off + k); Jo[i][k] = chain ? g.Jat(c, i, 6 - off + k) : 0.0; }
      for (int r = 0; r < 6; r++)
        for (int q = 0; q < 6; q++) {
          double sd = 0, se = 0;
          for (int i = 0; i < 6; i++) sd += Jn[i][r] * Jn[i][q];
          D[r * 6 + q] += sd;
          if (chain) {                                             // H(nd, nd - 1)[r][q] = sum_i J[i][nd's column r] * J[i][(nd - 1)'s column q]
            for (int i = 0; i < 6; i++) se += Jn[i][r] * Jo[i][q];
            E[r * 6 + q] += se;
          }
        }
    }
    for (int k = 0; k < 6; k++) D[k * 7] += g.diag[(size_t)6 * nd + k] / radius;
    for (int q = 0; q < 36; q++) { g.Ld[(size_t)36 * nd + q] = D[q]; g.Lo[(size_t)36 * nd + q] = E[q]; }
  }
  __syncthreads();
}

// ChainPrecond::build, second half: the block-tridiagonal Cholesky factor in place.  Lane r < 6 owns row r of the blocks.
__device__ bool factor_chain(const G& g, bool with_chain) {
  const int r = g.lane < 6 ? g.lane : 5;
  double Lp[6] = {0, 0, 0, 0, 0, 0};                              // row r of the previous diagonal factor
  bool ok = true;
  for (int nd = 1; nd < g.n; nd++) {
    double S[6], X[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 6; q++) S[q] = g.Ld[(size_t)36 * nd + r * 6 + q];
    if (nd > 1 && with_chain) {
      // Lo = E Lp^-T (row r by forward substitution); S -= Lo Lo^T
      for (int q = 0; q < 6; q++) {
        double s = g.Lo[(size_t)36 * nd + r * 6 + q];
        for (int k = 0; k < q; k++) s -= X[k] * readlane_f64(Lp[k], q);
        X[q] = s / readlane_f64(Lp[q], q);
      }
      for (int q = 0; q < 6; q++) {
        double s = 0;
        for (int k = 0; k < 6; k++) s += X[k] * readlane_f64(X[k], q);
        S[q] -= s;
      }
    }
    // llt6, column by column: lane j has the pivot, the lanes below it their entry of column j
    double Lr[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 6; j++) {
      double s = S[j];
      for (int k = 0; k < j; k++) s -= Lr[k] * readlane_f64(Lr[k], j);
      const double piv = readlane_f64(s, j);
      if (!(piv > 0.0)) { ok = false; break; }
      const double dj = std::sqrt(piv);
      Lr[j] = r == j ? dj : (r > j ? s / dj : 0.0);
    }
    if (!ok) break;
    if (g.lane < 6)
      for (int q = 0; q < 6; q++) { g.Ld[(size_t)36 * nd + r * 6 + q] = Lr[q]; g.Lo[(size_t)36 * nd + r * 6 + q] = X[q]; }
    for (int q = 0; q < 6; q++) Lp[q] = Lr[q];
  }
  __syncthreads();
  return ok;
}

// ChainPrecond::apply: z = M^-1 r.  Lanes 0 .. 5 hold row k (forward) or column k (backward) of the step.
__device__ void precond_apply(const G& g, const double* rv, double* z) {
  const int k = g.lane < 6 ? g.lane : 5, n = g.n;
  if (g.lane < 6) z[g.lane] = 0.0;
  double zu[6] = {0, 0, 0, 0, 0, 0};                               // the neighbouring node's solution, uniform
  double lo[6] = {0, 0, 0, 0, 0, 0}, ld[6] = {1, 1, 1, 1, 1, 1}, rhs = 0.0, lo_n[6] = {0, 0, 0, 0, 0, 0}, ld_n[6] = {1, 1, 1, 1, 1, 1}, rhs_n = 0.0;
  auto load_rows = [&](int nd, double* a, double* b, double& c) {
    for (int t = 0; t < 6; t++) { a[t] = g.Lo[(size_t)36 * nd + k * 6 + t]; b[t] = g.Ld[(size_t)36 * nd + k * 6 + t]; }
    c = rv[(size_t)6 * nd + k];
  };
  if (n > 1) load_rows(1, lo, ld, rhs);
  for (int nd = 1; nd < n; nd++) {                                 // forward: L y = r
    if (nd + 1 < n) load_rows(nd + 1, lo_n, ld_n, rhs_n);
    if (nd > 1) for (int t = 0; t < 6; t++) rhs -= lo[t] * zu[t];
    double mine = 0.0;
    for (int kk = 0; kk < 6; kk++) {
      double s = rhs;
      for (int t = 0; t < kk; t++) s -= ld[t] * zu[t];
      s /= ld[kk];
      zu[kk] = readlane_f64(s, kk);
      if (k == kk) mine = s;
    }
    if (g.lane < 6) z[(size_t)6 * nd + k] = mine;
    for (int t = 0; t < 6; t++) { lo[t] = lo_n[t]; ld[t] = ld_n[t]; }
    rhs = rhs_n;
  }
  __syncthreads();
  double dg = 1.0, dg_n = 1.0;
  auto load_cols = [&](int nd, double* a, double* b, double& d, double& c) {
    for (int t = 0; t < 6; t++) {
      a[t] = nd + 1 < n ? g.Lo[(size_t)36 * (nd + 1) + t * 6 + k] : 0.0;
      b[t] = g.Ld[(size_t)36 * nd + t * 6 + k];
    }
    d = g.Ld[(size_t)36 * nd + k * 7];
    c = z[(size_t)6 * nd + k];
  };
  if (n > 1) load_cols(n - 1, lo, ld, dg, rhs);
  for (int nd = n - 1; nd >= 1; nd--) {                            // backward: L^T x = y
    if (nd > 1) load_cols(nd - 1, lo_n, ld_n, dg_n, rhs_n);
    if (nd + 1 < n) for (int t = 0; t < 6; t++) rhs -= lo[t] * zu[t];
    double mine = 0.0;
    for (int kk = 5; kk >= 0; kk--) {
      double s = rhs;
      for (int t = kk + 1; t < 6; t++) s -= ld[t] * zu[t];
      s /= dg;
      zu[kk] = readlane_f64(s, kk);
      if (k == kk) mine = s;
    }
    if (g.lane < 6) z[(size_t)6 * nd + k] = mine;
    for (int t = 0; t < 6; t++) { lo[t] = lo_n[t]; ld[t] = ld_n[t]; }
    dg = dg_n;
    rhs = rhs_n;
  }
  __syncthreads();
}

__device__ double x_norm_of(const G& g) {
  double s = 0;
  for (int i = 1 + g.lane; i < g.n; i += kPgoThreads) {
    for (int k = 0; k < 3; k++) s += g.x[i].p[k] * g.x[i].p[k];
    for (int k = 0; k < 4; k++) s += g.x[i].q[k] * g.x[i].q[k];
  }
  return std::sqrt(wave_sum_xor32_to_1(s));
}
__device__ double max_abs(const G& g, const double* v) {
  double m = 0;
  for (int k = g.lane; k < 6 * g.n; k += kPgoThreads) m = fmax(m, std::fabs(v[k]));
  return wave_max(m);
}

__global__ __launch_bounds__(kPgoThreads) void pgo_batch_kernel(PgoArgs a) {
  const PgoGraph gr = a.graphs[blockIdx.x];
  G g;
  g.n = gr.n; g.m = gr.m; g.n_odom = gr.n_odom; g.lane = threadIdx.x;
  g.x = a.x + gr.node0; g.cand = a.cand + gr.node0;
  g.ca = a.ca + gr.con0; g.cb = a.cb + gr.con0; g.lidx = a.lidx + gr.con0; g.meas = a.meas + gr.con0;
  g.nc_ptr = a.nc_ptr + gr.ptr0; g.nc_idx = a.nc_idx + 2 * gr.con0;
  g.factors = a.factors;
  g.res = a.res + 6 * gr.con0; g.J = a.J + 72 * gr.con0; g.t = a.t + 6 * gr.con0;
  g.scale = a.scale + 6 * gr.node0; g.diag = a.diag + 6 * gr.node0; g.gs = a.gs + 6 * gr.node0; g.y = a.y + 6 * gr.node0;
  g.r = a.r + 6 * gr.node0; g.z = a.z + 6 * gr.node0; g.p = a.p + 6 * gr.node0; g.Ap = a.Ap + 6 * gr.node0;
  g.Ld = a.Ld + 36 * gr.node0; g.Lo = a.Lo + 36 * gr.node0;
  g.cauchy_a = a.cauchy_a;
  const int n = g.n, nv = 6 * n, lane = g.lane;

  // ---- ceres::Solve: trust-region Levenberg-Marquardt, as cfear_pgo_solve --------------------------------------------
  const double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  const double min_relative_decrease = 1e-3, min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32, max_radius = 1e16, min_radius = 1e-32;
  double radius = 1e4, decrease_factor = 2.0;
  bool reuse_diagonal = false;
  double x_cost = evaluate(g, g.x, true);
  gradient(g, g.gs);                                               // of the unscaled Jacobian
  double gradient_max_norm = max_abs(g, g.gs);
  node_sums<true>(g, g.diag);
  for (int k = lane; k < nv; k += kPgoThreads) g.scale[k] = k < 6 ? 1.0 : 1.0 / (1.0 + std::sqrt(g.diag[k]));
  __syncthreads();
  scale_columns(g);
  double x_norm = x_norm_of(g);
  const double initial_cost = x_cost;
  double min_cost = x_cost, it_cost = x_cost, it_rel = 0.0;
  bool it_success = true, usable = true;
  int iteration = 0, invalid = 0, n_pushed = 0, linear_iterations = 0;
  for (;;) {
    n_pushed++;
    min_cost = min_cost < it_cost ? min_cost : it_cost;
    if (iteration >= a.max_iter) break;
    if (it_success && gradient_max_norm <= gradient_tolerance) break;
    if (radius <= min_radius) break;
    iteration++;
    it_cost = 0.0; it_rel = 0.0; it_success = false;
    // LevenbergMarquardtStrategy::ComputeStep
    if (!reuse_diagonal) {
      node_sums<true>(g, g.diag);                                  // of the scaled Jacobian
      for (int k = lane; k < nv; k += kPgoThreads) g.diag[k] = fmin(fmax(g.diag[k], min_lm_diagonal), max_lm_diagonal);
      __syncthreads();
    }
    gradient(g, g.gs);                                             // J_s^T r
    // (J_s^T J_s + D^2) y = J_s^T r by preconditioned conjugate gradients
    assemble_blocks(g, radius, true);
    if (!factor_chain(g, true)) {
      assemble_blocks(g, radius, false);
      if (!factor_chain(g, false)) { usable = false; break; }
    }
    for (int k = lane; k < nv; k += kPgoThreads) { g.y[k] = 0.0; g.r[k] = g.gs[k]; }
    __syncthreads();
    precond_apply(g, g.r, g.z);
    for (int k = lane; k < nv; k += kPgoThreads) g.p[k] = g.z[k];
    __syncthreads();
    double rz = dot(g, g.r, g.z);
    const double r0 = std::sqrt(dot(g, g.r, g.r));
    int cg = 0;
    for (; cg < 500 && r0 > 0.0; cg++) {
      JtJv(g, g.p, radius, g.Ap);
      const double pAp = dot(g, g.p, g.Ap);
      if (!(pAp > 0.0)) break;
      const double alpha = rz / pAp;
      for (int k = lane; k < nv; k += kPgoThreads) { g.y[k] += alpha * g.p[k]; g.r[k] -= alpha * g.Ap[k]; }
      __syncthreads();
      if (std::sqrt(dot(g, g.r, g.r)) <= 1e-13 * r0) { cg++; break; }
      precond_apply(g, g.r, g.z);
      const double rz2 = dot(g, g.r, g.z);
      const double beta = rz2 / rz;
      rz = rz2;
      for (int k = lane; k < nv; k += kPgoThreads) g.p[k] = g.z[k] + beta * g.p[k];
      __syncthreads();
    }
    linear_iterations += cg;
    reuse_diagonal = true;
    bool bad = false;
    for (int k = lane; k < nv; k += kPgoThreads) bad = bad || !std::isfinite(g.y[k]);
    const bool finite = __ballot(bad) == 0;
    // model_cost_change = -(J step)^T (r + J step / 2), step = -y
    double model_cost_change = 0.0;
    if (finite) {
      Jv(g, g.y, -1.0);
      double s = 0.0;
      for (int c = lane; c < g.m; c += kPgoThreads)
        for (int i = 0; i < 6; i++) { const double t = g.t[(size_t)i * g.m + c]; s -= t * (g.res[(size_t)i * g.m + c] + t / 2.0); }
      model_cost_change = wave_sum_xor32_to_1(s);
    }
    if (!finite || !(model_cost_change > 0.0)) {                   // HandleInvalidStep
      if (++invalid >= 5) { usable = false; break; }
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
      it_cost = x_cost; it_success = false; it_rel = 0.0;
      continue;
    }
    invalid = 0;
    double step_norm2 = 0.0;
    if (lane == 0) g.cand[0] = g.x[0];
    for (int i = 1 + lane; i < n; i += kPgoThreads) {
      double d[6];
      for (int k = 0; k < 6; k++) d[k] = -g.y[(size_t)6 * i + k] * g.scale[(size_t)6 * i + k];
      const cfear_pose3d xi = g.x[i];
      cfear_pose3d ci;
      pgo::plus(xi, d, ci);
      g.cand[i] = ci;
      for (int k = 0; k < 3; k++) step_norm2 += (xi.p[k] - ci.p[k]) * (xi.p[k] - ci.p[k]);
      for (int k = 0; k < 4; k++) step_norm2 += (xi.q[k] - ci.q[k]) * (xi.q[k] - ci.q[k]);
    }
    __syncthreads();
    step_norm2 = wave_sum_xor32_to_1(step_norm2);
    const double cand_cost = evaluate(g, g.cand, false);
    if (std::sqrt(step_norm2) <= parameter_tolerance * (x_norm + parameter_tolerance)) break;    // ParameterToleranceReached
    const double cost_change = x_cost - cand_cost;
    if (std::fabs(cost_change) <= function_tolerance * x_cost) break;                            // FunctionToleranceReached
    it_rel = cost_change / model_cost_change;
    if (it_rel > min_relative_decrease) {                          // HandleSuccessfulStep
      for (int i = lane; i < n; i += kPgoThreads) g.x[i] = g.cand[i];
      __syncthreads();
      x_norm = x_norm_of(g);
      x_cost = evaluate(g, g.x, true);
      gradient(g, g.gs);
      gradient_max_norm = max_abs(g, g.gs);
      scale_columns(g);
      it_cost = x_cost; it_success = true;
      const double q = 2.0 * it_rel - 1.0;
      radius = fmin(max_radius, radius / fmax(1.0 / 3.0, 1.0 - q * q * q));
      decrease_factor = 2.0; reuse_diagonal = false;
    } else {
      it_cost = cand_cost; it_success = false;
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
    }
  }
  if (lane == 0) {
    cfear_pgo_summary s;
    s.initial_cost = initial_cost;
    s.final_cost = initial_cost < min_cost ? initial_cost : min_cost;   // solver.cc SetSummaryFinalCost
    s.iterations = n_pushed - 1;
    s.usable = usable ? 1 : 0;
    s.num_residual_blocks = g.m;
    s.linear_iterations = linear_iterations;
    a.summaries[blockIdx.x] = s;
  }
}

// one graph as the validation pass leaves it: its residual blocks in solver order
struct Prepared {
  int64_t term0;             // first of its entries in the batch's term list
  int32_t m, n_odom;
  int64_t factor0;           // first of its sqrt_information factors (information mode only)
};

size_t graph_bytes(int64_t n, int64_t m, bool shared_factors) {
  return (size_t)n * (2 * sizeof(cfear_pose3d) + 8 * 48 + 2 * 288 + 4) + (size_t)m * (3 * 4 + sizeof(cfear_pose3d) + 2 * 4 + 8 * (6 + 72 + 6) + (shared_factors ? 0 : 288)) +
         sizeof(PgoGraph) + sizeof(cfear_pgo_summary) + 16 * 256;
}

}  // namespace

extern "C" int cfear_pgo_solve_batch(cfear_ctx* ctx, cfear_pose3d* poses, const uint64_t* ids, const int64_t* node_offsets,
                                     int64_t n_nodes, const cfear_graph_constraint* constraints, const int64_t* constraint_offsets,
                                     int64_t n_constraints, int32_t n_graphs, const cfear_pgo_params* par, cfear_pgo_summary* summaries,
                                     int32_t* failed_graph) {
  if (failed_graph) *failed_graph = -1;
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n_graphs < 0 || n_nodes < 0 || n_constraints < 0 || !par || !node_offsets || !constraint_offsets)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null or negative argument (node_offsets and constraint_offsets hold n_graphs + 1 entries)");
  if (n_graphs > 0 && (!poses || !ids || !summaries || (n_constraints > 0 && !constraints)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (cfear_is_device_ptr(poses) || cfear_is_device_ptr(summaries))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "poses and summaries must be host memory");
  const OffsetsReport nodes = check_offsets(node_offsets, n_graphs, n_nodes), cons = check_offsets(constraint_offsets, n_graphs, n_constraints);
  if (nodes.start_not_0 || cons.start_not_0 || nodes.end_not_total || cons.end_not_total)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "offsets must run from 0 to n_nodes / n_constraints over n_graphs + 1 entries");
  const int64_t descends = std::min(nodes.descends, cons.descends);   // between a right start and a right end only a descent is left
  for (int gi = 0; gi < n_graphs; gi++)
    if (gi == descends || node_offsets[gi + 1] - node_offsets[gi] > INT32_MAX / 72 || constraint_offsets[gi + 1] - constraint_offsets[gi] > INT32_MAX / 72) {
      if (failed_graph) *failed_graph = gi;
      return cfear_set_error(ctx, gi == descends ? CFEAR_ERR_INVALID_ARGUMENT : CFEAR_ERR_CAPACITY,
                             "graph %d: offsets descend, or more than %d nodes / constraints", gi, INT32_MAX / 72);
    }
  if (n_graphs == 0) return CFEAR_OK;
  // ---- every graph is checked before anything is launched or written: what cfear_pgo_solve refuses fails the batch --------
  const bool shared_factors = par->replace_cov_by_identity != 0;
  std::vector<Prepared> prep(n_graphs);
  std::vector<pgo::Term> terms, all_terms;
  std::vector<pgo::Factor> factors, all_factors;
  for (int gi = 0; gi < n_graphs; gi++) {
    const int64_t n = node_offsets[gi + 1] - node_offsets[gi], m = constraint_offsets[gi + 1] - constraint_offsets[gi];
    int rc = n < 1 || m < 1 ? CFEAR_ERR_INVALID_ARGUMENT
                            : pgo::collect_terms(ids + node_offsets[gi], (int)n, constraints + constraint_offsets[gi], (int)m, par, terms, factors);
    if (rc == CFEAR_OK && graph_bytes(n, (int64_t)terms.size(), shared_factors) > kPgoBudget) rc = CFEAR_ERR_CAPACITY;
    if (rc != CFEAR_OK) {
      if (failed_graph) *failed_graph = gi;
      return cfear_set_error(ctx, rc, rc == CFEAR_ERR_CAPACITY ? "graph %d needs more than the %zu MB a chunk may take"
                                                               : "graph %d refused: ids must ascend, constraints must join known nodes, at least one "
                                                                 "odometry or loop constraint, positive definite information",
                             gi, kPgoBudget >> 20);
    }
    prep[gi].term0 = (int64_t)all_terms.size();
    prep[gi].m = (int32_t)terms.size();
    prep[gi].n_odom = 0;
    for (const pgo::Term& t : terms) prep[gi].n_odom += t.cauchy ? 0 : 1;
    prep[gi].factor0 = (int64_t)all_factors.size();
    all_terms.insert(all_terms.end(), terms.begin(), terms.end());
    if (!shared_factors) all_factors.insert(all_factors.end(), factors.begin(), factors.end());
  }
  if (shared_factors) {
    // with the identity replacement all graphs share two factors, [0] odometry and [1] loops; one that is not positive
    // definite was refused above if any graph uses it
    all_factors.assign(2, pgo::Factor{});
    for (int pass = 0; pass < 2; pass++) (void)pgo::scaled_factor(par, constraints[0], pass, all_factors[pass]);
  }
  std::vector<int32_t> fill;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int64_t cap = ctx->opt[CFEAR_OPT_PGO_GRAPH_CHUNK];
  for (int g0 = 0; g0 < n_graphs;) {
    // ---- the chunk: as many graphs as the budget (and the option) allow; at least one (checked above) -------------------
    int g1 = g0;
    size_t bytes = 0;
    int64_t nodes = 0, cons = 0;
    while (g1 < n_graphs && (cap <= 0 || g1 - g0 < cap)) {
      const int64_t n = node_offsets[g1 + 1] - node_offsets[g1];
      const size_t b = graph_bytes(n, prep[g1].m, shared_factors);
      if (g1 > g0 && bytes + b > kPgoBudget) break;
      bytes += b; nodes += n; cons += prep[g1].m;
      g1++;
    }
    const int ng = g1 - g0;
    const int64_t n_fac = shared_factors ? 2 : cons;
    HostStage st(ctx, kWsPgo);
    PgoArgs a{};
    a.cauchy_a = par->loop_loss_limit;
    a.max_iter = par->max_num_iterations;
    st.in(a.x, poses + node_offsets[g0], (size_t)nodes * sizeof(cfear_pose3d), true);
    st.out(a.summaries, summaries + g0, (size_t)ng * sizeof(cfear_pgo_summary));
    // the tables the host builds, in one record: graphs | ca | cb | lidx | nc_ptr | nc_idx | meas | factors
    const size_t o_graphs = 0, o_ca = o_graphs + (size_t)ng * sizeof(PgoGraph), o_cb = o_ca + (size_t)cons * 4, o_lidx = o_cb + (size_t)cons * 4;
    const size_t o_ptr = o_lidx + (size_t)cons * 4, o_idx = o_ptr + (size_t)(nodes + ng) * 4;
    const size_t o_meas = (o_idx + (size_t)cons * 8 + 15) & ~(size_t)15, o_fac = o_meas + (size_t)cons * sizeof(cfear_pose3d);
    const size_t tab_bytes = o_fac + (size_t)n_fac * sizeof(pgo::Factor);
    char* d_tab;
    st.piece(d_tab, tab_bytes);
    st.piece(a.cand, (size_t)nodes * sizeof(cfear_pose3d));
    st.piece(a.res, (size_t)cons * 48);
    st.piece(a.J, (size_t)cons * 576);
    st.piece(a.t, (size_t)cons * 48);
    for (double** v : {&a.scale, &a.diag, &a.gs, &a.y, &a.r, &a.z, &a.p, &a.Ap}) st.piece(*v, (size_t)nodes * 48);
    st.piece(a.Ld, (size_t)nodes * 288);
    st.piece(a.Lo, (size_t)nodes * 288);
    CFEAR_CHECK(st.carve());
    char* h = (char*)st.record(tab_bytes);
    PgoGraph* hg = (PgoGraph*)(h + o_graphs);
    int32_t *h_ca = (int32_t*)(h + o_ca), *h_cb = (int32_t*)(h + o_cb), *h_lidx = (int32_t*)(h + o_lidx);
    int32_t *h_ptr = (int32_t*)(h + o_ptr), *h_idx = (int32_t*)(h + o_idx);
    cfear_pose3d* h_meas = (cfear_pose3d*)(h + o_meas);
    pgo::Factor* h_fac = (pgo::Factor*)(h + o_fac);
    if (shared_factors) { h_fac[0] = all_factors[0]; h_fac[1] = all_factors[1]; }
    int64_t node0 = 0, con0 = 0;
    for (int gi = g0; gi < g1; gi++) {
      const int n = (int)(node_offsets[gi + 1] - node_offsets[gi]), m = prep[gi].m;
      const pgo::Term* tm = all_terms.data() + prep[gi].term0;
      const cfear_graph_constraint* gc = constraints + constraint_offsets[gi];
      hg[gi - g0] = PgoGraph{node0, con0, node0 + (gi - g0), n, m, prep[gi].n_odom, 0};
      int32_t* ptr = h_ptr + node0 + (gi - g0);
      for (int i = 0; i <= n; i++) ptr[i] = 0;
      for (int c = 0; c < m; c++) {
        h_ca[con0 + c] = tm[c].a; h_cb[con0 + c] = tm[c].b;
        h_meas[con0 + c] = gc[tm[c].j].t_be;
        if (shared_factors) h_lidx[con0 + c] = tm[c].cauchy ? 1 : 0;
        else { h_lidx[con0 + c] = (int32_t)(con0 + c); h_fac[con0 + c] = all_factors[prep[gi].factor0 + tm[c].l]; }
        ptr[tm[c].a + 1]++; ptr[tm[c].b + 1]++;
      }
      for (int i = 0; i < n; i++) ptr[i + 1] += ptr[i];
      // counting sort by node, stable in the block order: a node's entries ascend, the a side of a block before its b side
      fill.assign(ptr, ptr + n);
      for (int c = 0; c < m; c++) {
        h_idx[2 * con0 + fill[tm[c].a]++] = c << 1;
        h_idx[2 * con0 + fill[tm[c].b]++] = c << 1 | 1;
      }
      node0 += n; con0 += m;
    }
    CFEAR_CHECK(st.upload(d_tab, h, tab_bytes));
    a.graphs = (const PgoGraph*)(d_tab + o_graphs);
    a.ca = (const int32_t*)(d_tab + o_ca); a.cb = (const int32_t*)(d_tab + o_cb); a.lidx = (const int32_t*)(d_tab + o_lidx);
    a.nc_ptr = (const int32_t*)(d_tab + o_ptr); a.nc_idx = (const int32_t*)(d_tab + o_idx);
    a.meas = (const cfear_pose3d*)(d_tab + o_meas);
    a.factors = (const double*)(d_tab + o_fac);
    {
      ProfScope ps(ctx, "pgo_batch");
      hipLaunchKernelGGL(pgo_batch_kernel, dim3(ng), dim3(kPgoThreads), 0, ctx->stream, a);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    CFEAR_CHECK(st.finish());
    g0 = g1;
  }
  return CFEAR_OK;
}
