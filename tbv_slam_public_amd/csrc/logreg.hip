// logreg.hip -- cfear_logreg_fit_batch: the coefficients of the alignment and loop classifiers, fitted on the device
// (gfx950, wave64, fp64).
//
// What the reference gets from sklearn.linear_model.LogisticRegression(class_weight="balanced", max_iter=1000) through
// pybind11 (alignmentinterface.cpp:192-222) is the minimiser of
//     F(w, b) = 1/2 w.w + C sum_i s_i [log(1 + exp(z_i)) - y_i z_i],   z_i = w.x_i + b,   s_i = n / (2 n_class(i)),
// which is unique when both classes are present.  logreg_kernel finds it by a damped Newton iteration, one workgroup per
// model and the whole loop on the device, the way pgo_batch_kernel keeps its solver loop there:
//   * one pass over the rows per iteration accumulates F, the gradient and the upper Hessian in registers, one row per
//     thread and step;
//   * every sum is reduced by a fixed tree: a DPP butterfly inside each row of 16 lanes, two cross-row exchanges, then the
//     wavefronts' partial sums are added through LDS in wavefront order.  No atomics, and a fixed number of threads, so a
//     model's record depends on its rows alone -- not on its position in the batch, its neighbours, or where X came from;
//   * thread 0 solves the (d + 1)^2 system by LDL^T of the Jacobi-scaled Hessian, in LDS, and steers the loop through a
//     flag the workgroup reads after a barrier;
//   * Armijo backtracking, one objective pass per trial step;
//   * the stop rule is relative: the Newton decrement against max(1, |F|), or no trial step that decreases F.  An
//     absolute gradient norm is never reached on 58 k rows (the sums carry about 1e-9 of rounding).
// tests/logreg_cpu.py restates the same iteration in NumPy; DESIGN.md section 4.11 says what is pinned.
#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kLrThreads = 512;                              // 8 wavefronts: 256 VGPRs a lane, enough for the 55 sums of d = 8
constexpr int kLrWaves = kLrThreads / CFEAR_WAVE;
constexpr int kLrMaxD = CFEAR_LOGREG_MAX_FEATURES, kLrMaxP = kLrMaxD + 1;
constexpr int kLrMaxSums = 1 + kLrMaxP + kLrMaxP * (kLrMaxP + 1) / 2;
constexpr double kLrDecTol = 1e-16, kLrArmijo = 1e-4, kLrMinStep = 1.0 / 1048576.0;

struct LrJob {
  const double* X;
  const double* y;
  const uint8_t* mask;
  int64_t n_rows;
  int32_t stride, d;
  int32_t col[kLrMaxD];
};

enum LrFlag : int { kLrContinue = 0, kLrConverged, kLrFailed, kLrAccepted, kLrRetry };

// The same bits in every lane: each level adds a pair both ways round, and a + b == b + a.  Not common.hpp's wave_sum_f64
// nor pgo_batch.hip's sum: the order of the additions differs, so the rounding does.
__device__ __forceinline__ double wave_sum_rows_xor16_xor32(double v) {
  v = row16_sum_f64(v);                                      // the DPP butterfly inside each row of 16 lanes
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// tot[k] = sum over the workgroup of acc[k], k < N: wavefronts in order 0 .. 7.  Ends with a barrier; tot is then valid for all.
template <int N> __device__ void block_sums(double (&acc)[N], double* part, double* tot) {
  const int lane = threadIdx.x & (CFEAR_WAVE - 1), wave = threadIdx.x / CFEAR_WAVE;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double s = wave_sum_rows_xor16_xor32(acc[k]);
    if (lane == 0) part[wave * N + k] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < N) {
    double s = part[threadIdx.x];
    for (int w = 1; w < kLrWaves; w++) s += part[w * N + threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
}

// log(1 + exp(z)) and the logistic terms without overflow at any finite z: everything goes through e = exp(-|z|) <= 1
struct Logistic { double softplus, p, q; };                  // p = sigmoid(z), q = p (1 - p)
__device__ __forceinline__ Logistic logistic(double z) {
  const double e = exp(-fabs(z)), inv = 1.0 / (1.0 + e);
  return Logistic{fmax(z, 0.0) + log1p(e), z >= 0.0 ? inv : e * inv, e * inv * inv};
}

template <int D> __device__ __forceinline__ void load_row(const LrJob& j, int64_t i, double one, double (&a)[D + 1]) {
  const double* r = j.X + i * j.stride;
#pragma unroll
  for (int k = 0; k < D; k++) a[k] = r[j.col[k]];
  a[D] = one;
}
template <int D> __device__ __forceinline__ double logit(const double (&a)[D + 1], const double* v) {
  double z = 0.0;
#pragma unroll
  for (int k = 0; k <= D; k++) z += v[k] * a[k];
  return z;
}

// LDL^T of S H S, S = diag(H)^-1/2, and H dw = -g.  Thread 0 only; H (full, p x p), L, and the vectors live in LDS.
__device__ bool solve_newton(int p, const double* H, const double* g, double* L, double* sc, double* dg, double* dw) {
  for (int i = 0; i < p; i++) {
    sc[i] = 1.0 / sqrt(H[i * p + i]);
    if (!isfinite(sc[i])) return false;
  }
  for (int c = 0; c < p; c++) {
    double d = H[c * p + c] * sc[c] * sc[c];
    for (int k = 0; k < c; k++) d -= L[c * p + k] * L[c * p + k] * dg[k];
    if (!(d > 0.0)) return false;
    dg[c] = d;
    for (int r = c + 1; r < p; r++) {
      double s = H[r * p + c] * sc[r] * sc[c];
      for (int k = 0; k < c; k++) s -= L[r * p + k] * L[c * p + k] * dg[k];
      L[r * p + c] = s / d;
    }
  }
  for (int i = 0; i < p; i++) {
    double s = -g[i] * sc[i];
    for (int k = 0; k < i; k++) s -= L[i * p + k] * dw[k];
    dw[i] = s;
  }
  for (int i = 0; i < p; i++) dw[i] /= dg[i];
  for (int i = p - 1; i >= 0; i--) {
    double s = dw[i];
    for (int k = i + 1; k < p; k++) s -= L[k * p + i] * dw[k];
    dw[i] = s;
  }
  for (int i = 0; i < p; i++) {
    dw[i] *= sc[i];
    if (!isfinite(dw[i])) return false;
  }
  return true;
}

struct LrShared {
  double part[kLrWaves * kLrMaxSums], tot[kLrMaxSums];
  double H[kLrMaxP * kLrMaxP], L[kLrMaxP * kLrMaxP];
  double v[kLrMaxP], vt[kLrMaxP], dw[kLrMaxP], g[kLrMaxP], sc[kLrMaxP], dg[kLrMaxP];
  double F, dec, t, grad_inf;
  int flag, iterations;
};

template <int D>
__device__ void fit_model(const LrJob& j, const cfear_logreg_params& par, LrShared& sh, cfear_logreg_result* out) {
  constexpr int P = D + 1, NH = P * (P + 1) / 2, NS = 1 + P + NH;
  const int tid = threadIdx.x;
  const int64_t n = j.n_rows;
  const double one = par.fit_intercept ? 1.0 : 0.0;

  // ---- the rows: used, positive, unusable (a label that is not 0 or 1, a value that is not finite).  Counts are exact in fp64.
  {
    double c[3] = {0.0, 0.0, 0.0};
    for (int64_t i = tid; i < n; i += kLrThreads) {
      if (j.mask && !j.mask[i]) continue;
      double a[P];
      load_row<D>(j, i, one, a);
      const double y = j.y[i];
      bool bad = !(y == 0.0 || y == 1.0);
#pragma unroll
      for (int k = 0; k < D; k++) bad = bad || !isfinite(a[k]);
      c[0] += 1.0; c[1] += y == 1.0 ? 1.0 : 0.0; c[2] += bad ? 1.0 : 0.0;
    }
    block_sums<3>(c, sh.part, sh.tot);
  }
  const double n_used = sh.tot[0], n_pos = sh.tot[1], n_bad = sh.tot[2];
  __syncthreads();                                           // tot is rewritten by the next reduction
  if (n_used == 0.0 || n_bad > 0.0 || n_pos == 0.0 || n_pos == n_used) {
    if (tid == 0) {
      cfear_logreg_result r{};
      r.n_used = (int64_t)n_used; r.n_pos = (int64_t)n_pos;
      r.status = CFEAR_ERR_INVALID_ARGUMENT;
      *out = r;
    }
    return;
  }
  const double s_pos = par.C * (par.class_weight_balanced ? n_used / (2.0 * n_pos) : 1.0);
  const double s_neg = par.C * (par.class_weight_balanced ? n_used / (2.0 * (n_used - n_pos)) : 1.0);
  if (tid < P) sh.v[tid] = 0.0;
  if (tid == 0) sh.iterations = 0;
  __syncthreads();

  for (;;) {
    // ---- F, gradient and upper Hessian at v: one pass ------------------------------------------------------------------
    {
      double v[P];
#pragma unroll
      for (int k = 0; k < P; k++) v[k] = sh.v[k];
      double acc[NS];
#pragma unroll
      for (int k = 0; k < NS; k++) acc[k] = 0.0;
      for (int64_t i = tid; i < n; i += kLrThreads) {
        if (j.mask && !j.mask[i]) continue;
        double a[P];
        load_row<D>(j, i, one, a);
        const double y = j.y[i], s = y != 0.0 ? s_pos : s_neg;
        const double z = logit<D>(a, v);
        const Logistic lg = logistic(z);
        acc[0] += s * (lg.softplus - y * z);
        const double r = s * (lg.p - y), sq = s * lg.q;
        int h = 1 + P;
#pragma unroll
        for (int k = 0; k < P; k++) {
          acc[1 + k] += r * a[k];
          const double qa = sq * a[k];
#pragma unroll
          for (int m = k; m < P; m++) acc[h++] += qa * a[m];
        }
      }
      block_sums<NS>(acc, sh.part, sh.tot);
    }
    if (tid == 0) {
      double ww = 0.0, gmax = 0.0;
      for (int k = 0; k < D; k++) ww += sh.v[k] * sh.v[k];
      const double F = 0.5 * ww + sh.tot[0];
      int h = 1 + P;
      for (int k = 0; k < P; k++) {
        sh.g[k] = sh.tot[1 + k] + (k < D ? sh.v[k] : 0.0);
        gmax = fmax(gmax, fabs(sh.g[k]));
        for (int m = k; m < P; m++) { sh.H[k * P + m] = sh.H[m * P + k] = sh.tot[h++] + (k == m && k < D ? 1.0 : 0.0); }
      }
      if (!par.fit_intercept) sh.H[D * P + D] = 1.0;         // the column of ones is a column of zeros: dw[D] = 0
      sh.F = F; sh.grad_inf = gmax;
      int flag = kLrContinue;
      if (!isfinite(F) || !isfinite(gmax) || !solve_newton(P, sh.H, sh.g, sh.L, sh.sc, sh.dg, sh.dw)) flag = kLrFailed;
      else {
        double dec = 0.0;
        for (int k = 0; k < P; k++) dec -= sh.g[k] * sh.dw[k];
        sh.dec = dec;
        if (!(dec > kLrDecTol * fmax(1.0, fabs(F)))) flag = dec == dec ? kLrConverged : kLrFailed;
        else if (sh.iterations >= par.max_iterations) flag = kLrFailed;
        else {
          sh.t = 1.0;
          for (int k = 0; k < P; k++) sh.vt[k] = sh.v[k] + sh.dw[k];
        }
      }
      sh.flag = flag;
    }
    __syncthreads();
    if (sh.flag != kLrContinue) break;
    // ---- backtracking: one objective pass per trial ------------------------------------------------------------------------
    for (;;) {
      double v[P];
#pragma unroll
      for (int k = 0; k < P; k++) v[k] = sh.vt[k];
      double f[1] = {0.0};
      for (int64_t i = tid; i < n; i += kLrThreads) {
        if (j.mask && !j.mask[i]) continue;
        double a[P];
        load_row<D>(j, i, one, a);
        const double y = j.y[i], s = y != 0.0 ? s_pos : s_neg;
        const double z = logit<D>(a, v);
        f[0] += s * (logistic(z).softplus - y * z);
      }
      block_sums<1>(f, sh.part, sh.tot);
      if (tid == 0) {
        double ww = 0.0;
        for (int k = 0; k < D; k++) ww += sh.vt[k] * sh.vt[k];
        const double Ft = 0.5 * ww + sh.tot[0];
        if (Ft <= sh.F - kLrArmijo * sh.t * sh.dec) {
          for (int k = 0; k < P; k++) sh.v[k] = sh.vt[k];
          sh.iterations++;
          sh.flag = kLrAccepted;
        } else {
          sh.t *= 0.5;
          if (sh.t < kLrMinStep) sh.flag = kLrConverged;     // no trial step decreases F: v is as good as fp64 sums can tell
          else {
            for (int k = 0; k < P; k++) sh.vt[k] = sh.v[k] + sh.t * sh.dw[k];
            sh.flag = kLrRetry;
          }
        }
      }
      __syncthreads();
      if (sh.flag != kLrRetry) break;
      __syncthreads();                                       // every thread has read the flag before thread 0 may rewrite it
    }
    if (sh.flag == kLrConverged) break;
    __syncthreads();
  }
  const int flag = sh.flag;

  // ---- what the reference prints after fit(): the confusion matrix and balanced accuracy of predict() on the training rows ----
  double c[4] = {0.0, 0.0, 0.0, 0.0};
  {
    double v[P];
#pragma unroll
    for (int k = 0; k < P; k++) v[k] = sh.v[k];
    for (int64_t i = tid; i < n; i += kLrThreads) {
      if (j.mask && !j.mask[i]) continue;
      double a[P];
      load_row<D>(j, i, one, a);
      const bool pos = j.y[i] != 0.0, pred = logit<D>(a, v) > 0.0;
      c[0] += !pos && !pred ? 1.0 : 0.0; c[1] += !pos && pred ? 1.0 : 0.0;
      c[2] += pos && !pred ? 1.0 : 0.0; c[3] += pos && pred ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  block_sums<4>(c, sh.part, sh.tot);
  if (tid == 0) {
    cfear_logreg_result r{};
    bool finite = true;
    for (int k = 0; k < D; k++) { r.coef[k] = sh.v[k]; finite = finite && isfinite(sh.v[k]); }
    r.intercept = sh.v[D];
    r.objective = sh.F; r.grad_inf = sh.grad_inf;
    r.n_used = (int64_t)n_used; r.n_pos = (int64_t)n_pos;
    for (int k = 0; k < 4; k++) r.confusion[k] = (int64_t)sh.tot[k];
    r.balanced_accuracy = 0.5 * (sh.tot[3] / (sh.tot[2] + sh.tot[3]) + sh.tot[0] / (sh.tot[0] + sh.tot[1]));
    r.iterations = sh.iterations;
    r.status = flag == kLrConverged && finite && isfinite(sh.v[D]) ? CFEAR_OK : CFEAR_ERR_SOLVER;
    *out = r;
  }
}

__global__ __launch_bounds__(kLrThreads) void logreg_kernel(const LrJob* jobs, cfear_logreg_params par, cfear_logreg_result* results) {
  __shared__ LrShared sh;
  const LrJob j = jobs[blockIdx.x];
  cfear_logreg_result* out = results + blockIdx.x;
  switch (j.d) {                                             // uniform: the sums of a model live in registers, so d is a template argument
    case 1: fit_model<1>(j, par, sh, out); break;
    case 2: fit_model<2>(j, par, sh, out); break;
    case 3: fit_model<3>(j, par, sh, out); break;
    case 4: fit_model<4>(j, par, sh, out); break;
    case 5: fit_model<5>(j, par, sh, out); break;
    case 6: fit_model<6>(j, par, sh, out); break;
    case 7: fit_model<7>(j, par, sh, out); break;
    default: fit_model<8>(j, par, sh, out); break;
  }
}

}  // namespace

extern "C" void cfear_logreg_params_default(cfear_logreg_params* p) {
  if (!p) return;
  p->C = 1.0;                              // sklearn's default, which the reference leaves (alignmentinterface.cpp:203)
  p->class_weight_balanced = 1;
  p->fit_intercept = 1;
  p->max_iterations = 100;
  p->pad = 0;
}

extern "C" int cfear_logreg_fit_batch(cfear_ctx* ctx, const cfear_logreg_job* jobs, int32_t n_jobs, const cfear_logreg_params* par,
                                      cfear_logreg_result* results) {
  // ---- refused at entry, before the context is touched and with nothing launched ------------------------------------------
  if (n_jobs < 0 || !par || (n_jobs > 0 && (!jobs || !results)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null or negative argument");
  if (!(par->C > 0.0) || !std::isfinite(par->C) || par->max_iterations < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "C must be positive and finite, max_iterations >= 0");
  for (int i = 0; i < n_jobs; i++) {
    const cfear_logreg_job& j = jobs[i];
    if (!j.X || !j.y || j.n_rows < 0)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: X or y is null, or n_rows < 0", i);
    if (j.n_features < 1 || j.n_features > CFEAR_LOGREG_MAX_FEATURES)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: n_features %d outside 1..%d", i, j.n_features, CFEAR_LOGREG_MAX_FEATURES);
    int32_t need = j.n_features;
    for (int k = 0; j.columns && k < j.n_features; k++) {
      if (j.columns[k] < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: negative column index", i);
      need = std::max(need, j.columns[k] + 1);
    }
    if (j.row_stride < need)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: row_stride %d is smaller than the %d values a row must hold", i, j.row_stride, need);
  }
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n_jobs == 0) return CFEAR_OK;
  if (cfear_is_device_ptr(results)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "results must be host memory");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // ---- every distinct buffer once, at the longest extent a job names: the models of one table share its upload -------------
  struct Up { size_t bytes = 0; const char* dev = nullptr; };
  std::map<const void*, Up> ups;
  auto want = [&](const void* p, size_t bytes) { if (p) { Up& u = ups[p]; u.bytes = std::max(u.bytes, bytes); } };
  for (int i = 0; i < n_jobs; i++) {
    const cfear_logreg_job& j = jobs[i];
    want(j.X, (size_t)j.n_rows * j.row_stride * sizeof(double));
    want(j.y, (size_t)j.n_rows * sizeof(double));
    want(j.row_mask, (size_t)j.n_rows);
  }
  HostStage st(ctx, kWsLogreg);
  for (auto& kv : ups) st.in(kv.second.dev, (const char*)kv.first, kv.second.bytes);
  LrJob* d_jobs;
  cfear_logreg_result* d_res;
  st.piece(d_jobs, (size_t)n_jobs * sizeof(LrJob));
  st.out(d_res, results, (size_t)n_jobs * sizeof(cfear_logreg_result));
  CFEAR_CHECK(st.carve());
  LrJob* h = (LrJob*)st.record((size_t)n_jobs * sizeof(LrJob));
  for (int i = 0; i < n_jobs; i++) {
    const cfear_logreg_job& j = jobs[i];
    h[i].X = (const double*)ups[j.X].dev;
    h[i].y = (const double*)ups[j.y].dev;
    h[i].mask = j.row_mask ? (const uint8_t*)ups[j.row_mask].dev : nullptr;
    h[i].n_rows = j.n_rows; h[i].stride = j.row_stride; h[i].d = j.n_features;
    for (int k = 0; k < kLrMaxD; k++) h[i].col[k] = k < j.n_features ? (j.columns ? j.columns[k] : k) : 0;
  }
  CFEAR_CHECK(st.upload(d_jobs, h, (size_t)n_jobs * sizeof(LrJob)));
  {
    ProfScope ps(ctx, "logreg_fit");
    hipLaunchKernelGGL(logreg_kernel, dim3(n_jobs), dim3(kLrThreads), 0, ctx->stream, (const LrJob*)d_jobs, *par, d_res);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}
