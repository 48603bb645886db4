// covfit.hip -- covariance of a registration by cost sampling: the fit on the device.
//
// cov_fit_kernel does per job what cfear_covariance_by_sampling_batch (register.hip) does on the host between the matcher's
// sampling launch and its outputs: the carry-over of failed samples, CovFit::solve (covfit.hpp) -- the ten coefficients of the
// quadratic, the convexity test by cyclic Jacobi, 2 H^-1 scaled by the registration's score -- and Register's constant
// covariance where the fit is refused.  One lane per job; every sum in the host's order, one accumulator per coefficient.  The
// library is built with -ffp-contract=off and fp64 + - x / sqrt round on the device as on the host, so cov36 and success are
// the host fit's bit for bit (tests/test_gpu_covfit_device.py holds them to tests/cpp/covfit_check.cpp).  The pseudo-inverse
// of the design matrix is still CovFit::prepare's, built once per call on the host and uploaded.
#include <cmath>

#include "covfit.hpp"
#include "registration.hpp"

namespace {

constexpr int kCovFitThreads = 256;

// sym3_eigenvalues (covfit.hpp) without the sort: the verdict "finite and all > 0" does not depend on the order
__device__ __forceinline__ bool sym3_positive(const double Hin[9]) {
  double a[9];
#pragma unroll
  for (int k = 0; k < 9; k++) a[k] = Hin[k];
  for (int sweep = 0; sweep < 50; sweep++) {
    const double off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5];
    const double diag = a[0] * a[0] + a[4] * a[4] + a[8] * a[8];
    if (off <= 1e-32 * diag || off == 0.0) break;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const int p = r == 2 ? 1 : 0, q = r == 0 ? 1 : 2;
      const double apq = a[p * 3 + q];
      if (apq == 0.0) continue;
      const double theta = (a[q * 3 + q] - a[p * 3 + p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
      for (int k = 0; k < 3; k++) {                      // A <- A J
        const double akp = a[k * 3 + p], akq = a[k * 3 + q];
        a[k * 3 + p] = c * akp - s * akq;
        a[k * 3 + q] = s * akp + c * akq;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {                      // A <- J^T A
        const double apk = a[p * 3 + k], aqk = a[q * 3 + k];
        a[p * 3 + k] = c * apk - s * aqk;
        a[q * 3 + k] = s * apk + c * aqk;
      }
    }
  }
  const bool finite = fabs(a[0]) <= 1.7976931348623157e308 && fabs(a[4]) <= 1.7976931348623157e308 && fabs(a[8]) <= 1.7976931348623157e308;
  return finite && a[0] > 0.0 && a[4] > 0.0 && a[8] > 0.0;
}

// regs [n_jobs], samples [n_jobs][m], pinv [10][m] -> cov36 [n_jobs][36], success [n_jobs]
__global__ __launch_bounds__(kCovFitThreads) void cov_fit_kernel(const cfear_reg_result* __restrict__ regs,
                                                                 const cfear_reg_result* __restrict__ samples,
                                                                 const double* __restrict__ pinv, int n_jobs, int m,
                                                                 double covariance_scaler, double* __restrict__ cov36,
                                                                 int32_t* __restrict__ success) {
  const int j = blockIdx.x * kCovFitThreads + threadIdx.x;
  if (j >= n_jobs) return;
  const cfear_reg_result* sj = samples + (size_t)j * m;
  double q[10];
#pragma unroll
  for (int k = 0; k < 10; k++) q[k] = 0.0;
  double sample_cost = 0.0;                                  // a failed GetCost leaves the previous value (odometrykeyframefuser.cpp:282, 307)
  for (int s = 0; s < m; s++) {
    if (sj[s].status == CFEAR_OK) sample_cost = sj[s].final_cost;
#pragma unroll
    for (int k = 0; k < 10; k++) q[k] += pinv[(size_t)k * m + s] * sample_cost;
  }
  const int dof = regs[j].num_residuals - 3;                // GetCovarianceScaler (n_scan_normal.cpp:433-439)
  bool ok = dof != 0;
  double c3[9];
  if (ok) {
    const double score_scale = regs[j].final_cost / (double)dof;
    const double H[9] = {2 * q[0], q[3], q[5], q[3], 2 * q[1], q[4], q[5], q[4], 2 * q[2]};
    ok = sym3_positive(H);
    const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
    double inv[9];
    inv[0] = (H[4] * H[8] - H[5] * H[7]) / det; inv[1] = (H[2] * H[7] - H[1] * H[8]) / det; inv[2] = (H[1] * H[5] - H[2] * H[4]) / det;
    inv[3] = (H[5] * H[6] - H[3] * H[8]) / det; inv[4] = (H[0] * H[8] - H[2] * H[6]) / det; inv[5] = (H[2] * H[3] - H[0] * H[5]) / det;
    inv[6] = (H[3] * H[7] - H[4] * H[6]) / det; inv[7] = (H[1] * H[6] - H[0] * H[7]) / det; inv[8] = (H[0] * H[4] - H[1] * H[3]) / det;
#pragma unroll
    for (int k = 0; k < 9; k++) c3[k] = 2.0 * inv[k] * score_scale * covariance_scaler;
  }
  if (!ok) {                                                 // Register's constant reg_cov (n_scan_normal.cpp:171-175)
#pragma unroll
    for (int k = 0; k < 9; k++) c3[k] = 0.0;
    c3[0] = 0.01; c3[4] = 0.01; c3[8] = 1e-4;
  }
  const double one = ok ? 1.0 : 0.0;                         // the fitted 6 x 6 keeps the identity on z, roll, pitch
  double* c = cov36 + (size_t)j * 36;
#pragma unroll
  for (int k = 0; k < 36; k++) c[k] = 0.0;
  c[14] = one; c[21] = one; c[28] = one;
  c[0] = c3[0]; c[1] = c3[1]; c[6] = c3[3]; c[7] = c3[4];
  c[35] = c3[8];
  c[5] = c3[2]; c[11] = c3[5]; c[30] = c3[6]; c[31] = c3[7];
  success[j] = ok ? 1 : 0;
}

}  // namespace

size_t cfear_cov_fit_pinv_bytes(int samples_per_axis) {
  return (size_t)10 * samples_per_axis * samples_per_axis * samples_per_axis * sizeof(double);
}

void cfear_cov_fit_fill_pinv(const cfear_cov_sampling_params* sp, double* dst) {
  CovFit fit;
  fit.prepare(sp->samples_per_axis, sp->xy_range * 0.5, sp->yaw_range * 0.5);       // odometrykeyframefuser.cpp:276-277
  std::copy(fit.pinv.begin(), fit.pinv.end(), dst);
}

int cfear_cov_fit_launch(cfear_ctx* ctx, const cfear_reg_result* d_regs, const cfear_reg_result* d_samples, int n_jobs, int m,
                         const double* d_pinv, double covariance_scaler, double* d_cov36, int32_t* d_success) {
  ProfScope ps(ctx, "cov_fit");
  hipLaunchKernelGGL(cov_fit_kernel, dim3((unsigned)((n_jobs + kCovFitThreads - 1) / kCovFitThreads)), dim3(kCovFitThreads), 0, ctx->stream,
                     d_regs, d_samples, d_pinv, n_jobs, m, covariance_scaler, d_cov36, d_success);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_cov_check_sampling(cfear_ctx* ctx, const cfear_cov_sampling_params* sp) {
  if (sp->samples_per_axis < 1 || sp->samples_per_axis > 15)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "samples_per_axis must be in [1,15]");
  return CFEAR_OK;
}

extern "C" int cfear_cov_fit_records(cfear_ctx* ctx, const cfear_reg_result* regs, const cfear_reg_result* samples, int32_t n_jobs,
                                     const cfear_cov_sampling_params* sp, double* cov36, int32_t* success) {
  if (!regs || !samples || !sp || !cov36 || !success || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(cfear_cov_check_sampling(ctx, sp));
  if (memory_kind({regs, samples, cov36, success}) < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "regs, samples, cov36 and success must be all host or all device memory");
  if (!ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null context");
  if (n_jobs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int m = sp->samples_per_axis * sp->samples_per_axis * sp->samples_per_axis;
  HostStage st(ctx, kWsRegJobs);
  const cfear_reg_result *d_regs, *d_samples;
  double *d_cov, *d_pinv;
  int32_t* d_ok;
  st.in(d_regs, regs, (size_t)n_jobs * sizeof(cfear_reg_result));
  st.in(d_samples, samples, (size_t)n_jobs * m * sizeof(cfear_reg_result));
  st.out(d_cov, cov36, (size_t)n_jobs * 36 * sizeof(double));
  st.out(d_ok, success, (size_t)n_jobs * sizeof(int32_t));
  st.piece(d_pinv, cfear_cov_fit_pinv_bytes(sp->samples_per_axis));
  CFEAR_CHECK(st.carve());
  // the pseudo-inverse goes up from the pinned staging: a call whose records all sit on the device stays asynchronous
  double* h_pinv = (double*)st.pinned(cfear_cov_fit_pinv_bytes(sp->samples_per_axis));
  if (!h_pinv) return CFEAR_ERR_HIP;
  cfear_cov_fit_fill_pinv(sp, h_pinv);
  CFEAR_CHECK(st.upload(d_pinv, h_pinv, cfear_cov_fit_pinv_bytes(sp->samples_per_axis)));
  CFEAR_CHECK(cfear_cov_fit_launch(ctx, d_regs, d_samples, n_jobs, m, d_pinv, sp->covariance_scaler, d_cov, d_ok));
  return st.finish();
}
