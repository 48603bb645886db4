// Stand-alone driver of the covariance fit (tbv_slam_public_amd/csrc/covfit.hpp) for tests/test_covfit_cpu.py.
//   covfit_check fit  n xy_half yaw_half score_scale scaler   (m = n^3 costs on stdin, any strtod spelling)
//       -> "offsets" 3m, "pinv" 10m, "verdict" 0|1, "cov36" 36 numbers, as hex floats
//   covfit_check old  n xy_half yaw_half    -> "pinv" 10m: the pseudo-inverse built column by column, one full solve per
//                                              unit right-hand side, as CovFit::prepare did before it factorised once
//   covfit_check time n xy_half yaw_half reps -> "seconds" the fastest of reps prepare() calls
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tbv_slam_public_amd/csrc/covfit.hpp"

namespace {

// ---- test code: the column-by-column construction, kept verbatim from the library's earlier form ----
void old_lstsq_jacobi(const std::vector<double>& A /*m x n row-major*/, const std::vector<double>& b, int m, int n, double* x) {
  const bool tall = m >= n;
  const int rows = tall ? m : n, cols = tall ? n : m;
  std::vector<double> W((size_t)rows * cols), R((size_t)cols * cols, 0.0);
  for (int i = 0; i < m; i++)
    for (int j = 0; j < n; j++) {
      if (tall) W[(size_t)j * rows + i] = A[(size_t)i * n + j];
      else W[(size_t)i * rows + j] = A[(size_t)i * n + j];
    }
  for (int j = 0; j < cols; j++) R[(size_t)j * cols + j] = 1.0;
  const double eps = std::numeric_limits<double>::epsilon();
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < cols - 1; p++)
      for (int q = p + 1; q < cols; q++) {
        double* wp = &W[(size_t)p * rows];
        double* wq = &W[(size_t)q * rows];
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < rows; i++) { alpha += wp[i] * wp[i]; beta += wq[i] * wq[i]; gamma += wp[i] * wq[i]; }
        if (gamma == 0.0 || std::fabs(gamma) <= eps * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < rows; i++) {
          const double a0 = wp[i], a1 = wq[i];
          wp[i] = c * a0 - s * a1;
          wq[i] = s * a0 + c * a1;
        }
        double* rp = &R[(size_t)p * cols];
        double* rq = &R[(size_t)q * cols];
        for (int i = 0; i < cols; i++) {
          const double a0 = rp[i], a1 = rq[i];
          rp[i] = c * a0 - s * a1;
          rq[i] = s * a0 + c * a1;
        }
      }
    if (!rotated) break;
  }
  std::vector<double> sig2(cols);
  double smax2 = 0.0;
  for (int j = 0; j < cols; j++) {
    double t = 0.0;
    for (int i = 0; i < rows; i++) t += W[(size_t)j * rows + i] * W[(size_t)j * rows + i];
    sig2[j] = t;
    smax2 = std::max(smax2, t);
  }
  const double thr = std::sqrt(smax2) * (double)std::min(m, n) * eps;
  for (int j = 0; j < n; j++) x[j] = 0.0;
  for (int j = 0; j < cols; j++) {
    if (!(std::sqrt(sig2[j]) > thr)) continue;
    if (tall) {
      double dot = 0.0;
      for (int i = 0; i < m; i++) dot += W[(size_t)j * rows + i] * b[i];
      const double f = dot / sig2[j];
      for (int i = 0; i < n; i++) x[i] += R[(size_t)j * cols + i] * f;
    } else {
      double dot = 0.0;
      for (int i = 0; i < m; i++) dot += R[(size_t)j * cols + i] * b[i];
      const double f = dot / sig2[j];
      for (int i = 0; i < n; i++) x[i] += W[(size_t)j * rows + i] * f;
    }
  }
}

std::vector<double> old_pinv(const CovFit& fit) {
  const int m = fit.m;
  std::vector<double> A((size_t)m * 10), pinv((size_t)10 * m, 0.0), e(m, 0.0);
  for (int s = 0; s < m; s++) {
    const double x = fit.offsets[3 * (size_t)s], y = fit.offsets[3 * (size_t)s + 1], z = fit.offsets[3 * (size_t)s + 2];
    double* r = A.data() + (size_t)s * 10;
    r[0] = x * x; r[1] = y * y; r[2] = z * z; r[3] = x * y; r[4] = y * z; r[5] = z * x;
    r[6] = x; r[7] = y; r[8] = z; r[9] = 1.0;
  }
  double q[10];
  for (int s = 0; s < m; s++) {
    e[s] = 1.0;
    old_lstsq_jacobi(A, e, m, 10, q);
    e[s] = 0.0;
    for (int k = 0; k < 10; k++) pinv[(size_t)k * m + s] = q[k];
  }
  return pinv;
}

void print(const char* name, const double* v, size_t n) {
  std::printf("%s", name);
  for (size_t i = 0; i < n; i++) std::printf(" %a", v[i]);
  std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: covfit_check fit|old|time n xy_half yaw_half ...\n"); return 2; }
  const int n = std::atoi(argv[2]);
  const double xy_half = std::strtod(argv[3], nullptr), yaw_half = std::strtod(argv[4], nullptr);
  if (n < 1 || n > 15) { std::fprintf(stderr, "n out of range\n"); return 2; }
  CovFit fit;
  if (!std::strcmp(argv[1], "time")) {
    const int reps = argc > 5 ? std::atoi(argv[5]) : 3;
    double best = 1e300;
    for (int r = 0; r < reps; r++) {
      const auto t0 = std::chrono::steady_clock::now();
      fit.prepare(n, xy_half, yaw_half);
      best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("seconds %.9g\n", best);
    return fit.pinv.size() == (size_t)10 * n * n * n ? 0 : 1;
  }
  fit.prepare(n, xy_half, yaw_half);
  if (!std::strcmp(argv[1], "old")) {
    const std::vector<double> p = old_pinv(fit);
    print("pinv", p.data(), p.size());
    return 0;
  }
  if (std::strcmp(argv[1], "fit") || argc < 7) { std::fprintf(stderr, "bad arguments\n"); return 2; }
  const double score_scale = std::strtod(argv[5], nullptr), scaler = std::strtod(argv[6], nullptr);
  std::vector<double> costs;
  char tok[128];
  while ((int)costs.size() < fit.m && std::scanf("%127s", tok) == 1) costs.push_back(std::strtod(tok, nullptr));
  if ((int)costs.size() != fit.m) { std::fprintf(stderr, "expected %d costs, read %zu\n", fit.m, costs.size()); return 2; }
  double cov36[36];
  for (int k = 0; k < 36; k++) cov36[k] = 0.0;
  const bool ok = fit.solve(costs.data(), score_scale, scaler, cov36);
  print("offsets", fit.offsets.data(), fit.offsets.size());
  print("pinv", fit.pinv.data(), fit.pinv.size());
  std::printf("verdict %d\n", ok ? 1 : 0);
  print("cov36", cov36, 36);
  return 0;
}
