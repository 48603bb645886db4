// The trajectory-evaluation entry of include/cfear_hip.hpp (EvalTrajectories) compiled with the reference-side stand-ins:
// a syntax check of the header and the host helpers it is fed from on a host without a GPU (tests/test_kitti_eval_cpu.py);
// tests/test_gpu_kitti_eval.py runs it and reads the line it prints: pairs, rows, status, ATE, det of the alignment.
#include <cstdio>

#include "cfear_hip.hpp"

int main() {
  try {
    const double xyt[9] = {0.0, 0.0, 0.0, 1.0, 0.5, 0.1, 2.0, -0.5, 0.2};
    double xyt_est[9];
    for (int i = 0; i < 9; i++) xyt_est[i] = xyt[i] * (i % 3 == 2 ? 1.0 : 1.01);
    std::vector<double> poses(36), est(36);
    if (cfear_kitti_from_xyt(xyt, 3, 3, poses.data()) != CFEAR_OK || cfear_kitti_from_xyt(xyt_est, 3, 3, est.data()) != CFEAR_OK) return 1;
    CFEAR_Radarodometry::Context ctx;
    std::vector<cfear_eval_row> rows;
    const std::vector<cfear_eval_summary> s = EvalTrajectories(ctx, {est}, {poses}, nullptr, &rows);
    const double* r = s[0].align;
    const double det = r[0] * (r[5] * r[10] - r[6] * r[9]) - r[1] * (r[4] * r[10] - r[6] * r[8]) + r[2] * (r[4] * r[9] - r[5] * r[8]);
    printf("%d %d %d %.17g %.17g\n", (int)s.size(), (int)rows.size(), (int)s[0].status, s[0].ate, det);
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
