// The whole-graph Scan Context entry of include/cfear_hip.hpp (DetectLoopClosureSequence) compiled with the reference-side
// stand-ins: a syntax check of the header.  Matrices come from a 4 x 4 type with operator()(row, col), as Eigen's
// GetPose().matrix() and GetPose().inverse().matrix() are on a real host.
#include <cstdio>

#include "cfear_hip.hpp"

struct Mat4 {
  double m[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  double operator()(int r, int c) const { return m[r][c]; }
};

int main() {
  try {
    CFEAR_Radarodometry::Context ctx;
    CFEAR_Radarodometry::PointCloud a(3), b(2);
    Mat4 T, Tinv;
    T.m[0][3] = 2.5;
    Tinv.m[0][3] = -2.5;
    const std::vector<const CFEAR_Radarodometry::PointCloud*> clouds{&a, &b};
    const std::vector<ScNodeRows8> rows{ScNodeRows(Mat4()), ScNodeRows(T)}, inv{ScNodeRows(Mat4()), ScNodeRows(Tinv)};
    const std::vector<std::vector<cfear_sc_candidate>> c = DetectLoopClosureSequence(ctx, clouds, rows, inv, {0, 1}, 1, 1);
    printf("%d\n", (int)c.size());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
