// The batched Scan Context entry of include/cfear_hip.hpp (DetectLoopClosureBatch) compiled with the reference-side
// stand-ins: a syntax check of the header, next to sc_sequence_signature.cpp.
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
    ScGraph g;
    g.clouds = {&a, &b};
    g.T = {ScNodeRows(Mat4()), ScNodeRows(T)};
    g.Tinv = {ScNodeRows(Mat4()), ScNodeRows(Tinv)};
    g.ids = {0, 1};
    g.n_detect = 1;
    const std::vector<std::vector<std::vector<cfear_sc_candidate>>> c = DetectLoopClosureBatch(ctx, {g, ScGraph(), g}, 1);
    printf("%d\n", (int)c.size());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
