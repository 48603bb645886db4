// The cen2019features mirror of include/cfear_hip.hpp in the reference's own shape (Utils.h:46: a cv::Mat, a matrix of
// targets, max_points, min_range), compiled against the stand-ins: a syntax check of the header, it proves nothing about
// OpenCV or Eigen.  Run with a file of rows x cols bytes it prints the targets: the GPU test compares them with the restatement.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cfear_hip.hpp"

// what the mirror asks of Eigen::MatrixXd: Ones(rows, cols), cols() and (row, col) access
struct TargetMatrix {
  int r = 0, c = 0;
  std::vector<double> v;
  static TargetMatrix Ones(int rows, int cols) { TargetMatrix m; m.r = rows; m.c = cols; m.v.assign((size_t)rows * cols, 1.0); return m; }
  double& operator()(int i, int j) { return v[(size_t)i * c + j]; }
  int cols() const { return c; }
};

int main(int argc, char** argv) {
  try {
    const int rows = argc > 3 ? atoi(argv[2]) : 8, cols = argc > 3 ? atoi(argv[3]) : 64;
    cv::Mat fft_data(rows, cols);
    if (argc > 3) {
      FILE* f = fopen(argv[1], "rb");
      if (!f || fread(fft_data.data, 1, (size_t)rows * cols, f) != (size_t)rows * cols) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
      fclose(f);
    }
    TargetMatrix targets;
    CorAlignment::cen2019features(fft_data, targets, argc > 4 ? atoi(argv[4]) : 1000, argc > 5 ? atoi(argv[5]) : 0);
    printf("%d\n", targets.cols());
    for (int k = 0; k < targets.cols(); k++) printf("%d %d %g\n", (int)targets(0, k), (int)targets(1, k), targets(2, k));
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
