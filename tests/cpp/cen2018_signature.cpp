// The Cen2018Radar mirror of include/cfear_hip.hpp in the reference's own constructor shape (ScanType.cpp:68: a cv_bridge
// image and two Eigen::Affine3d), compiled against the stand-ins: a syntax check of the header, it proves nothing about
// OpenCV or Eigen.  Run with a file of rows x cols bytes it prints the cloud: the GPU test compares it with the restatement.
#include <cstdio>
#include <cstdlib>

#include "cfear_hip.hpp"

int main(int argc, char** argv) {
  try {
    const int rows = argc > 3 ? atoi(argv[2]) : 8, cols = argc > 3 ? atoi(argv[3]) : 64;
    cv_bridge::CvImagePtr polar(new cv_bridge::CvImage());
    polar->image = cv::Mat(rows, cols);
    polar->image.data = polar->image.store.data();
    if (argc > 3) {
      FILE* f = fopen(argv[1], "rb");
      if (!f || fread(polar->image.data, 1, (size_t)rows * cols, f) != (size_t)rows * cols) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
      fclose(f);
    }
    CorAlignment::Cen2018Radar::Parameters pars;
    pars.compensate = false;
    pars.range_res = 0.0438;
    Eigen::Affine3d T, Tmotion;
    CorAlignment::Cen2018Radar scan(pars, polar, T, Tmotion);
    printf("%d\n", (int)scan.GetCloud().size());
    for (size_t i = 0; i < scan.GetCloud().size(); i++) {
      const CFEAR_Radarodometry::PointXYZI& p = scan.GetCloud()[i];
      printf("%d %d %.9g %.9g %.9g\n", (int)scan.GetTargets()[2 * i], (int)scan.GetTargets()[2 * i + 1], p.x, p.y, p.intensity);
    }
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
