// The raw-sweep RSCManager entry of include/cfear_hip.hpp in the reference's own argument type (a cv::Mat, loopclosure.cpp:
// 573-577), compiled against the cv_bridge stand-in: a syntax check of the header, it proves nothing about OpenCV.
#include <cstdio>

#include "cfear_hip.hpp"

int main() {
  try {
    CFEAR_Radarodometry::Context ctx;
    RSCManager rsc(ctx);
    cv::Mat radar_scan_img(400, 3360);
    rsc.makeAndSaveScancontextAndKeysRadarRaw(radar_scan_img, CFEAR_Radarodometry::Pose2d{0.0, 0.0, 0.0});
    printf("%d\n", (int)rsc.detectLoopClosureID().size());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
