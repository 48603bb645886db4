// The CartesianRadar / CorAlCartQuality mirrors and the factory branch of include/cfear_hip.hpp in the reference's call shape
// (ScanType.cpp:191: (pars, polar, T, Tmotion); AlignmentQuality.h:184-200: (ref, src, par, Toffset), GetQualityMeasure /
// GetResiduals), compiled against the stand-in headers: a syntax check of the header, it proves nothing about OpenCV.
// Run with any argument it scores a sweep against itself and against a shifted copy on the GPU.
#include <cstdio>

#include "cfear_hip.hpp"

using CorAlignment::AlignmentQuality;
using CorAlignment::CartesianRadar;
using CorAlignment::CartesianRadar_S;

int main(int argc, char** argv) {
  try {
    cfear_cart_params cp;
    cfear_cart_params_default(&cp);
    CartesianRadar::Parameters pars;
    AlignmentQuality::parameters par;
    std::vector<double> (CorAlignment::CorAlCartQuality::*qual)() = &CorAlignment::CorAlCartQuality::GetQualityMeasure;
    std::vector<double> (CorAlignment::CorAlCartQuality::*res)() = &CorAlignment::CorAlCartQuality::GetResiduals;
    printf("%g %g %d | %g %d | %d %d\n", cp.radar_resolution, cp.cart_resolution, cp.cart_pixel_width, pars.cart_resolution,
           pars.cart_pixel_width, (int)sizeof(cfear_cart_job), (int)sizeof(cfear_cart_result));
    if (argc < 2) return qual && res && sizeof(cfear_cart_job) == 40 && sizeof(cfear_cart_result) == 16 && sizeof(cfear_cart_params) == 16 ? 0 : 3;
    boost::shared_ptr<cv_bridge::CvImage> polar(new cv_bridge::CvImage());
    polar->image = cv::Mat(400, 256);
    for (size_t k = 0; k < polar->image.store.size(); k++) polar->image.data[k] = (unsigned char)((k * 2654435761u) >> 24);
    const Eigen::Affine3d T = CFEAR_Radarodometry::Pose2dToAffine3d(CFEAR_Radarodometry::Pose2d{1.0, 2.0, 0.3});
    CartesianRadar_S a(new CartesianRadar(pars, polar, T, T)), b(new CartesianRadar(pars, polar, T, T));
    CFEAR_Radarodometry::Context& ctx = CFEAR_Radarodometry::Context::Default();
    CorAlignment::AlignmentQuality_S same = CorAlignment::AlignmentQualityFactory::CreateQualityType(ctx, a, b, par);
    CorAlignment::CorAlCartQuality moved(a, b, par, CFEAR_Radarodometry::Pose2d{0.5, 0.0, 0.01});
    printf("%.17g %.17g %d\n", same->GetQualityMeasure()[0], moved.GetQualityMeasure()[0], (int)moved.GetResiduals().size());
    return same->GetQualityMeasure()[0] == 0.0 && moved.GetQualityMeasure()[0] > 0.0 ? 0 : 4;
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}
