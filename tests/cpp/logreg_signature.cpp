// The LogisticRegression and ScanLearningInterface mirrors of include/cfear_hip.hpp in the reference's call shape
// (alignmentinterface.h:103-119, :127-218): a syntax check of the header.  Run with a file of training rows as SaveData
// writes them ("y,x0,x1,...") it fits them on the GPU and prints the record: the GPU test compares it with the Python fit.
#include <cstdio>

#include "cfear_hip.hpp"

int main(int argc, char** argv) {
  try {
    if (argc < 2) {                                            // nothing to run: the classes only have to compile
      CorAlignment::LogisticRegression clf;
      clf.AddDataPoint({0.5, 1.0, 2.0}, 1.0);
      clf.AddDataPoint({0.1, 0.2, 0.3, 0.4, 0.5, 0.6}, {0.0, 1.0});
      printf("%d rows of %d, valid %d, fit %d\n", (int)clf.y_.size(), (int)clf.cols_, (int)clf.DataValid(), (int)clf.IsFit());
      void (CorAlignment::ScanLearningInterface::*add)(const CorAlignment::ScanLearningInterface::s_scan&) = &CorAlignment::ScanLearningInterface::AddTrainingData;
      void (CorAlignment::ScanLearningInterface::*fit)(const std::string&) = &CorAlignment::ScanLearningInterface::FitModels;
      void (CorAlignment::ScanLearningInterface::*pred)(const CorAlignment::ScanLearningInterface::s_scan&, const CorAlignment::ScanLearningInterface::s_scan&,
                                                        std::map<std::string, double>&) = &CorAlignment::ScanLearningInterface::PredAlignment;
      void (CorAlignment::ScanLearningInterface::*save)(const std::string&) = &CorAlignment::ScanLearningInterface::SaveCoefficients;
      void (CorAlignment::ScanLearningInterface::*load)(const std::string&) = &CorAlignment::ScanLearningInterface::LoadCoefficients;
      return add && fit && pred && save && load ? 0 : 3;
    }
    CFEAR_Radarodometry::Context ctx(0);
    CorAlignment::LogisticRegression clf(ctx);
    clf.LoadData(argv[1]);
    clf.fit();
    printf("%.17g", clf.intercept());
    for (double c : clf.coef()) printf(" %.17g", c);
    const std::array<int64_t, 4> cm = clf.ConfusionMatrix();
    printf("\n%.17g %.17g %d\n", clf.record().objective, clf.Accuracy(), (int)clf.record().iterations);
    printf("%lld %lld %lld %lld\n", (long long)cm[0], (long long)cm[1], (long long)cm[2], (long long)cm[3]);
    if (argc > 2) {                                            // the two text formats round-trip
      clf.SaveCoefficients(argv[2]);
      CorAlignment::LogisticRegression back(ctx);
      back.LoadCoefficients(argv[2]);
      printf("%.17g %d\n", back.predict_linear(std::vector<double>(back.coef().size(), 1.0))[0], (int)back.IsFit());
    }
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
