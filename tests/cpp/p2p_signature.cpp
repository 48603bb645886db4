// The p2pQuality, keypointRepetability and scanEvaluator mirrors of include/cfear_hip.hpp in the reference's call shape
// (AlignmentQuality.h:119-150: (ref, src, par, Toffset), GetQualityMeasure / GetResiduals; ScanEvaluator.h:21-137:
// CreatePerturbations, SaveEvaluation, datapoint::HeaderToString / ValsToString / aligned): a syntax check of the header.
// Run with a file of clouds (int32 n_scans, then per scan: int32 n, float64 pose[3], float32 [n][4]) and an output path it
// scores scan 1 against scan 0 at the offset given and writes eval.txt of the sequence: the GPU test compares both with Python.
#include <cstdio>
#include <cstdlib>

#include "cfear_hip.hpp"

using CorAlignment::AlignmentQuality;
using CorAlignment::PoseScan_S;

int main(int argc, char** argv) {
  try {
    if (argc < 3) {                                            // nothing to run: the classes only have to compile
      std::vector<double> (AlignmentQuality::*res)() = &AlignmentQuality::GetResiduals;
      std::vector<double> (AlignmentQuality::*qual)() = &AlignmentQuality::GetQualityMeasure;
      std::vector<double> (CorAlignment::p2pQuality::*pres)() = &CorAlignment::p2pQuality::GetResiduals;
      std::vector<double> (CorAlignment::p2pQuality::*pqual)() = &CorAlignment::p2pQuality::GetQualityMeasure;
      void (CorAlignment::scanEvaluator::*pert)() = &CorAlignment::scanEvaluator::CreatePerturbations;
      void (CorAlignment::scanEvaluator::*save)() = &CorAlignment::scanEvaluator::SaveEvaluation;
      std::vector<std::string> (*header)() = &CorAlignment::datapoint::HeaderToString;
      bool (*aligned)(const std::vector<double>&) = &CorAlignment::datapoint::aligned;
      AlignmentQuality::parameters par;
      CorAlignment::scanEvaluator::parameters epar;
      const std::array<double, 6> T = AlignmentQuality::Tchange({0, 0, 0}, {0, 0, 0}, {0, 0, 0});
      printf("%s | %s %g | %d %g %g %d %g | %g %g %g\n", CorAlignment::Vec2String(header()).c_str(), par.method.c_str(), par.radius,
             epar.scan_spacing, epar.range_error, epar.theta_range, epar.offset_rotation_steps, epar.theta_error, T[0], T[2], T[4]);
      return res && qual && pres && pqual && pert && save && aligned({0, 0, 0}) && !aligned({0.5, 0, 0}) ? 0 : 3;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n_scans = 0;
    if (fread(&n_scans, 4, 1, f) != 1) return 2;
    std::vector<PoseScan_S> scans;
    for (int s = 0; s < n_scans; s++) {
      int32_t n = 0;
      double pose[3];
      if (fread(&n, 4, 1, f) != 1 || fread(pose, 8, 3, f) != 3) return 2;
      PoseScan_S sc = std::make_shared<CorAlignment::PoseScan>();
      sc->cloud.resize((size_t)n);
      if (n && fread(sc->cloud.data(), 16, (size_t)n, f) != (size_t)n) return 2;
      sc->T = CFEAR_Radarodometry::Pose2d{pose[0], pose[1], pose[2]};
      sc->pose_id = 100 + s;
      scans.push_back(sc);
    }
    fclose(f);
    CFEAR_Radarodometry::Context ctx(0);
    AlignmentQuality::parameters par;
    par.method = "P2P";
    par.radius = argc > 3 ? atof(argv[3]) : 3.0;
    const CFEAR_Radarodometry::Pose2d off{0.3, -0.2, 0.01};
    CorAlignment::p2pQuality p2p(ctx, scans[0], scans[1], par, off);
    CorAlignment::keypointRepetability rep(ctx, scans[0], scans[1], par, off);
    const std::vector<double> q = p2p.GetQualityMeasure(), r = rep.GetQualityMeasure(), res = p2p.GetResiduals();
    double tail = 0.0;
    for (double v : res) tail += v;
    printf("%.17g %.17g %.17g\n%.17g %.17g %.17g\n%d %.17g\n", q[0], q[1], q[2], r[0], r[1], r[2], (int)res.size(), tail);
    CorAlignment::scanEvaluator::parameters epar;
    CorAlignment::scanEvaluator ev(ctx, scans, epar, par);
    ev.SaveEvaluation(argv[2]);
    printf("%d %d\n", (int)ev.datapoints_.size(), (int)ev.vek_perturbation_.size());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
