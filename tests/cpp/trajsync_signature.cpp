// The trajectory-synchronisation entries of include/cfear_hip.hpp (EvalTrajectory) and of the C ABI compiled with the
// reference-side stand-ins.  `refuse <dir>` needs no GPU (tests/test_trajsync_cpu.py): a refusal made on host buffers without
// a context, the collector's bookkeeping, and the estimate-only Save() into <dir>/est/.  `run <dir>` needs one
// (tests/test_gpu_trajsync.py): Save() with a ground truth into <dir>/est/ and <dir>/gt/, Interpolate, and the hand-over of
// GetGtVek() to AddGroundTruth's argument; it prints the sizes before and after.
#include <cstdio>
#include <cstring>

#include "cfear_hip.hpp"

using CFEAR_Radarodometry::EvalTrajectory;
using CFEAR_Radarodometry::Pose2d;
using CFEAR_Radarodometry::poseStamped;

static const int64_t kT0 = 1547000000ll * 1000000000ll;

static poseStamped stamped(int i, int64_t t) {
  poseStamped p(Pose2d{0.5 * i, 0.25 * i, 0.1 * i}, t);
  for (int k = 0; k < 36; k++) p.cov[(size_t)k] = k * (i + 1) * 1e-3;
  return p;
}

// offline_odometry.cpp:134-137: the hand-over must compile as the reference writes it
void SaveAndLabel(EvalTrajectory& eval, CFEAR_Radarodometry::OdometryKeyframeFuser& fuser) {
  eval.Save();
  fuser.AddGroundTruth(eval.GetGtVek());
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = std::string(argv[2]) + "/";
  try {
    EvalTrajectory::Parameters par;
    par.est_output_dir = dir + "est/";
    par.gt_output_dir = dir + "gt/";
    par.sequence = "05.txt";
    if (!strcmp(argv[1], "refuse")) {
      const int64_t es[2] = {kT0 + 5, kT0 + 15}, gs[4] = {kT0, kT0 + 10, kT0 + 9, kT0 + 30};
      const int32_t n_est = 2, n_gt = 4;
      double est[24] = {0}, gt[48] = {0}, est_out[24], gt_out[24];
      int64_t stamps_out[2];
      cfear_sync_row rows[2];
      int32_t count = 0;
      const int rc = cfear_sync_trajectories(nullptr, CFEAR_SYNC_CHAINED, est, es, nullptr, &n_est, gt, gs, nullptr, &n_gt, 1, est_out, gt_out,
                                             stamps_out, rows, &count);
      printf("%d %s\n", rc, cfear_last_error(nullptr));
      EvalTrajectory both(par);
      both.CallbackEigen(stamped(0, kT0), stamped(0, kT0));
      both.CallbackEigen(stamped(1, kT0 + 1), stamped(1, kT0 + 1));
      both.CallbackESTEigen(stamped(2, kT0 + 2));
      printf("%d %d %d\n", (int)both.GetEstVek().size(), (int)both.GetGtVek().size(), (int)both.GetSize());
      EvalTrajectory only(par);
      for (int i = 0; i < 3; i++) only.CallbackESTEigen(stamped(i, kT0 + i * 250000000ll));
      only.Save();
      return 0;
    }
    // 9 estimates at 4 Hz from kT0 on; 70 ground-truth poses at 50 Hz from 0.3 s to 1.68 s
    EvalTrajectory eval(par);
    for (int i = 0; i < 9; i++) eval.CallbackESTEigen(stamped(i, kT0 + i * 250000000ll));
    for (int i = 0; i < 70; i++) eval.CallbackGTEigen(poseStamped(Pose2d{0.04 * i, 0.02 * i, 0.008 * i}, kT0 + 300000000ll + i * 20000000ll));
    poseStamped at;
    const bool inside = eval.Interpolate(kT0 + 500000000ll, at), outside = eval.Interpolate(kT0, at);
    printf("%d %d %d %d\n", (int)eval.GetEstVek().size(), (int)eval.GetGtVek().size(), (int)inside, (int)outside);
    eval.Save();
    const CFEAR_Radarodometry::poseStampedVector& gt = eval.GetGtVek();               // OdometryKeyframeFuser::AddGroundTruth's argument
    printf("%d %d %lld %.17g\n", (int)eval.GetEstVek().size(), (int)gt.size(), (long long)(gt.empty() ? 0 : gt[0].t - kT0),
           gt.empty() ? 0.0 : gt[0].pose[3]);
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
