// The replay of include/cfear_hip.hpp (OdometryReplay) compiled with the reference-side stand-ins: a syntax and layout check
// on a host without a GPU (tests/test_replay_abi.py).  It prints the size of the record; without a device the context cannot
// be made and the program exits 2.  With one it replays three frames of a 20 x 20 lattice standing still and prints the
// statuses, the keyframe flags and the number of window scans of every frame.
#include <cstddef>
#include <cstdio>

#include "cfear_hip.hpp"

static_assert(sizeof(cfear_replay_frame) == 160 && offsetof(cfear_replay_frame, dev) == 48 && offsetof(cfear_replay_frame, score) == 72 &&
                  offsetof(cfear_replay_frame, n_points) == 96 && offsetof(cfear_replay_frame, sanity_ok) == 128 &&
                  offsetof(cfear_replay_frame, exposed) == 156,
              "cfear_replay_frame layout");
static_assert(CFEAR_OPT_REPLAY_CHUNK >= CFEAR_OPT_COUNT, "the chunk option is numbered apart from the enum");

int main() {
  using namespace CFEAR_Radarodometry;
  printf("%d\n", (int)sizeof(cfear_replay_frame));
  try {
    Context ctx;
    PointCloud lattice;
    for (int i = 0; i < 400; i++) {
      lattice.emplace_back();
      lattice.back().x = 0.5f * (float)(i % 20) - 5.f;
      lattice.back().y = 0.5f * (float)(i / 20) - 5.f;
      lattice.back().intensity = 100.f;
    }
    cfear_odometry_params par;
    cfear_odometry_params_default(&par);
    const std::vector<Pose2d> trace(3, Pose2d{0, 0, 0});
    const std::vector<cfear_replay_frame> rec = OdometryReplay(ctx, {lattice, lattice, lattice}, trace, par);
    for (const cfear_replay_frame& r : rec) printf("%d %d %d\n", (int)r.reg_status, (int)r.is_keyframe, (int)r.n_targets);
  } catch (const CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
