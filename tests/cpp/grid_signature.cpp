// The odometry grid of include/cfear_hip.hpp (OdometryGrid) compiled with the reference-side stand-ins: a syntax check on a
// host without a GPU (tests/test_grid_cpp.py).  The plan is host code and is printed first: two sequences x (CFEAR-3, CFEAR-3
// with k = 12, CFEAR-1) -> "streams sweeps classes derived surface matcher", then a refused grid's reason.  Without a device
// the context cannot be made and the program exits 2.  With one it advances the six streams over two frames of a sweep that
// holds one bright ring and prints the keyframe flags of the first frame and the registration statuses of the second.
#include <cstdio>

#include "cfear_hip.hpp"

int main() {
  using namespace CFEAR_Radarodometry;
  std::vector<cfear_odometry_params> configs(3);
  cfear_odometry_params_preset(&configs[0], CFEAR_PRESET_CFEAR3, CFEAR_DATASET_OXFORD);
  configs[1] = configs[0];
  configs[1].kstrong.k_strongest = 12;
  cfear_odometry_params_preset(&configs[2], CFEAR_PRESET_CFEAR1, CFEAR_DATASET_OXFORD);
  const int rows = 400, cols = 512;
  const OdometryGrid::Plan plan = OdometryGrid::plan(rows, cols, configs, 2);
  printf("%d %d %d %d %d %d\n", (int)plan.streams.size(), (int)plan.totals.n_sweeps, (int)plan.totals.n_classes,
         (int)plan.totals.n_derived_classes, (int)plan.totals.n_surface_groups, (int)plan.totals.n_matcher_groups);
  try {
    std::vector<cfear_odometry_params> bad = configs;
    bad[2].keep_nodes = 1;
    OdometryGrid::plan(rows, cols, bad, 2);
    printf("accepted\n");
  } catch (const CfearError& e) {
    printf("%s\n", e.what());
  }
  fflush(stdout);
  try {
    Context ctx;
    OdometryGrid grid(ctx, rows, cols, configs, 2);
    std::vector<uint8_t> polar((size_t)2 * rows * cols, 0);
    for (int q = 0; q < 2; q++)
      for (int r = 0; r < rows; r++)
        for (int b = 0; b < 3; b++) polar[((size_t)q * rows + r) * cols + 200 + 40 * q + (r % 7) + b] = (uint8_t)(200 - b);
    for (int f = 0; f < 2; f++) {
      const std::vector<cfear_frame_info> info = grid.processFrame(polar.data());
      for (int s = 0; s < grid.size(); s++) printf("%d ", f == 0 ? (int)info[s].keyframe_added : (int)info[s].reg_status);
      printf("\n");
    }
  } catch (const CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
