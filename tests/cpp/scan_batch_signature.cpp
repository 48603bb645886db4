// The scan batch of include/cfear_hip.hpp (ScanBatch) compiled with the reference-side stand-ins: a syntax check on a host
// without a GPU (tests/test_scan_batch_cpu.py).  Without a device the context cannot be made and the program exits 2.  With
// one it builds three scans in one call -- a 20 x 20 lattice, an empty cloud, the lattice again compensated by a small motion
// -- and prints the statuses, the cell counts and whether destroying a borrowed handle was refused.
#include <cstdio>

#include "cfear_hip.hpp"

int main() {
  using namespace CFEAR_Radarodometry;
  try {
    Context ctx;
    PointCloud lattice;
    for (int i = 0; i < 400; i++) {
      lattice.emplace_back();
      lattice.back().x = 0.5f * (float)(i % 20);
      lattice.back().y = 0.5f * (float)(i / 20);
      lattice.back().intensity = 100.f;
    }
    const std::vector<Pose2d> motions = {Pose2d{0, 0, 0}, Pose2d{0, 0, 0}, Pose2d{0.5, 0.1, 0.01}};
    ScanBatch batch(ctx, {lattice, PointCloud(), lattice}, 3.0f, 64, 0, 0, true, motions);
    const int refused = cfear_scan_destroy(const_cast<cfear_scan*>(batch.at(0)->device()));
    printf("%d %d %d | %d %d | %d %d\n", (int)batch.status(0), (int)batch.status(1), (int)batch.status(2), (int)batch.at(0)->GetSize(),
           (int)batch.at(2)->GetSize(), batch.at(1) == nullptr, refused == CFEAR_ERR_INVALID_ARGUMENT);
  } catch (const CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
