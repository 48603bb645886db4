// The cen2019OrderAudit mirror of include/cfear_hip.hpp, compiled against the stand-ins: a syntax check of the header.  Run with
// a file of rows x cols bytes it prints the record's counts and the targets with their certain flags: the GPU test compares them
// with the restatement.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cfear_hip.hpp"

int main(int argc, char** argv) {
  try {
    const int rows = argc > 3 ? atoi(argv[2]) : 8, cols = argc > 3 ? atoi(argv[3]) : 64;
    std::vector<uint8_t> img((size_t)rows * cols, 0);
    if (argc > 3) {
      FILE* f = fopen(argv[1], "rb");
      if (!f || fread(img.data(), 1, img.size(), f) != img.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
      fclose(f);
    }
    const CorAlignment::Cen2019OrderAudit a = CorAlignment::cen2019OrderAudit(
        CFEAR_Radarodometry::Context::Default(), img.data(), rows, cols, cols, argc > 4 ? atoi(argv[4]) : 1000, argc > 5 ? atoi(argv[5]) : 0);
    printf("%d %d %d %d %d %d\n", a.record.n_targets, a.record.n_targets_certain, a.record.n_band, a.record.n_marks_in, a.record.n_marks_out,
           (int)a.clear());
    for (size_t k = 0; k < a.certain.size(); k++) printf("%d %d %d\n", a.targets[2 * k], a.targets[2 * k + 1], (int)a.certain[k]);
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
