// The tie audit of include/cfear_hip.hpp (MapPointNormal::GetClosestTies, AssociationTies) compiled with the reference-side
// stand-ins: a syntax and layout check on a host without a GPU (tests/test_tieaudit_cpu.py).  It prints the record's size;
// without a device the context cannot be made and the program exits 2.  With one it audits a pair of three-cell scans whose
// target holds a bitwise copy of a cell, and prints the record and the tie group of the first query.
#include <cstddef>
#include <cstdio>

#include "cfear_hip.hpp"

static_assert(sizeof(cfear_tie_record) == 32 && offsetof(cfear_tie_record, max_group) == 20 && offsetof(cfear_tie_record, status) == 24,
              "cfear_tie_record layout");
static_assert(CFEAR_TIE_TILE % 256 == 0, "a tile is staged by whole workgroups");

int main() {
  using namespace CFEAR_Radarodometry;
  printf("%d\n", (int)sizeof(cfear_tie_record));
  try {
    Context ctx;
    std::vector<cfear_cell> cells(3);
    for (size_t i = 0; i < cells.size(); i++) {
      cfear_cell c = {};
      c.mean[0] = i == 2 ? 1.0 : 1.0 + 4.0 * (double)i; c.mean[1] = 0.5;
      c.normal[0] = 1.0; c.cov[0] = 0.1; c.cov[3] = 0.1; c.scale = 1.0; c.avg_intensity = 1.0; c.lambda_min = 1.0; c.lambda_max = 1.0;
      c.nsamples = 7;
      cells[i] = c;
    }
    MapPointNormal tar(ctx, cells), src(ctx, cells);
    const MapPointNormal::ClosestTies g = tar.GetClosestTies(1.25, 0.5, 2.0);
    cfear_reg_params par;
    cfear_reg_params_default(&par);
    std::vector<int32_t> per_query;
    std::vector<int64_t> offsets;
    const std::vector<cfear_tie_record> rec = AssociationTies(ctx, {{&tar, &src}}, {{Pose2d{0, 0, 0}, Pose2d{0.25, 0, 0}}}, par, 1, &per_query, &offsets);
    printf("%d %d %d | %d %d %d %d %d %d %d | %d %d %d | %lld\n", g.lo, g.hi, g.count, (int)rec[0].n_queries, (int)rec[0].n_in_radius,
           (int)rec[0].n_associated, (int)rec[0].n_tied, (int)rec[0].n_tied_effective, (int)rec[0].max_group, (int)rec[0].status,
           (int)per_query[0], (int)per_query[1], (int)per_query[2], (long long)offsets.back());
  } catch (const CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}
