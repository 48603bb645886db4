// The loop-evaluation entries of include/cfear_hip.h compiled as C++14 against the header alone: a signature and layout
// check on a host without a GPU (tests/test_loopeval_cpu.py).  Without a context the calls validate their arguments and
// refuse, so the program also runs there: it prints the status and the failed candidate of a batch whose second candidate
// names a node outside its graph, those of a valid batch (refused for the missing context only), the status and failed
// experiment of a curve batch whose offsets descend, and the defaults.
#include <cstddef>
#include <cstdio>

#include "cfear_hip.h"

static_assert(sizeof(cfear_loop_stats_params) == 40 && offsetof(cfear_loop_stats_params, min_index_gap) == 32, "cfear_loop_stats_params layout");
static_assert(sizeof(cfear_loop_candidate) == 40 && offsetof(cfear_loop_candidate, guess_xyt) == 16, "cfear_loop_candidate layout");
static_assert(sizeof(cfear_loop_row) == 88 && offsetof(cfear_loop_row, close_xy) == 56 && offsetof(cfear_loop_row, id_close) == 72,
              "cfear_loop_row layout");
static_assert(sizeof(cfear_loop_curves_params) == 16 && offsetof(cfear_loop_curves_params, reference_endpoints) == 12,
              "cfear_loop_curves_params layout");
static_assert(sizeof(cfear_loop_curves_result) == 96 && offsetof(cfear_loop_curves_result, confusion) == 48 &&
                  offsetof(cfear_loop_curves_result, status) == 92,
              "cfear_loop_curves_result layout");
static_assert((CFEAR_LOOPEVAL_LDS_ROWS & (CFEAR_LOOPEVAL_LDS_ROWS - 1)) == 0, "the LDS sort runs over a power of two");

int main() {
  cfear_loop_stats_params sp;
  cfear_loop_stats_params_default(&sp);
  const double gt[3][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}};
  const uint8_t has[3] = {1, 1, 1};
  const int64_t offsets[3] = {0, 2, 3};
  cfear_loop_candidate cands[2] = {{0, 1, 0, 0, {0, 0, 0}}, {1, 1, 0, 0, {0, 0, 0}}};
  cfear_loop_row rows[2];
  int64_t failed = 7;
  const int rc_bad = cfear_loop_stats_batch(nullptr, offsets, &gt[0][0], has, 3, 2, cands, 2, &sp, rows, &failed);
  printf("%d %d", rc_bad, (int)failed);
  cands[1].from = 0;
  const int rc_ok = cfear_loop_stats_batch(nullptr, offsets, &gt[0][0], has, 3, 2, cands, 2, &sp, rows, &failed);
  printf(" %d %d", rc_ok, (int)failed);

  cfear_loop_curves_params cp;
  cfear_loop_curves_params_default(&cp);
  const uint8_t y[4] = {1, 0, 1, 0};
  const double score[4] = {0.9, 0.1, 0.8, 0.3};
  const int64_t rows_off[3] = {0, 3, 2};
  double out[6][6];
  cfear_loop_curves_result res[2];
  int32_t failed_exp = 7;
  const int rc_curves = cfear_loop_curves_batch(nullptr, rows_off, y, score, nullptr, 4, 2, &cp, out[0], out[1], out[2], out[3], out[4], out[5],
                                                res, &failed_exp);
  printf(" %d %d %g %g %g %g %d %g %d %d\n", rc_curves, (int)failed_exp, sp.max_distance, sp.max_registration_translation,
         sp.max_registration_rotation_deg, sp.no_loop_distance, (int)sp.min_index_gap, cp.p_threshold, (int)cp.drop_intermediate,
         (int)cp.reference_endpoints);
  return 0;
}
