// The vicinity-closure entry of include/cfear_hip.h compiled as C++14 against the header alone: a signature and layout check
// on a host without a GPU (tests/test_closure_cpu.py).  Without a context the call validates its arguments and refuses, so
// the program also runs there: it prints the status and the failed graph of a batch whose second graph has a negative step,
// then those of a valid batch (refused for the missing context only: failed graph -1).
#include <cstddef>
#include <cstdio>

#include "cfear_hip.h"

static_assert(sizeof(cfear_closure_params) == 40 && offsetof(cfear_closure_params, min_d_travel) == 8 &&
                  offsetof(cfear_closure_params, odom_sigma_error) == 32,
              "cfear_closure_params layout");
static_assert(sizeof(cfear_closure_candidate) == 40 && offsetof(cfear_closure_candidate, eucl) == 8 &&
                  offsetof(cfear_closure_candidate, odom_bounds) == 32,
              "cfear_closure_candidate layout");
static_assert(CFEAR_CLOSURE_TILE % CFEAR_CLOSURE_ORIGINS == 0, "a tile is a whole number of workgroups' origins");

int main() {
  cfear_closure_params par;
  cfear_closure_params_default(&par, CFEAR_CLOSURE_MINI);
  const double positions[5][3] = {{0, 0, 0}, {1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {2, 0, 0}};
  double steps[5] = {1.0, 0.0, 1.0, -1.0, 0.0};
  const int64_t offsets[3] = {0, 2, 5};
  cfear_closure_candidate out[5];
  int32_t failed = 7;
  const int rc_bad = cfear_closure_candidates_batch(nullptr, &positions[0][0], steps, nullptr, offsets, 5, 2, &par, out, &failed);
  printf("%d %d", rc_bad, (int)failed);
  steps[3] = 1.0;
  const int rc_ok = cfear_closure_candidates_batch(nullptr, &positions[0][0], steps, nullptr, offsets, 5, 2, &par, out, &failed);
  printf(" %d %d %g %g %g\n", rc_ok, (int)failed, par.min_d_travel, par.max_d_travel, par.max_d_close);
  return 0;
}
