// The graph-candidate verification entries of include/cfear_hip.h and their C++ mirror (LoopVerifyGraphs,
// VerifyGraphCandidates, VerifyScRows in include/cfear_hip.hpp) compiled as C++14 with the reference-side stand-ins: a
// signature and layout check on a host without a GPU (tests/test_loop_verify_cpu.py).  Without a context the calls validate
// their arguments and refuse, so the program also runs there: per line it prints the status and the message of a list whose
// second candidate has to >= from, of rows whose n_detect exceeds a graph, and of a good list (refused for the missing
// context only), then the defaults.  With an argument it goes through the wrappers, which need a device.
#include <cstddef>
#include <cstdio>

#include "cfear_hip.hpp"

static_assert(sizeof(cfear_loop_graphs) == 56 && offsetof(cfear_loop_graphs, node_off) == 8 && offsetof(cfear_loop_graphs, rel_xyt) == 48,
              "cfear_loop_graphs layout");
static_assert(sizeof(cfear_loop_verify_candidate) == 64 && offsetof(cfear_loop_verify_candidate, query) == 16 &&
                  offsetof(cfear_loop_verify_candidate, guess_xyt) == 24 && offsetof(cfear_loop_verify_candidate, odom_term) == 56,
              "cfear_loop_verify_candidate layout");
static_assert(sizeof(cfear_loop_verify_params) == 184 && offsetof(cfear_loop_verify_params, odom_sigma_error) == 160 &&
                  offsetof(cfear_loop_verify_params, odometry_coupled_closure) == 180,
              "cfear_loop_verify_params layout");

static int through_the_wrappers() {
  try {
    CFEAR_Radarodometry::Context ctx;
    CFEAR_Radarodometry::PointCloud a(3), b(2);
    LoopVerifyGraphs graphs;
    graphs.AddGraph({&a, &b}, {CFEAR_Radarodometry::Pose2d{0, 0, 0}, CFEAR_Radarodometry::Pose2d{1, 0, 0}}, {CFEAR_Radarodometry::Pose2d{1, 0, 0}});
    graphs.AddGraph({}, {}, {});
    const LoopVerifyOutput none = VerifyGraphCandidates(ctx, graphs, {});
    const LoopVerifyOutput rows = VerifyScRows(ctx, graphs, {}, {}, {0, 0}, 3);
    printf("%d %d\n", (int)none.results.size(), (int)rows.list.size());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}

int main(int argc, char**) {
  if (argc > 1) return through_the_wrappers();
  cfear_loop_verify_params par;
  cfear_loop_verify_params_default(&par);
  const int32_t node_off[3] = {0, 2, 5};
  const int64_t peak_off[6] = {0, 1, 2, 3, 4, 5};
  const float peaks[5][4] = {};
  const double poses[5][3] = {}, rel[5][3] = {};
  cfear_loop_graphs g = cfear_loop_graphs();
  g.n_graphs = 2; g.node_off = node_off; g.peaks_xyzi = &peaks[0][0]; g.peak_off = peak_off; g.poses_xyt = &poses[0][0]; g.rel_xyt = &rel[0][0];
  cfear_loop_verify_candidate cands[2] = {{1, 2, 0, 0, 7, 0, {0, 0, 0}, 0.1, 0.0}, {0, 1, 1, 0, 1, 0, {0, 0, 0}, 0.1, 0.0}};
  cfear_verify_result res[2];
  int rc = cfear_verify_graph_candidates(nullptr, &g, cands, 2, &par, res, nullptr, nullptr);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  const int32_t n_detect[2] = {3, 0};
  cfear_sc_candidate rows[9] = {};
  const int32_t n_out[3] = {0, 0, 0};
  int32_t n = -1;
  rc = cfear_verify_sc_rows(nullptr, &g, rows, n_out, n_detect, 3, &par, res, nullptr, nullptr, &n);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  cands[1].to = 0;
  rc = cfear_verify_graph_candidates(nullptr, &g, cands, 2, &par, res, nullptr, nullptr);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  printf("%g %d %d %d %d %g\n", par.odom_sigma_error, (int)par.verify_via_odometry, (int)par.transl_guess, (int)par.speedup,
         (int)par.odometry_coupled_closure, CFEAR_LOOP_SPEEDUP_ODOM);
  return 0;
}
