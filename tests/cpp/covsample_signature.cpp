// The device-side covariance sampling entries of include/cfear_hip.h (cfear_cov_fit_records,
// cfear_covariance_by_sampling_candidates, cfear_verify_sample_covariances) and their C++ mirror (CovFitRecords,
// n_scan_normal_reg::CovarianceBySamplingCandidates, VerifySampleCovariances in include/cfear_hip.hpp) compiled as C++14 with
// the reference-side stand-ins: a signature check on a host without a GPU (tests/test_cov_device_cpu.py).  Without a context
// the calls validate their arguments and refuse, so the program also runs there: per line it prints the status and the
// message of a fit with 16 samples per axis, of a good fit call (refused for the missing context only), of a verified list
// whose second candidate has to >= from, and of a good list over graphs without a table.  With an argument it goes through
// the wrappers, which need a device.
#include <cstddef>
#include <cstdio>

#include "cfear_hip.hpp"

static_assert(sizeof(cfear_reg_result) == 72 && sizeof(cfear_candidate) == 56 && sizeof(cfear_cov_sampling_params) == 32,
              "records of the sampling pass");
static_assert(sizeof(cfear_verify_result) == 480 && offsetof(cfear_verify_result, cov) == 24 && offsetof(cfear_verify_result, cov_sampled) == 396 &&
                  offsetof(cfear_verify_result, reg) == 408,
              "cfear_verify_result layout");

// the three declarations, as function pointers of the types the issue gives
static int (*const kFit)(cfear_ctx*, const cfear_reg_result*, const cfear_reg_result*, int32_t, const cfear_cov_sampling_params*, double*,
                         int32_t*) = &cfear_cov_fit_records;
static int (*const kCands)(cfear_ctx*, const cfear_scan_table*, const cfear_candidate*, int32_t, const cfear_reg_params*, const cfear_reg_result*,
                           const cfear_cov_sampling_params*, double*, int32_t*) = &cfear_covariance_by_sampling_candidates;
static int (*const kVerified)(cfear_ctx*, const cfear_loop_graphs*, const cfear_loop_verify_candidate*, int32_t, const cfear_loop_verify_params*,
                              cfear_verify_result*) = &cfear_verify_sample_covariances;

static int through_the_wrappers() {
  try {
    CFEAR_Radarodometry::Context ctx;
    cfear_cov_sampling_params sp;
    cfear_cov_sampling_params_default(&sp);
    std::vector<double> cov;
    std::vector<int32_t> ok;
    CFEAR_Radarodometry::CovFitRecords(ctx, {}, {}, sp, cov, ok);
    LoopVerifyGraphs graphs;
    graphs.AddGraph({}, {}, {});
    LoopVerifyOutput out;
    VerifySampleCovariances(ctx, graphs, out);
    printf("%d %d\n", (int)cov.size(), (int)out.results.size());
  } catch (const CFEAR_Radarodometry::CfearError& e) {
    fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  return 0;
}

int main(int argc, char**) {
  if (argc > 1) return through_the_wrappers();
  cfear_cov_sampling_params sp;
  cfear_cov_sampling_params_default(&sp);
  cfear_reg_result regs[2] = {}, samples[54] = {};
  double cov[72];
  int32_t ok[2];
  sp.samples_per_axis = 16;
  int rc = kFit(nullptr, regs, samples, 2, &sp, cov, ok);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  sp.samples_per_axis = 3;
  rc = kFit(nullptr, regs, samples, 2, &sp, cov, ok);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  cfear_loop_verify_params par;
  cfear_loop_verify_params_default(&par);
  const int32_t node_off[3] = {0, 2, 5};
  const double poses[5][3] = {};
  cfear_loop_graphs g = cfear_loop_graphs();
  g.n_graphs = 2; g.node_off = node_off; g.poses_xyt = &poses[0][0];
  cfear_loop_verify_candidate list[2] = {{1, 2, 0, 0, 7, 0, {0, 0, 0}, 0.1, 0.0}, {0, 1, 1, 0, 1, 0, {0, 0, 0}, 0.1, 0.0}};
  cfear_verify_result res[2] = {};
  rc = kVerified(nullptr, &g, list, 2, &par, res);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  list[1].to = 0;
  rc = kVerified(nullptr, &g, list, 2, &par, res);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  rc = kCands(nullptr, nullptr, nullptr, 0, nullptr, regs, &sp, cov, ok);
  printf("%d %s\n", rc, cfear_last_error(nullptr));
  printf("%g %g %d %g\n", par.verify.sampling.xy_range, par.verify.sampling.yaw_range, (int)par.verify.sampling.samples_per_axis,
         par.verify.sampling.covariance_scaler);
  return 0;
}
