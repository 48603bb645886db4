// verify.hip -- loop-candidate verification: the caller that chains the registration path with its two
// alignment-quality measures and turns them into a loop probability.
//
// Restates, for a BATCH of candidates, what the loop-closure thread does per candidate in
// ScanContextClosure::SearchAndAddConstraint (tbv_slam/src/tbv_slam/loopclosure.cpp:658-725):
//   RegisterLoopCandidate (:320-364) -> loopclosure::Register (:35-97)          [matcher_kernel]
//   VerifyLoopCandidate (:365-384) -> VerifyByAlignment (:759-774) ->
//     ScanLearningInterface::PredAlignment (alignmentinterface.cpp:349-367):
//       getCorAlQualityMeasure (:437-456)                                         [coral_kernel]
//       getCFEARQualityMeasure (:459-478) -> CFEARQuality (AlignmentQuality.cpp:330-354)  [matcher_kernel, cost only]
//       combined logistic model -> quality["alignment_quality"]
//   VerificationModel (:220-238) over {odom-bounds, sc-sim, alignment_quality}
//   ApplyConstratins (:261-274): accept by probability, all candidates or the best of each query.
// Three device launches for the whole batch; the classifiers are a dozen multiply-adds per candidate on the host,
// as in the reference.  Coefficients come in through cfear_verify_params; fitting them (sklearn through pybind11 in the
// reference, alignmentinterface.cpp:192-222) is cfear_logreg_fit_batch, csrc/logreg.hip.
#include <chrono>
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "registration.hpp"

extern "C" void cfear_verify_params_default(cfear_verify_params* p) {
  if (!p) return;
  // tbv_slam/model_parameters/trained_alignment_classifier.txt (intercept, then CorAl x 3, CFEAR x 3), loaded by
  // ScanLearningInterface::LoadCoefficients (alignmentinterface.cpp:396-403) in the shipped launch files
  p->align_intercept = -8.42595;
  const double ac[6] = {-15.2287, 7.47573, -0.0680198, -1.74182, 0.0945444, 0.022217};
  for (int k = 0; k < 6; k++) p->align_coef[k] = ac[k];
  // preset of VerificationModel when no classifier was fitted (loopclosure.cpp:224-232)
  p->loop_intercept = 2.67958289;
  p->loop_coef[0] = -2.89398535; p->loop_coef[1] = -9.40230684; p->loop_coef[2] = 0.23891265;
  p->model_threshold = 0.8;                    // loopclosure.h:133
  p->all_candidates = 1;                       // :137
  p->verification_disabled = 0;                // :120
  p->use_covariance_sampling = 0;              // :130
  p->pad = 0;
  cfear_coral_params_default(&p->coral);       // radius 1.0, no intensity weights (alignmentinterface.cpp:444)
  p->sampling.xy_range = 0.4;                  // loopclosure.cpp:108: linspace(-0.2, 0.2)
  p->sampling.yaw_range = 0.0044;              // :109
  p->sampling.samples_per_axis = 3;            // :110
  p->sampling.pad = 0;
  p->sampling.covariance_scaler = 4.0;         // :112
}

// loopclosure::VerifyByOdometry (loopclosure.cpp:776-808): how far the odometry chain between the two nodes says
// they are apart, relative to the distance travelled.  rel_xyt [n][3]: ConstraintsHandler::RelativeMotion(i, i+1)
// for i = to .. from-1 as planar poses.
extern "C" int cfear_verify_by_odometry(const double* rel_xyt, int32_t n, double odom_sigma_error,
                                        int32_t verify_via_odometry, double* similarity) {
  if (!similarity || n < 0 || (n > 0 && !rel_xyt)) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!verify_via_odometry) { *similarity = 1.0; return CFEAR_OK; }             // :777-781
  double T[3] = {0.0, 0.0, 0.0}, trav = 0.0;
  for (int i = 0; i < n; i++) {
    const double* d = rel_xyt + 3 * (size_t)i;
    trav += std::sqrt(d[0] * d[0] + d[1] * d[1]);
    double t[3];
    xyt_compose(T, d, t);
    T[0] = t[0]; T[1] = t[1]; T[2] = t[2];
  }
  const double est = std::sqrt(T[0] * T[0] + T[1] * T[1]);
  const double error = std::max(est - 5.0, 0.0);                                 // within 5 m: always nearby (:792)
  const double rel = error / trav;                                               // n == 0: 0/0, as the reference
  const double prob = std::exp(-rel * rel / (2.0 * odom_sigma_error * odom_sigma_error));
  *similarity = 1.0 - prob;
  return CFEAR_OK;
}

// ---- the device chain (the usual configuration: Register's constant covariance) ---------------------------------------
// Round 5's step was half host time: between the registration and the two quality measures the host read the poses back,
// composed Talign / Tto per candidate, marshalled 4096 CorAl jobs and 4096 cost jobs and uploaded them, and at the end ran
// the classifiers -- 0.5 ms of a 2.1 ms step with the GPU idle.  Now ONE 296-byte record per candidate goes up and the
// whole chain is enqueued at once:  expand -> matcher (Register) -> prepare (Talign, Tto, the cost and CorAl job records,
// the rotated covariance) -> matcher (cost only: CFEARQuality) -> coral_kernel -> finish (feature vector, both logistic
// models) -> ONE read-back of the 480-byte results.  The host keeps what needs a sort: ApplyConstratins.
namespace {

struct VerifyDev {                      // what a candidate needs on the device
  ScanView to, from;
  const float4* from_peaks;
  const float4* to_peaks;
  int32_t n_from, n_to;
  double from_pose[3], t_be_guess[3];
  double sc_sim, odom_bounds;
};

struct VerifyChain {
  const VerifyDev* cand;
  char* reg_jobs;                       // RegJob records, `stride` bytes apart: scans {to, from}, poses {Tto, Tfrom}
  char* cost_jobs;                      // scans {from, to}, poses {Tfrom, Tto'}: feature_vek = {ref, src} (AlignmentQuality.cpp:330-354)
  size_t stride;
  CoralJob* coral_jobs;
  const cfear_reg_result* reg;
  const cfear_reg_result* q;
  const cfear_coral_result* coral;
  cfear_verify_result* out;
  const int32_t* out_index;             // record j's place in `out` (the graph route skips candidates); nullptr: j
  int32_t* first_bad;                   // smallest candidate index whose CorAl job failed (INT_MAX: none)
  int n;
  cfear_verify_params par;
};

// RegisterLoopCandidate's problem (loopclosure.cpp:35-60): scans {to, from}, poses {Tto = Tfrom * t_be, Tfrom}
__global__ __launch_bounds__(256) void verify_expand_kernel(const VerifyChain c) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) *c.first_bad = 0x7fffffff;
  if (j >= c.n) return;
  const VerifyDev& v = c.cand[j];
  RegJob* r = (RegJob*)(c.reg_jobs + (size_t)j * c.stride);
  r->n_scans = 2; r->itr = 0;
  double tto[3];
  xyt_compose(v.from_pose, v.t_be_guess, tto);
#pragma unroll
  for (int k = 0; k < 3; k++) { r->poses[0][k] = tto[k]; r->poses[1][k] = v.from_pose[k]; }
  r->scans[0] = v.to; r->scans[1] = v.from;
}

// Talign = Trevised^-1 * Tto (loopclosure.cpp:90-94), the covariance in that frame (:62-71 constant; :93), and the job records
// of the two quality measures at Tfrom, Tto' = Tfrom * t_be (:367-372; current = from, prev = to)
__global__ __launch_bounds__(256) void verify_prepare_kernel(const VerifyChain c) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= c.n) return;
  const VerifyDev& v = c.cand[j];
  const cfear_reg_result reg = c.reg[j];
  const RegJob* rj = (const RegJob*)(c.reg_jobs + (size_t)j * c.stride);
  cfear_verify_result& r = c.out[c.out_index ? c.out_index[j] : j];
  r.reg = reg;
  r.reg_ok = reg.status == CFEAR_OK ? 1 : 0;
  r.cov_sampled = 0;
  double* C = r.cov;
  if (r.reg_ok) {
    double inv[3];
    xyt_inverse(reg.pose, inv);                          // Trevised^-1
    xyt_compose(inv, rj->poses[0], r.t_be);              // Talign = Trevised^-1 * Tto
    for (int k = 0; k < 36; k++) C[k] = 0.0;
    C[0] = 0.01; C[7] = 0.01; C[35] = 1e-4;                 // n_scan_normal.cpp:171-175
    // reg_cov.block<3,3>(0,0) = R^-1 * block * R^-T: only the x-y part of the block is touched by a yaw rotation
    double sn, cs;
    sincos(inv[2], &sn, &cs);
    const double R[9] = {cs, -sn, 0, sn, cs, 0, 0, 0, 1};
    double B[9], T[9];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) B[a * 3 + b] = C[a * 6 + b];
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
      double t = 0.0;
      for (int k = 0; k < 3; k++) t += R[a * 3 + k] * B[k * 3 + b];
      T[a * 3 + b] = t;
    }
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
      double t = 0.0;
      for (int k = 0; k < 3; k++) t += T[a * 3 + k] * R[b * 3 + k];
      C[a * 6 + b] = t;
    }
  } else {                                                 // Tdiff and Cov keep their initial Identity (:351-353)
    r.t_be[0] = r.t_be[1] = r.t_be[2] = 0.0;
    for (int k = 0; k < 36; k++) C[k] = (k % 7 == 0) ? 1.0 : 0.0;
  }
  double to_pose[3];
  xyt_compose(v.from_pose, r.t_be, to_pose);
  RegJob* qj = (RegJob*)(c.cost_jobs + (size_t)j * c.stride);
  qj->n_scans = 2; qj->itr = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) { qj->poses[0][k] = v.from_pose[k]; qj->poses[1][k] = to_pose[k]; }
  qj->scans[0] = v.from; qj->scans[1] = v.to;
  CoralJob& cj = c.coral_jobs[j];                          // CreateQualityType(scan_curr, scan_prev): ref = current
  cj.ref = v.from_peaks; cj.src = v.to_peaks; cj.n_ref_ptr = nullptr; cj.n_src_ptr = nullptr;
  cj.n_ref = v.n_from; cj.n_src = v.n_to;
#pragma unroll
  for (int k = 0; k < 3; k++) { cj.ref_pose[k] = v.from_pose[k]; cj.src_pose[k] = to_pose[k]; cj.offset[k] = 0.0; }
}

// PredAlignment's feature vector and the two logistic models (alignmentinterface.cpp:349-367, 271-279; loopclosure.cpp:220-238)
__global__ __launch_bounds__(256) void verify_finish_kernel(const VerifyChain c) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= c.n) return;
  const VerifyDev& v = c.cand[j];
  cfear_verify_result& r = c.out[c.out_index ? c.out_index[j] : j];
  const cfear_coral_result co = c.coral[j];
  const cfear_reg_result q = c.q[j];
  if (co.status != CFEAR_OK && co.status != CFEAR_ERR_EMPTY_CLOUD) atomicMin(c.first_bad, j);
  r.coral[0] = co.joint; r.coral[1] = co.sep; r.coral[2] = co.overlap;
  if (q.status == CFEAR_OK) {                               // AlignmentQuality.cpp:344-348
    r.cfear[0] = q.final_cost;
    r.cfear[1] = (double)q.num_residuals;
    r.cfear[2] = (*v.to.n_cells + *v.from.n_cells) / 2.0;
  } else {
    r.cfear[0] = r.cfear[1] = r.cfear[2] = 0.0;             // :349-351
  }
  double z = c.par.align_intercept;                         // predict_linear (alignmentinterface.cpp:271-279)
  for (int k = 0; k < 3; k++) z += c.par.align_coef[k] * r.coral[k];
  for (int k = 0; k < 3; k++) z += c.par.align_coef[3 + k] * r.cfear[k];
  r.alignment_quality = z;
  r.odom_bounds = v.odom_bounds;
  r.sc_sim = v.sc_sim;
  if (c.par.verification_disabled) {
    r.probability = 0.0;                                    // loopclosure.cpp:377
  } else {
    const double zl = c.par.loop_coef[0] * r.odom_bounds + c.par.loop_coef[1] * r.sc_sim + c.par.loop_coef[2] * r.alignment_quality +
                      c.par.loop_intercept;
    r.probability = 1.0 / (1.0 + exp(-zl));
  }
  r.accepted = 0;
  r.rank = 0;
}

// ApplyConstratins per query (candidates sharing `group`): sort by probability, larger first; accept above the threshold, every
// candidate or only the best (loopclosure.cpp:261-274).  The keys are pulled out of the 480-byte records first (the sort then
// walks 16-byte entries); candidate lists arrive grouped by query, so the usual case is one pass over short runs.
// pick (optional, [n], ascending): the records that take part -- groups and results are indexed by pick[i] instead of i.
void apply_constraints_groups(const int32_t* groups, size_t group_stride_bytes, size_t n, const cfear_verify_params* par,
                              cfear_verify_result* results, const int32_t* pick = nullptr) {
  struct Key { int32_t group, index; double prob; };
  std::vector<Key> keys(n);
  bool grouped = true;
  for (size_t i = 0; i < n; i++) {
    const size_t at = pick ? (size_t)pick[i] : i;
    keys[i].group = *(const int32_t*)((const char*)groups + at * group_stride_bytes);
    keys[i].index = (int32_t)at;
    keys[i].prob = results[at].probability;
    grouped = grouped && (i == 0 || keys[i].group >= keys[i - 1].group);
  }
  // NaN (the odom-bounds feature of an empty odometry chain is 0/0) after every finite probability: `a.prob > b.prob` alone is
  // no strict weak order with NaN among the keys (the reference's std::sort is undefined there), and a finite best could lose
  // its place to one.  The stable sort keeps NaN entries in input order; `>` below never accepts them.
  auto by_prob = [](const Key& a, const Key& b) { return a.prob > b.prob || (b.prob != b.prob && a.prob == a.prob); };
  if (!grouped) std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.group < b.group; });
  for (size_t i = 0; i < n;) {
    size_t e = i;
    while (e < n && keys[e].group == keys[i].group) e++;
    std::stable_sort(keys.begin() + (ptrdiff_t)i, keys.begin() + (ptrdiff_t)e, by_prob);
    for (size_t k = i; k < e; k++) {
      cfear_verify_result& r = results[keys[k].index];
      r.rank = (int32_t)(k - i);
      const bool considered = par->all_candidates || k == i;
      r.accepted = considered && r.probability > par->model_threshold ? 1 : 0;
    }
    i = e;
  }
}
void apply_constraints(const cfear_verify_job* jobs, size_t n, const cfear_verify_params* par, cfear_verify_result* results) {
  if (n) apply_constraints_groups(&jobs[0].group, sizeof(cfear_verify_job), n, par, results);
}

// ---- the chain in three parts, shared by the two routes that fill VerifyDev: the host (verify_device_chain, from
// cfear_verify_job records) and the device (verify_graph_route, from the candidates of batched graphs) ------------------
// The chain's own buffers for n candidates, planned before carve(); `out`, `out_index` and `first_bad` are the route's.
void verify_chain_plan(HostStage& st, VerifyChain& c, size_t n) {
  c.stride = reg_job_stride(2);
  c.out_index = nullptr;
  st.piece(c.cand, n * sizeof(VerifyDev));
  st.piece(c.reg_jobs, n * c.stride);
  st.piece(c.cost_jobs, n * c.stride);
  st.piece(c.coral_jobs, n * sizeof(CoralJob));
  st.piece(c.reg, n * sizeof(cfear_reg_result));
  st.piece(c.q, n * sizeof(cfear_reg_result));
  st.piece(c.coral, n * sizeof(cfear_coral_result));
}
// The two matcher launches' parameters and geometry from the largest cell count among the candidates' scans, and the
// matcher's scratch for n candidates.
struct ChainGeometry {
  cfear_reg_params rp, qp;
  int pairs_cap = 1, pairs_cap_q = 1;
  RegLaunchHint hint, hint_q;
  char* scr = nullptr;
};
int verify_chain_geometry(cfear_ctx* ctx, int max_cells, size_t n, ChainGeometry& g) {
  // RegisterLoopCandidate: P2L, Huber 0.1, uniform weights, SetParameters(4, 10) (loopclosure.cpp:56-57); CFEARQuality:
  // n_scan_normal_reg(P2L, Huber, 0.3), fresh -- itr_ = 0 (AlignmentQuality.cpp:330-354)
  cfear_reg_params_default(&g.rp);
  g.rp.cost = CFEAR_P2L; g.rp.max_itr_association = 4; g.rp.max_itr_solver = 10;
  cfear_reg_params_default(&g.qp);
  g.qp.cost = CFEAR_P2L; g.qp.loss_limit = 0.3; g.qp.itr = 0;
  cfear_reg_pair_geometry(&g.rp, max_cells, max_cells, &g.pairs_cap, &g.hint);
  cfear_reg_pair_geometry(&g.qp, max_cells, max_cells, &g.pairs_cap_q, &g.hint_q);
  g.hint_q.small_pairs = false;
  g.scr = (char*)cfear_workspace(ctx, kWsRegScratch, reg_scratch_bytes(std::max(g.pairs_cap, g.pairs_cap_q)) * n);
  if (!g.scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  return CFEAR_OK;
}
// expand -> matcher -> prepare -> matcher (cost only) -> coral -> finish over the n_jobs records at c.cand; cap = the largest
// n_from + n_to among them.  Nothing is read back.
int verify_chain_launch(cfear_ctx* ctx, VerifyChain& c, int32_t n_jobs, int cap, const cfear_verify_params* par, const ChainGeometry& g) {
  c.n = n_jobs; c.par = *par;
  const dim3 grid((unsigned)(((size_t)n_jobs + 255) / 256)), block(256);
  { ProfScope ps(ctx, "verify_glue"); hipLaunchKernelGGL(verify_expand_kernel, grid, block, 0, ctx->stream, c); }
  int rc = cfear_register_launch(ctx, c.reg_jobs, n_jobs, &g.rp, g.pairs_cap, g.scr, (cfear_reg_result*)c.reg, nullptr, c.stride, g.hint);
  if (rc == CFEAR_OK) {
    { ProfScope ps(ctx, "verify_glue"); hipLaunchKernelGGL(verify_prepare_kernel, grid, block, 0, ctx->stream, c); }
    RegCostMode mode;                                        // GetCost at the jobs' own poses
    rc = cfear_register_launch(ctx, c.cost_jobs, n_jobs, &g.qp, g.pairs_cap_q, g.scr, (cfear_reg_result*)c.q, &mode, c.stride, g.hint_q);
  }
  if (rc == CFEAR_OK) rc = cfear_coral_launch_device(ctx, c.coral_jobs, n_jobs, cap, &par->coral, (cfear_coral_result*)c.coral);
  if (rc != CFEAR_OK) return rc;
  { ProfScope ps(ctx, "verify_glue"); hipLaunchKernelGGL(verify_finish_kernel, grid, block, 0, ctx->stream, c); }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int verify_device_chain(cfear_ctx* ctx, const cfear_verify_job* jobs, int32_t n_jobs, const cfear_verify_params* par,
                        cfear_verify_result* results) {
  const size_t n = (size_t)n_jobs;
#ifdef CFEAR_VERIFY_TIMING
  auto t_last = std::chrono::steady_clock::now();
  double t_acc[8] = {0};
  auto mark = [&](int k) { const auto t = std::chrono::steady_clock::now(); t_acc[k] += std::chrono::duration<double, std::micro>(t - t_last).count(); t_last = t; };
#else
  auto mark = [](int) {};
#endif
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // ---- host: one record per candidate; peak clouds that live on the host are staged once each -----------------------
  int32_t first_bad = 0x7fffffff;
  HostStage st(ctx, kWsVerify);
  int max_cells = 0, cap = 1;
  for (size_t j = 0; j < n; j++) {
    const cfear_verify_job& jb = jobs[j];
    if (jb.from_scan->ctx != ctx || jb.to_scan->ctx != ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %zu: scan belongs to another context", j);
    if (jb.n_from < 0 || jb.n_to < 0 || (jb.n_from > 0 && !jb.from_peaks) || (jb.n_to > 0 && !jb.to_peaks))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %zu: null cloud", j);
    if ((long long)jb.n_from + jb.n_to > cfear_coral_max_points())
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "job %zu: %d + %d points exceed %d", j, jb.n_from, jb.n_to, cfear_coral_max_points());
    cap = std::max(cap, jb.n_from + jb.n_to);
    st.cloud_in(jb.from_peaks, jb.n_from);
    st.cloud_in(jb.to_peaks, jb.n_to);
    const int ct = cfear_scan_size(jb.to_scan), cf = cfear_scan_size(jb.from_scan);
    if (ct < 0) return ct;
    if (cf < 0) return cf;
    max_cells = std::max(max_cells, std::max(ct, cf));
  }
  // ---- device buffers: one workspace, carved ---------------------------------------------------------------------------
  VerifyChain c;
  verify_chain_plan(st, c, n);
  // results on the DEVICE (a sharded caller gathers them there): the finish kernel writes them in place, nothing but the error
  // flag comes back, and ApplyConstratins is the caller's (cfear_verify_apply_constraints over the gathered list)
  const bool host_out = st.out(c.out, results, n * sizeof(cfear_verify_result));
  st.piece(c.first_bad, 4);
  ChainGeometry geo;
  CFEAR_CHECK(verify_chain_geometry(ctx, max_cells, n, geo));
  CFEAR_CHECK(st.carve());
  mark(0);
  VerifyDev* hc = (VerifyDev*)st.pinned(n * sizeof(VerifyDev));
  if (!hc) return CFEAR_ERR_HIP;
  for (size_t j = 0; j < n; j++) {
    const cfear_verify_job& jb = jobs[j];
    VerifyDev& v = hc[j];
    v.to = jb.to_scan->view; v.from = jb.from_scan->view;
    v.from_peaks = jb.n_from > 0 ? st.cloud(jb.from_peaks) : nullptr;
    v.to_peaks = jb.n_to > 0 ? st.cloud(jb.to_peaks) : nullptr;
    v.n_from = jb.n_from; v.n_to = jb.n_to;
    for (int k = 0; k < 3; k++) { v.from_pose[k] = jb.from_pose[k]; v.t_be_guess[k] = jb.t_be_guess[k]; }
    v.sc_sim = jb.sc_sim; v.odom_bounds = jb.odom_bounds;
  }
  mark(1);
  // ---- the chain ---------------------------------------------------------------------------------------------------------
  CFEAR_CHECK(st.upload((void*)c.cand, hc, n * sizeof(VerifyDev)));
  CFEAR_CHECK(verify_chain_launch(ctx, c, n_jobs, cap, par, geo));
  mark(2);
  st.back(&first_bad, c.first_bad, 4);
  CFEAR_CHECK(st.finish());
  if (first_bad != 0x7fffffff) {
    cfear_coral_result bad;
    st.fetch(&bad, c.coral + first_bad, sizeof(bad));
    CFEAR_CHECK(st.wait());
    return cfear_set_error(ctx, bad.status, "job %d: %s", first_bad, cfear_status_string(bad.status));
  }
  mark(3);
  if (host_out) apply_constraints(jobs, n, par, results);
  mark(4);
#ifdef CFEAR_VERIFY_TIMING
  fprintf(stderr, "verify us: scan clouds + sizes %.0f | fill records %.0f | enqueue the chain %.0f | kernels + read-back %.0f | ApplyConstratins %.0f\n",
          t_acc[0], t_acc[1], t_acc[2], t_acc[3], t_acc[4]);
#endif
  return CFEAR_OK;
}

// ---- the graph route: VerifyDev filled on the device from the candidates of batched graphs ---------------------------------
// What ScanContextClosure::SearchAndAddConstraint does per candidate before it registers (loopclosure.cpp:653-701), for all
// candidates of a batch of graphs at once and without the host seeing one:
//   rows form only:  sc_rows_scan_kernel    the first candidate of every detector row (one workgroup's prefix sum over n_out)
//                    sc_rows_expand_kernel  row records -> the compacted list in (row, guess_nr) order: from, to, guess_nr,
//                                           the narrowed sc-sim, Tsrcguess, the speedup rule
//   both forms:      graph_skip_scan_kernel every candidate's rank among the registered ones
//                    verify_fill_kernel     list -> VerifyDev (views from the scan table, peaks from peak_off, the pose, and
//                                           VerifyByOdometry over the graph's motions), validation, and the header
//   ONE read-back of the 32-byte header; then the chain of verify_chain_launch over the registered candidates, writing each
//   record at its place in the list, and
//                    graph_list_finish_kernel  the records of the skipped candidates, and the cfear_loop_candidate list
// A list of c candidates costs O(c) host work whatever the graphs' lengths: the odometry chains are walked by the lanes.
constexpr int kNone = 0x7fffffff;

struct GraphHeader {                    // the graph route's one read-back
  int32_t n_list;                       // candidates in the compacted list
  int32_t n_active;                     // of them not skipped: the chain's batch
  int32_t max_points;                   // largest n_from + n_to among those
  int32_t max_cells;                    // largest cell count among their scans
  int32_t first_invalid;                // smallest index of a candidate that cannot be used (kNone: none)
  int32_t first_capacity;               // ... whose two peak clouds exceed cfear_coral_max_points()
  int32_t first_bad_row;                // rows form: smallest row whose n_out lies outside [0, n_candidates]
  int32_t pad;
};
static_assert(sizeof(GraphHeader) == 32, "header record");

struct GraphArgs {
  const ScanView* views;                // [n_nodes] the scan table
  const float4* peaks;                  // [peak_off[n_nodes]]
  const int64_t* peak_off;              // [n_nodes + 1]
  const double* poses;                  // [n_nodes][3]
  const double* rel;                    // [n_nodes][3] or nullptr
  const int32_t* node_off;              // [n_graphs + 1]
  cfear_loop_verify_candidate* list;    // [cap] the compacted list
  int32_t* active_rank;                 // [cap] candidates before j that are not skipped
  int32_t* out_index;                   // [cap] registered candidate a -> its place j in the list
  VerifyDev* cand;                      // [cap] the chain's records, dense over the registered candidates
  GraphHeader* hdr;
  cfear_verify_result* out;             // [cap]
  cfear_loop_candidate* loops;          // [cap] or nullptr
  // rows form
  const cfear_sc_candidate* rows;       // [n_rows][nc]
  const int32_t* n_out;                 // [n_rows]
  const int32_t* det_off;               // [n_graphs + 1] the first row of every graph
  int32_t* row_start;                   // [n_rows] the first candidate of every row
  int32_t n_rows, nc;
  int32_t n_graphs;
  int32_t n_fixed;                      // list form: the list's length; rows form: -1 (hdr->n_list)
  int32_t max_points_allowed;
  int32_t verify_via_odometry, transl_guess, speedup_rule;
  int32_t skipped_rank;                 // -1 for host results, 0 for device results (no selection was made)
  double two_sigma2;
};

__host__ __device__ inline bool fin1(double x) { return fabs(x) <= 1.7976931348623157e308; }
// 0: usable; else an index into kGraphCandFault.  The same test on the host (host lists) and in verify_fill_kernel.
__host__ __device__ inline int graph_cand_fault(const cfear_loop_verify_candidate& c, const int32_t* node_off, int n_graphs) {
  if (c.graph < 0 || c.graph >= n_graphs) return 1;
  const int nn = node_off[c.graph + 1] - node_off[c.graph];
  if (c.from < 0 || c.from >= nn) return 2;
  if (c.to < 0 || c.to >= nn) return 3;
  if (c.to >= c.from) return 4;
  if (c.guess_nr < 0) return 5;
  if (!fin1(c.guess_xyt[0]) || !fin1(c.guess_xyt[1]) || !fin1(c.guess_xyt[2])) return 6;
  if (!fin1(c.sc_sim)) return 7;
  return 0;
}
const char* const kGraphCandFault[] = {"", "its graph does not exist", "its from node does not exist", "its to node does not exist",
                                       "to must lie before from", "guess_nr is negative", "its guess is not finite", "its sc_sim is not finite"};

// Exclusive prefix sums of value(i), i < n, by ONE workgroup of 256 threads, 256 items a round: write(i, sum before i).
// Returns the total in every thread.
template <class V, class W>
__device__ __forceinline__ int block_excl_scan_256(int n, V value, W write) {
  __shared__ int wave_total[4];
  const int wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + (int)threadIdx.x;
    const int v = i < n ? value(i) : 0;
    const int incl = wave_incl_scan_i32(v);
    __syncthreads();                                   // the previous round's readers are done with wave_total
    if ((threadIdx.x & 63) == 63) wave_total[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; w++) before += wave_total[w];
    if (i < n) write(i, before + incl - v);
    carry += ((wave_total[0] + wave_total[1]) + wave_total[2]) + wave_total[3];
  }
  return carry;
}

__global__ __launch_bounds__(256) void sc_rows_scan_kernel(const GraphArgs a) {
  int bad = kNone;
  const int total = block_excl_scan_256(
      a.n_rows,
      [&](int d) {
        const int c = a.n_out[d];
        if (c < 0 || c > a.nc) { bad = min(bad, d); return 0; }
        return c;
      },
      [&](int d, int start) { a.row_start[d] = start; });
  if (bad != kNone) atomicMin(&a.hdr->first_bad_row, bad);
  if (threadIdx.x == 0) a.hdr->n_list = total;
}

// loopclosure.cpp:660-696 for record s of row d
__global__ __launch_bounds__(256) void sc_rows_expand_kernel(const GraphArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)a.n_rows * a.nc) return;
  const int d = (int)(t / a.nc), s = (int)(t % a.nc);
  const int cnt = a.n_out[d];
  if (cnt < 0 || cnt > a.nc || s >= cnt) return;           // a bad row writes nothing (the host refuses it by the header)
  int lo = 0, hi = a.n_graphs;                             // the last graph whose first row is <= d (empty graphs share a first row)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.det_off[mid] <= d) lo = mid; else hi = mid;
  }
  const cfear_sc_candidate r = a.rows[(size_t)d * a.nc + s];
  cfear_loop_verify_candidate c;
  c.graph = lo;
  c.from = d - a.det_off[lo];                              // idx_from = the query node (:660)
  c.to = r.nn_idx;                                         // idx_to (:661)
  c.guess_nr = s;                                          // std::distance(candidates.begin(), itr) (:675)
  c.query = a.node_off[lo] + c.from;
  c.skip = a.speedup_rule && r.min_dist_odom > CFEAR_LOOP_SPEEDUP_ODOM ? 1 : 0;   // :682-688
  const double yaw[3] = {0.0, 0.0, (double)r.yaw_diff_rad};                         // rot_offset: -src_yaw_offset = sc_cand_yaw (:692-694)
  if (a.transl_guess) {                                    // Tsrcguess = Taug^-1 * rot_offset (:695-696)
    double inv[3];
    xyt_inverse(r.Taug, inv);
    xyt_compose(inv, yaw, c.guess_xyt);
  } else {
    c.guess_xyt[0] = yaw[0]; c.guess_xyt[1] = yaw[1]; c.guess_xyt[2] = yaw[2];
  }
  c.sc_sim = c.skip ? r.min_dist : (double)(float)r.min_dist;                       // `const float sc_cand_sim` (:677); :684 passes itr->min_dist
  c.odom_term = r.min_dist_odom;
  a.list[a.row_start[d] + s] = c;
}

__global__ __launch_bounds__(256) void graph_skip_scan_kernel(const GraphArgs a) {
  const int n = a.n_fixed >= 0 ? a.n_fixed : a.hdr->n_list;
  const int total = block_excl_scan_256(
      n, [&](int j) { return a.list[j].skip ? 0 : 1; }, [&](int j, int rank) { a.active_rank[j] = rank; });
  if (threadIdx.x == 0) { a.hdr->n_active = total; a.hdr->n_list = n; }
}

// One lane per candidate: the VerifyDev record verify_device_chain fills on the host, and quality["odom-bounds"]
__global__ __launch_bounds__(256) void verify_fill_kernel(const GraphArgs a) {
  const int n = a.n_fixed >= 0 ? a.n_fixed : a.hdr->n_list;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const cfear_loop_verify_candidate c = a.list[j];
  if (graph_cand_fault(c, a.node_off, a.n_graphs)) { atomicMin(&a.hdr->first_invalid, j); return; }
  if (c.skip) return;
  const int node0 = a.node_off[c.graph];
  const int kf = node0 + c.from, kt = node0 + c.to;
  const long long nf = a.peak_off[kf + 1] - a.peak_off[kf], nt = a.peak_off[kt + 1] - a.peak_off[kt];
  if (nf + nt > a.max_points_allowed) { atomicMin(&a.hdr->first_capacity, j); return; }
  const int at = a.active_rank[j];
  a.out_index[at] = j;
  VerifyDev& v = a.cand[at];
  v.to = a.views[kt]; v.from = a.views[kf];
  v.from_peaks = nf > 0 ? a.peaks + a.peak_off[kf] : nullptr;
  v.to_peaks = nt > 0 ? a.peaks + a.peak_off[kt] : nullptr;
  v.n_from = (int32_t)nf; v.n_to = (int32_t)nt;
#pragma unroll
  for (int k = 0; k < 3; k++) { v.from_pose[k] = a.poses[3 * (size_t)kf + k]; v.t_be_guess[k] = c.guess_xyt[k]; }
  v.sc_sim = c.sc_sim;
  // VerifyByOdometry(from, to): RelativeMotion(k, k + 1), k = to .. from - 1, of the candidate's graph (:776-806)
  v.odom_bounds = a.verify_via_odometry ? odom_chain_similarity(a.rel + 3 * (size_t)node0, c.to, c.from, a.two_sigma2) : 1.0;
  atomicMax(&a.hdr->max_points, (int)(nf + nt));
  atomicMax(&a.hdr->max_cells, max(*v.to.n_cells, *v.from.n_cells));
}

// After the chain: a skipped candidate's record (UpdateStatistics' row of loopclosure.cpp:684 and a constraint that was never
// registered: Tdiff and Cov keep their Identity), and the candidate list cfear_loop_stats_batch takes
__global__ __launch_bounds__(256) void graph_list_finish_kernel(const GraphArgs a) {
  const int n = a.n_fixed >= 0 ? a.n_fixed : a.hdr->n_list;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const cfear_loop_verify_candidate c = a.list[j];
  cfear_verify_result& r = a.out[j];
  if (c.skip) {
    double* w = (double*)&r;
    for (int k = 0; k < (int)(sizeof(cfear_verify_result) / 8); k++) w[k] = 0.0;
    for (int k = 0; k < 36; k += 7) r.cov[k] = 1.0;
    r.alignment_quality = -20.0;
    r.odom_bounds = c.odom_term;
    r.sc_sim = c.sc_sim;
    r.rank = a.skipped_rank;
  }
  if (a.loops) {
    cfear_loop_candidate l;
    l.graph = c.graph; l.from = c.from; l.to = c.to; l.guess_nr = c.guess_nr;
    l.guess_xyt[0] = r.t_be[0]; l.guess_xyt[1] = r.t_be[1]; l.guess_xyt[2] = r.t_be[2];
    a.loops[j] = l;
  }
}
static_assert(sizeof(cfear_verify_result) % 8 == 0 && sizeof(cfear_loop_verify_candidate) == 64 && sizeof(cfear_loop_verify_params) == 184 &&
                  sizeof(cfear_loop_graphs) == 56,
              "records of the graph route");

struct GraphRows {                      // the rows form's inputs; rows == nullptr: the list form
  const cfear_sc_candidate* rows = nullptr;
  const int32_t* n_out = nullptr;
  const int32_t* n_detect = nullptr;
  int32_t nc = 0;
};

// Everything that can be refused without a device, in the order the header gives.  n_nodes, n_rows and the rows' first row per
// graph come back for the route.
int graph_route_check(cfear_ctx* ctx, const cfear_loop_graphs* g, const cfear_loop_verify_candidate* cands, int32_t n_cand,
                      const GraphRows& rw, const cfear_loop_verify_params* par, const void* results, const void* list_out,
                      const void* loops_out, const int32_t* n_list, std::vector<int32_t>& det_off, int64_t* n_cap) {
  const auto refuse = [&](const char* what) { return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%s", what); };
  if (!g || !par || n_cand < 0) return refuse("null or negative argument");
  if (g->n_graphs < 0 || !g->node_off) return refuse("null or negative argument (node_off holds n_graphs + 1 entries)");
  if (cfear_is_device_ptr(g->node_off) || cfear_is_device_ptr(g->peak_off) || cfear_is_device_ptr(g->poses_xyt) || cfear_is_device_ptr(g->rel_xyt) ||
      cfear_is_device_ptr(rw.n_detect))
    return refuse("node_off, peak_off, poses_xyt, rel_xyt and n_detect must be host memory");
  if (par->verify.use_covariance_sampling) return refuse("use_covariance_sampling is not available for candidates verified on the device");
  if (par->verify_via_odometry && !(par->odom_sigma_error == par->odom_sigma_error)) return refuse("odom_sigma_error is NaN");
  const int G = g->n_graphs;
  if (g->node_off[0] != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph 0: node_off must start at 0");
  for (int gi = 0; gi < G; gi++)
    if (g->node_off[gi + 1] < g->node_off[gi]) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: node_off descends", gi);
  const int N = g->node_off[G];
  if (N > 0 && (!g->peak_off || !g->poses_xyt)) return refuse("null peak_off or poses_xyt with nodes");
  if (N > 0 && par->verify_via_odometry && !g->rel_xyt) return refuse("rel_xyt may be null only with verify_via_odometry = 0");
  if (N > 0 && g->peak_off[0] != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph 0, node 0: peak_off must start at 0");
  for (int gi = 0; gi < G; gi++)
    for (int k = g->node_off[gi]; k < g->node_off[gi + 1]; k++) {
      const int kk = k - g->node_off[gi];
      if (g->peak_off[k + 1] < g->peak_off[k] || g->peak_off[k + 1] - g->peak_off[k] > INT32_MAX)
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: peak_off descends (or more than 2^31 - 1 points)", gi, kk);
      const double* p = g->poses_xyt + 3 * (size_t)k;
      if (!fin1(p[0]) || !fin1(p[1]) || !fin1(p[2]))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: a pose that is not finite", gi, kk);
      if (par->verify_via_odometry && k + 1 < g->node_off[gi + 1]) {
        const double* r = g->rel_xyt + 3 * (size_t)k;
        if (!fin1(r[0]) || !fin1(r[1]) || !fin1(r[2]))
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: a relative motion that is not finite", gi, kk);
      }
    }
  if (N > 0 && g->peak_off[N] > 0 && !g->peaks_xyzi) return refuse("null peaks_xyzi with points");
  if (rw.rows || rw.n_out || n_list) {                     // the rows form
    if (!n_list) return refuse("null n_list");
    if (rw.nc < 1) return refuse("n_candidates must be at least 1");
    det_off.assign((size_t)G + 1, 0);
    for (int gi = 0; gi < G; gi++) {
      const int nn = g->node_off[gi + 1] - g->node_off[gi], nd = rw.n_detect ? rw.n_detect[gi] : nn;
      if (nd < 0 || nd > nn) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: n_detect %d outside [0, %d]", gi, nd, nn);
      det_off[(size_t)gi + 1] = det_off[(size_t)gi] + nd;
    }
    const int D = det_off[(size_t)G];
    if ((int64_t)D * rw.nc > INT32_MAX) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 - 1 row records");
    *n_cap = (int64_t)D * rw.nc;
    if (D > 0 && (!rw.rows || !rw.n_out)) return refuse("null rows or n_out with detected nodes");
    if (D > 0 && memory_kind({rw.rows, rw.n_out}) < 0) return refuse("rows and n_out must be both host or both device memory");
    if (D > 0 && memory_kind({rw.rows}) == 0)
      for (int gi = 0; gi < G; gi++)
        for (int d = det_off[(size_t)gi]; d < det_off[(size_t)gi + 1]; d++) {
          const int from = d - det_off[(size_t)gi];
          if (rw.n_out[d] < 0 || rw.n_out[d] > rw.nc)
            return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: n_out %d outside [0, %d]", gi, from, rw.n_out[d], rw.nc);
          for (int s = 0; s < rw.n_out[d]; s++) {
            const cfear_sc_candidate& r = rw.rows[(size_t)d * rw.nc + s];
            const bool finite = fin1(r.min_dist) && fin1(r.min_dist_odom) && fin1((double)r.yaw_diff_rad) && fin1(r.Taug[0]) && fin1(r.Taug[1]) && fin1(r.Taug[2]);
            if (r.nn_idx < 0 || r.nn_idx >= from || !finite)
              return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: candidate %d %s", gi, from, s,
                                     finite ? "names a node that is not before its query" : "is not finite");
          }
        }
  } else {
    *n_cap = n_cand;
    if (n_cand > 0 && !cands) return refuse("null candidates with a positive count");
    if (n_cand > 0 && !cfear_is_device_ptr(cands))
      for (int j = 0; j < n_cand; j++) {
        const int f = graph_cand_fault(cands[j], g->node_off, G);
        if (f) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d: %s", j, kGraphCandFault[f]);
      }
  }
  if (*n_cap > 0 && !results) return refuse("null results with candidates");
  if (memory_kind({results, loops_out}) < 0) return refuse("loops_out must lie in the memory of results");
  (void)list_out;
  if (N > 0 && !g->table) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null scan table: it must hold one entry per node (%d)", N);
  if (g->table && (int)g->table->n_cells.size() != N)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "the scan table holds %d scans, the graphs %d nodes", (int)g->table->n_cells.size(), N);
  if (!ctx) return refuse("null context");
  if (g->table && g->table->ctx != ctx) return refuse("the scan table belongs to another context");
  return CFEAR_OK;
}

int verify_graph_route(cfear_ctx* ctx, const cfear_loop_graphs* g, const cfear_loop_verify_candidate* cands, int32_t n_cand,
                       const GraphRows& rw, const cfear_loop_verify_params* par, cfear_verify_result* results,
                       cfear_loop_verify_candidate* list_out, cfear_loop_candidate* loops_out, int32_t* n_list) {
  if (n_list) *n_list = 0;
  std::vector<int32_t> det_off;
  int64_t n_cap = 0;
  CFEAR_CHECK(graph_route_check(ctx, g, cands, n_cand, rw, par, results, list_out, loops_out, n_list, det_off, &n_cap));
  if (g->n_graphs == 0 || n_cap == 0) return CFEAR_OK;
  const bool rows_form = !det_off.empty();
  const size_t cap = (size_t)n_cap, N = (size_t)g->node_off[g->n_graphs], G = (size_t)g->n_graphs;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsVerify);
  GraphArgs a{};
  a.views = g->table->d_views.get();
  const float* d_peaks = nullptr;
  st.in(d_peaks, g->peaks_xyzi, (size_t)g->peak_off[N] * 16);
  st.in(a.peak_off, g->peak_off, (N + 1) * 8);
  st.in(a.poses, g->poses_xyt, N * 24);
  if (par->verify_via_odometry) st.in(a.rel, g->rel_xyt, N * 24);
  st.in(a.node_off, g->node_off, (G + 1) * 4);
  if (rows_form) {
    a.n_rows = det_off[G]; a.nc = rw.nc;
    st.in(a.rows, rw.rows, cap * sizeof(cfear_sc_candidate));
    st.in(a.n_out, rw.n_out, (size_t)a.n_rows * 4);
    st.piece(a.det_off, (G + 1) * 4);
    st.piece(a.row_start, (size_t)a.n_rows * 4);
  }
  // outputs of the caller in host memory get a piece and ONE copy-back of the records that were written
  const bool host_out = st.is_host(results);
  const bool host_list = list_out && st.is_host(list_out), host_loops = loops_out && host_out;
  const bool host_cands = !rows_form && st.is_host(cands);
  if (host_out) st.piece(a.out, cap * sizeof(cfear_verify_result)); else a.out = results;
  st.piece(a.list, cap * sizeof(cfear_loop_verify_candidate));   // a device list_out is written at the end: a refusal leaves it alone
  if (host_loops) st.piece(a.loops, cap * sizeof(cfear_loop_candidate)); else a.loops = loops_out;
  st.piece(a.active_rank, cap * 4);
  st.piece(a.out_index, cap * 4);
  st.piece(a.hdr, sizeof(GraphHeader));
  VerifyChain c;
  verify_chain_plan(st, c, cap);
  st.piece(c.first_bad, 4);
  CFEAR_CHECK(st.carve());
  a.peaks = (const float4*)d_peaks;
  a.cand = (VerifyDev*)c.cand;
  a.n_graphs = g->n_graphs;
  a.n_fixed = rows_form ? -1 : n_cand;
  a.max_points_allowed = cfear_coral_max_points();
  a.verify_via_odometry = par->verify_via_odometry;
  a.transl_guess = par->transl_guess;
  a.speedup_rule = par->speedup && par->odometry_coupled_closure;
  a.skipped_rank = host_out ? -1 : 0;
  a.two_sigma2 = 2.0 * par->odom_sigma_error * par->odom_sigma_error;
  // ---- the small records: the header, the rows' first row per graph --------------------------------------------------------
  const size_t rec_bytes = sizeof(GraphHeader) + (rows_form ? (G + 1) * 4 : 0);
  char* rec = (char*)st.record(rec_bytes);
  GraphHeader* h0 = (GraphHeader*)rec;
  h0->first_invalid = h0->first_capacity = h0->first_bad_row = kNone;
  CFEAR_CHECK(st.upload(a.hdr, h0, sizeof(GraphHeader)));
  const dim3 block(256), grid_cap((unsigned)((cap + 255) / 256));
  if (rows_form) {
    memcpy(rec + sizeof(GraphHeader), det_off.data(), (G + 1) * 4);
    CFEAR_CHECK(st.upload((void*)a.det_off, rec + sizeof(GraphHeader), (G + 1) * 4));
    ProfScope ps(ctx, "verify_graph_fill");
    hipLaunchKernelGGL(sc_rows_scan_kernel, dim3(1), block, 0, ctx->stream, a);
    hipLaunchKernelGGL(sc_rows_expand_kernel, grid_cap, block, 0, ctx->stream, a);
  } else if (host_cands) {
    CFEAR_CHECK(st.upload(a.list, cands, cap * sizeof(cfear_loop_verify_candidate)));
  } else {
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(a.list, cands, cap * sizeof(cfear_loop_verify_candidate), hipMemcpyDeviceToDevice, ctx->stream));
  }
  {
    ProfScope ps(ctx, "verify_graph_fill");
    hipLaunchKernelGGL(graph_skip_scan_kernel, dim3(1), block, 0, ctx->stream, a);
    hipLaunchKernelGGL(verify_fill_kernel, grid_cap, block, 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  GraphHeader hdr;
  st.fetch(&hdr, a.hdr, sizeof(hdr));
  CFEAR_CHECK(st.wait());
  // ---- the device's refusals: nothing has been written to the caller's outputs yet ------------------------------------------
  if (hdr.first_bad_row != kNone)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "row %d: n_out outside [0, %d]", hdr.first_bad_row, rw.nc);
  if (hdr.first_invalid != kNone)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d: its graph, from, to, guess_nr, guess or sc_sim are not usable", hdr.first_invalid);
  if (hdr.first_capacity != kNone)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "candidate %d: its two peak clouds exceed %d points", hdr.first_capacity, cfear_coral_max_points());
  const size_t n = (size_t)hdr.n_list;
  if (n == 0) return st.finish();
  // ---- the chain, with the geometry verify_device_chain takes for the same jobs -----------------------------------------------
  int32_t first_bad = kNone;
  if (hdr.n_active > 0) {
    ChainGeometry geo;
    CFEAR_CHECK(verify_chain_geometry(ctx, hdr.max_cells, (size_t)hdr.n_active, geo));
    c.out = a.out;
    c.out_index = a.out_index;
    CFEAR_CHECK(verify_chain_launch(ctx, c, hdr.n_active, std::max(1, hdr.max_points), &par->verify, geo));
    st.back(&first_bad, c.first_bad, 4);
  }
  {
    ProfScope ps(ctx, "verify_graph_fill");
    hipLaunchKernelGGL(graph_list_finish_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  std::vector<cfear_loop_verify_candidate> own_list;       // ApplyConstratins needs the queries and the skip flags
  const cfear_loop_verify_candidate* hl = list_out;
  if (host_out) st.back(results, a.out, n * sizeof(cfear_verify_result));
  if (host_list) st.back(list_out, a.list, n * sizeof(cfear_loop_verify_candidate));
  else if (list_out)
    CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(list_out, a.list, n * sizeof(cfear_loop_verify_candidate), hipMemcpyDeviceToDevice, ctx->stream));
  if (host_loops) st.back(loops_out, a.loops, n * sizeof(cfear_loop_candidate));
  if (host_out && !host_list) {
    own_list.resize(n);
    st.back(own_list.data(), a.list, n * sizeof(cfear_loop_verify_candidate));
    hl = own_list.data();
  }
  CFEAR_CHECK(st.finish());
  if (first_bad != kNone) {
    cfear_coral_result bad;
    int32_t at = 0;
    st.fetch(&bad, c.coral + first_bad, sizeof(bad));
    st.fetch(&at, a.out_index + first_bad, 4);
    CFEAR_CHECK(st.wait());
    return cfear_set_error(ctx, bad.status, "candidate %d: %s", at, cfear_status_string(bad.status));
  }
  if (n_list) *n_list = (int32_t)n;
  if (host_out) {
    std::vector<int32_t> pick;
    pick.reserve(n);
    for (size_t j = 0; j < n; j++)
      if (!hl[j].skip) pick.push_back((int32_t)j);
    if (!pick.empty()) apply_constraints_groups(&hl[0].query, sizeof(cfear_loop_verify_candidate), pick.size(), &par->verify, results, pick.data());
  }
  return CFEAR_OK;
}

}  // namespace

// The chain with the host between its kernels: kept for par.use_covariance_sampling (the sampled covariance is fitted on the
// host from 27 cost samples per candidate, loopclosure.cpp:62-71, 99-208).
static int verify_host_chain(cfear_ctx* ctx, const cfear_verify_job* jobs, int32_t n_jobs,
                             const cfear_verify_params* par, cfear_verify_result* results) {
  const size_t n = (size_t)n_jobs;
#ifdef CFEAR_VERIFY_TIMING
  auto t_last = std::chrono::steady_clock::now();
  double t_acc[8] = {0};
  auto mark = [&](int k) { const auto t = std::chrono::steady_clock::now(); t_acc[k] += std::chrono::duration<double, std::micro>(t - t_last).count(); t_last = t; };
#else
  auto mark = [](int) {};
#endif

  // ---- RegisterLoopCandidate: scans {to, from}, poses {Tto = Tfrom * t_be, Tfrom}; P2L, Huber 0.1, uniform
  // weights, SetParameters(4, 10) (loopclosure.cpp:56-57) ------------------------------------------------------
  cfear_reg_params rp;
  cfear_reg_params_default(&rp);
  rp.cost = CFEAR_P2L;
  rp.max_itr_association = 4;
  rp.max_itr_solver = 10;
  std::vector<const cfear_scan*> handles(2 * n);
  std::vector<double> poses(6 * n);
  std::vector<cfear_reg_job> rj(n);
  for (size_t j = 0; j < n; j++) {
    handles[2 * j] = jobs[j].to_scan;
    handles[2 * j + 1] = jobs[j].from_scan;
    xyt_compose(jobs[j].from_pose, jobs[j].t_be_guess, &poses[6 * j]);
    for (int k = 0; k < 3; k++) poses[6 * j + 3 + k] = jobs[j].from_pose[k];
    rj[j].scans = &handles[2 * j]; rj[j].n_scans = 2; rj[j].pad = 0; rj[j].poses_xyt = &poses[6 * j];
  }
  std::vector<cfear_reg_result> reg(n);
  mark(0);
  int rc = cfear_register_batch(ctx, rj.data(), n_jobs, &rp, reg.data());
  if (rc != CFEAR_OK) return rc;
  mark(1);

  // covariance: Register's constant, or the sampled one (:62-71)
  std::vector<double> cov(36 * n, 0.0);
  std::vector<int32_t> sampled(n, 0);
  if (par->use_covariance_sampling) {
    std::vector<double> posed(poses);                       // T_vek after Register
    for (size_t j = 0; j < n; j++)
      if (reg[j].status == CFEAR_OK) for (int k = 0; k < 3; k++) posed[6 * j + 3 + k] = reg[j].pose[k];
    std::vector<cfear_reg_job> cj(rj);
    for (size_t j = 0; j < n; j++) cj[j].poses_xyt = &posed[6 * j];
    rc = cfear_covariance_by_sampling_batch(ctx, cj.data(), n_jobs, &rp, reg.data(), &par->sampling, cov.data(), nullptr,
                                            sampled.data());
    if (rc != CFEAR_OK) return rc;
  } else {
    for (size_t j = 0; j < n; j++) { cov[36 * j] = 0.01; cov[36 * j + 7] = 0.01; cov[36 * j + 35] = 1e-4; }   // n_scan_normal.cpp:171
  }

  // Talign first: the CorAl jobs need nothing else of this block, and their kernel (the longest of a verification step) then
  // runs while the host rotates the covariances and marshals the cost jobs below
  std::vector<double> inv_yaw(n, 0.0);
  for (size_t j = 0; j < n; j++) {
    cfear_verify_result& r = results[j];
    r.reg = reg[j];
    r.reg_ok = reg[j].status == CFEAR_OK ? 1 : 0;
    r.cov_sampled = r.reg_ok ? sampled[j] : 0;
    if (r.reg_ok) {                                         // loopclosure.cpp:90-94
      double inv[3];
      xyt_inverse(reg[j].pose, inv);                        // Trevised^-1
      xyt_compose(inv, &poses[6 * j], r.t_be);              // Talign = Trevised^-1 * Tto
      inv_yaw[j] = inv[2];
    } else {                                                // Tdiff keeps its initial Identity (:351-353)
      r.t_be[0] = r.t_be[1] = r.t_be[2] = 0.0;
    }
  }

  // ---- VerifyByAlignment at Tfrom, Tto = Tfrom * t_be (loopclosure.cpp:367-372): current = from, prev = to ------
  std::vector<double> to_pose(3 * n);
  for (size_t j = 0; j < n; j++) xyt_compose(jobs[j].from_pose, results[j].t_be, &to_pose[3 * j]);
  std::vector<cfear_coral_job> cjobs(n);
  for (size_t j = 0; j < n; j++) {
    cfear_coral_job& c = cjobs[j];
    c.ref_xyzi = jobs[j].from_peaks; c.n_ref = jobs[j].n_from;      // CreateQualityType(scan_curr, scan_prev): ref = current
    c.src_xyzi = jobs[j].to_peaks; c.n_src = jobs[j].n_to;
    for (int k = 0; k < 3; k++) { c.ref_pose[k] = jobs[j].from_pose[k]; c.src_pose[k] = to_pose[3 * j + k]; c.offset[k] = 0.0; }
  }
  std::vector<cfear_coral_result> coral(n);
  mark(2);
  CoralPending pend(ctx);
  rc = cfear_coral_enqueue(ctx, cjobs.data(), n_jobs, &par->coral, false, pend);
  if (rc != CFEAR_OK) return rc;
  mark(3);

  for (size_t j = 0; j < n; j++) {                          // (the CorAl kernel is running)
    cfear_verify_result& r = results[j];
    double* C = r.cov;
    if (r.reg_ok) {
      for (int k = 0; k < 36; k++) C[k] = cov[36 * j + k];
      // reg_cov.block<3,3>(0,0) = R^-1 * block * R^-T: only the x-y part of the block is touched by a yaw rotation
      const double c = std::cos(inv_yaw[j]), s = std::sin(inv_yaw[j]);
      const double R[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
      double B[9], T[9];
      for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) B[a * 3 + b] = C[a * 6 + b];
      for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
        double t = 0.0;
        for (int k = 0; k < 3; k++) t += R[a * 3 + k] * B[k * 3 + b];
        T[a * 3 + b] = t;
      }
      for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
        double t = 0.0;
        for (int k = 0; k < 3; k++) t += T[a * 3 + k] * R[b * 3 + k];
        C[a * 6 + b] = t;
      }
    } else {                                                // Cov keeps its initial Identity (:351-353)
      for (int k = 0; k < 36; k++) C[k] = (k % 7 == 0) ? 1.0 : 0.0;
    }
  }

  cfear_reg_params qp;                                              // n_scan_normal_reg(P2L, Huber, 0.3), fresh: itr_ = 0
  cfear_reg_params_default(&qp);
  qp.cost = CFEAR_P2L;
  qp.loss_limit = 0.3;
  qp.itr = 0;
  std::vector<const cfear_scan*> qh(2 * n);
  std::vector<double> qposes(6 * n);
  std::vector<cfear_reg_job> qj(n);
  for (size_t j = 0; j < n; j++) {
    qh[2 * j] = jobs[j].from_scan;                                  // feature_vek = {ref, src}
    qh[2 * j + 1] = jobs[j].to_scan;
    for (int k = 0; k < 3; k++) { qposes[6 * j + k] = jobs[j].from_pose[k]; qposes[6 * j + 3 + k] = to_pose[3 * j + k]; }
    qj[j].scans = &qh[2 * j]; qj[j].n_scans = 2; qj[j].pad = 0; qj[j].poses_xyt = &qposes[6 * j];
  }
  std::vector<cfear_reg_result> q(n);
  mark(4);
  rc = cfear_get_cost_batch(ctx, qj.data(), n_jobs, &qp, q.data());   // (same stream: returns after the CorAl kernel too)
  const int rc_coral = cfear_coral_collect(ctx, cjobs.data(), pend, coral.data(), nullptr);
  if (rc != CFEAR_OK) return rc;
  if (rc_coral != CFEAR_OK) return rc_coral;
  mark(5);

  for (size_t j = 0; j < n; j++) {
    cfear_verify_result& r = results[j];
    r.coral[0] = coral[j].joint; r.coral[1] = coral[j].sep; r.coral[2] = coral[j].overlap;
    if (q[j].status == CFEAR_OK) {                                  // AlignmentQuality.cpp:344-348
      r.cfear[0] = q[j].final_cost;
      r.cfear[1] = (double)q[j].num_residuals;
      r.cfear[2] = (cfear_scan_size(jobs[j].to_scan) + cfear_scan_size(jobs[j].from_scan)) / 2.0;
    } else {
      r.cfear[0] = r.cfear[1] = r.cfear[2] = 0.0;                   // :349-351
    }
    double z = par->align_intercept;                                // predict_linear (alignmentinterface.cpp:271-279)
    for (int k = 0; k < 3; k++) z += par->align_coef[k] * r.coral[k];
    for (int k = 0; k < 3; k++) z += par->align_coef[3 + k] * r.cfear[k];
    r.alignment_quality = z;
    r.odom_bounds = jobs[j].odom_bounds;
    r.sc_sim = jobs[j].sc_sim;
    if (par->verification_disabled) {
      r.probability = 0.0;                                          // loopclosure.cpp:377
    } else {
      const double zl = par->loop_coef[0] * r.odom_bounds + par->loop_coef[1] * r.sc_sim +
                        par->loop_coef[2] * r.alignment_quality + par->loop_intercept;
      r.probability = 1.0 / (1.0 + std::exp(-zl));
    }
    r.accepted = 0;
    r.rank = 0;
  }

  apply_constraints(jobs, n, par, results);
  mark(6);
#ifdef CFEAR_VERIFY_TIMING
  fprintf(stderr, "verify us: marshal reg %.0f | register_batch %.0f | Talign + coral jobs %.0f | coral enqueue %.0f | cov + cost jobs %.0f | get_cost_batch + coral results %.0f | classify + sort %.0f\n",
          t_acc[0], t_acc[1], t_acc[2], t_acc[3], t_acc[4], t_acc[5], t_acc[6]);
#endif
  return CFEAR_OK;
}

extern "C" int cfear_verify_loop_candidates(cfear_ctx* ctx, const cfear_verify_job* jobs, int32_t n_jobs,
                                            const cfear_verify_params* par, cfear_verify_result* results) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !par || !results || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_jobs == 0) return CFEAR_OK;
  for (int j = 0; j < n_jobs; j++)
    if (!jobs[j].from_scan || !jobs[j].to_scan)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d: null scan handle", j);
  if (par->use_covariance_sampling) {
    if (cfear_is_device_ptr(results)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "results on the device are not available with use_covariance_sampling");
    return verify_host_chain(ctx, jobs, n_jobs, par, results);
  }
  return verify_device_chain(ctx, jobs, n_jobs, par, results);
}

extern "C" int cfear_verify_apply_constraints(const int32_t* groups, int32_t n, const cfear_verify_params* par, cfear_verify_result* results) {
  if (!par || n < 0 || (n > 0 && (!groups || !results))) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n > 0) apply_constraints_groups(groups, sizeof(int32_t), (size_t)n, par, results);
  return CFEAR_OK;
}

extern "C" void cfear_loop_verify_params_default(cfear_loop_verify_params* p) {
  if (!p) return;
  cfear_verify_params_default(&p->verify);
  p->odom_sigma_error = 0.03;                  // loopclosure.h:123
  p->verify_via_odometry = 1;                  // :122
  p->transl_guess = 1;                         // :126
  p->speedup = 0;                              // :127
  p->odometry_coupled_closure = 1;             // RSCManager's default, cfear_sc_manager_params_default
}

extern "C" int cfear_verify_graph_candidates(cfear_ctx* ctx, const cfear_loop_graphs* graphs, const cfear_loop_verify_candidate* cands,
                                             int32_t n_cand, const cfear_loop_verify_params* par, cfear_verify_result* results,
                                             cfear_loop_verify_candidate* list_out, cfear_loop_candidate* loops_out) {
  return verify_graph_route(ctx, graphs, cands, n_cand, GraphRows(), par, results, list_out, loops_out, nullptr);
}

extern "C" int cfear_verify_sc_rows(cfear_ctx* ctx, const cfear_loop_graphs* graphs, const cfear_sc_candidate* rows, const int32_t* n_out,
                                    const int32_t* n_detect, int32_t n_candidates, const cfear_loop_verify_params* par,
                                    cfear_verify_result* results, cfear_loop_verify_candidate* list_out, cfear_loop_candidate* loops_out,
                                    int32_t* n_list) {
  if (!n_list) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null n_list");
  GraphRows rw;
  rw.rows = rows; rw.n_out = n_out; rw.n_detect = n_detect; rw.nc = n_candidates;
  return verify_graph_route(ctx, graphs, nullptr, 0, rw, par, results, list_out, loops_out, n_list);
}

// ---- sampled covariances for candidates that were verified on the device ------------------------------------------------------
// What verify_host_chain does under use_covariance_sampling (loopclosure.cpp:62-71, 99-208), as a pass of its own over the
// records cfear_verify_graph_candidates / cfear_verify_sc_rows wrote, without the host seeing a candidate:
//   verify_sample_scan_kernel   every candidate's rank among those with skip == 0 and reg_ok == 1
//   verify_sample_fill_kernel   list + results -> cfear_candidate {to fixed at Tfrom * guess, from free} and the dense
//                               registration records (gathered from the 480-byte stride), validation, the header
//   ONE read-back of the 16-byte header; then CovSamplePass (register.hip): centre -> expand -> matcher (cost only) -> cov_fit_kernel
//   verify_sample_write_kernel  R^-1 C R^-T by the registered yaw into `cov`, cov_sampled = 1 -- where the fit was accepted;
//                               a refused fit leaves the record as it is: Register's constant, rotated, cov_sampled = 0
namespace {

struct SampleArgs {
  const ScanView* views;
  const double* poses;                  // [n_nodes][3]
  const int32_t* node_off;              // [n_graphs + 1]
  const cfear_loop_verify_candidate* list;
  cfear_verify_result* results;
  int32_t* active_rank;                 // [n]
  int32_t* out_index;                   // [n] sampled candidate a -> its place j in the list
  cfear_candidate* cands;               // [n] dense over the sampled candidates
  cfear_reg_result* regs;               // [n]
  int32_t* head;                        // {first unusable candidate, largest `to` cell count, largest `from` cell count, sampled candidates}
  const double* cov36;                  // [n][36] the fits
  const int32_t* success;               // [n]
  int32_t n_graphs, n;
};

__host__ __device__ inline bool sample_takes_part(const cfear_loop_verify_candidate& c, const cfear_verify_result& r) {
  return c.skip == 0 && r.reg_ok == 1;
}
__host__ __device__ inline bool sample_pose_usable(const cfear_verify_result& r) {
  return fin1(r.reg.pose[0]) && fin1(r.reg.pose[1]) && fin1(r.reg.pose[2]);
}

__global__ __launch_bounds__(256) void verify_sample_scan_kernel(const SampleArgs a) {
  const int total = block_excl_scan_256(
      a.n,
      [&](int j) {
        const cfear_loop_verify_candidate c = a.list[j];
        return !graph_cand_fault(c, a.node_off, a.n_graphs) && sample_takes_part(c, a.results[j]) ? 1 : 0;
      },
      [&](int j, int rank) { a.active_rank[j] = rank; });
  if (threadIdx.x == 0) a.head[3] = total;
}

__global__ __launch_bounds__(256) void verify_sample_fill_kernel(const SampleArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const cfear_loop_verify_candidate c = a.list[j];
  if (graph_cand_fault(c, a.node_off, a.n_graphs)) { atomicMin(&a.head[0], j); return; }
  const cfear_verify_result& r = a.results[j];
  if (!sample_takes_part(c, r)) return;
  if (!sample_pose_usable(r)) atomicMin(&a.head[0], j);   // (keeps its rank: the record below is never used after a refusal)
  const int node0 = a.node_off[c.graph];
  const int kf = node0 + c.from, kt = node0 + c.to;
  const int at = a.active_rank[j];
  a.out_index[at] = j;
  const cfear_reg_result reg = r.reg;
  cfear_candidate cd;
  cd.target = kt; cd.source = kf;
  double from_pose[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { from_pose[k] = a.poses[3 * (size_t)kf + k]; cd.source_xyt[k] = reg.pose[k]; }
  xyt_compose(from_pose, c.guess_xyt, cd.target_xyt);      // Tto = Tfrom * t_be, as verify_expand_kernel
  a.cands[at] = cd;
  a.regs[at] = reg;
  atomicMax(&a.head[1], *a.views[kt].n_cells);
  atomicMax(&a.head[2], *a.views[kf].n_cells);
}

__global__ __launch_bounds__(256) void verify_sample_write_kernel(const SampleArgs a, int n_active) {
  const int at = blockIdx.x * 256 + threadIdx.x;
  if (at >= n_active || !a.success[at]) return;
  cfear_verify_result& r = a.results[a.out_index[at]];
  const double* F = a.cov36 + (size_t)at * 36;
  double inv[3];
  xyt_inverse(a.regs[at].pose, inv);                       // Trevised^-1
  // reg_cov.block<3,3>(0,0) = R^-1 * block * R^-T: only the x-y part of the block is touched by a yaw rotation
  double sn, cs;
  sincos(inv[2], &sn, &cs);
  const double R[9] = {cs, -sn, 0, sn, cs, 0, 0, 0, 1};
  double B[9], T[9], O[9];
  for (int x = 0; x < 3; x++) for (int y = 0; y < 3; y++) B[x * 3 + y] = F[x * 6 + y];
  for (int x = 0; x < 3; x++) for (int y = 0; y < 3; y++) {
    double t = 0.0;
    for (int k = 0; k < 3; k++) t += R[x * 3 + k] * B[k * 3 + y];
    T[x * 3 + y] = t;
  }
  for (int x = 0; x < 3; x++) for (int y = 0; y < 3; y++) {
    double t = 0.0;
    for (int k = 0; k < 3; k++) t += T[x * 3 + k] * R[y * 3 + k];
    O[x * 3 + y] = t;
  }
  for (int x = 0; x < 6; x++) for (int y = 0; y < 6; y++) r.cov[x * 6 + y] = x < 3 && y < 3 ? O[x * 3 + y] : F[x * 6 + y];
  r.cov_sampled = 1;
}

// Everything that can be refused without a device, a null context last.
int sample_route_check(cfear_ctx* ctx, const cfear_loop_graphs* g, const cfear_loop_verify_candidate* list, int32_t n_list,
                       const cfear_loop_verify_params* par, const cfear_verify_result* results) {
  const auto refuse = [&](const char* what) { return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%s", what); };
  if (!g || !par || n_list < 0) return refuse("null or negative argument");
  if (g->n_graphs < 0 || !g->node_off) return refuse("null or negative argument (node_off holds n_graphs + 1 entries)");
  if (cfear_is_device_ptr(g->node_off) || cfear_is_device_ptr(g->poses_xyt)) return refuse("node_off and poses_xyt must be host memory");
  CFEAR_CHECK(cfear_cov_check_sampling(ctx, &par->verify.sampling));
  const int G = g->n_graphs;
  if (g->node_off[0] != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph 0: node_off must start at 0");
  for (int gi = 0; gi < G; gi++)
    if (g->node_off[gi + 1] < g->node_off[gi]) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: node_off descends", gi);
  const int N = g->node_off[G];
  if (N > 0 && !g->poses_xyt) return refuse("null poses_xyt with nodes");
  for (int gi = 0; gi < G; gi++)
    for (int k = g->node_off[gi]; k < g->node_off[gi + 1]; k++) {
      const double* p = g->poses_xyt + 3 * (size_t)k;
      if (!fin1(p[0]) || !fin1(p[1]) || !fin1(p[2]))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: a pose that is not finite", gi, k - g->node_off[gi]);
    }
  if (n_list > 0 && (!list || !results)) return refuse("null list or results with a positive count");
  if (memory_kind({list, results}) < 0) return refuse("list and results must be both host or both device memory");
  if (n_list > 0 && !cfear_is_device_ptr(list))
    for (int j = 0; j < n_list; j++) {
      const int f = graph_cand_fault(list[j], g->node_off, G);
      if (f) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d: %s", j, kGraphCandFault[f]);
      if (sample_takes_part(list[j], results[j]) && !sample_pose_usable(results[j]))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d: its registered pose is not finite", j);
    }
  if (N > 0 && !g->table) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null scan table: it must hold one entry per node (%d)", N);
  if (g->table && (int)g->table->n_cells.size() != N)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "the scan table holds %d scans, the graphs %d nodes", (int)g->table->n_cells.size(), N);
  if (!ctx) return refuse("null context");
  if (g->table && g->table->ctx != ctx) return refuse("the scan table belongs to another context");
  return CFEAR_OK;
}

}  // namespace

extern "C" int cfear_verify_sample_covariances(cfear_ctx* ctx, const cfear_loop_graphs* g, const cfear_loop_verify_candidate* list,
                                               int32_t n_list, const cfear_loop_verify_params* par, cfear_verify_result* results) {
  CFEAR_CHECK(sample_route_check(ctx, g, list, n_list, par, results));
  if (g->n_graphs == 0 || n_list == 0) return CFEAR_OK;
  const size_t n = (size_t)n_list, N = (size_t)g->node_off[g->n_graphs], G = (size_t)g->n_graphs;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsVerify);
  SampleArgs a{};
  a.views = g->table ? g->table->d_views.get() : nullptr;  // (no table: no nodes, and every candidate is refused before it is looked up)
  a.n_graphs = g->n_graphs; a.n = n_list;
  st.in(a.poses, g->poses_xyt, N * 24);
  st.in(a.node_off, g->node_off, (G + 1) * 4);
  st.in(a.list, list, n * sizeof(cfear_loop_verify_candidate));
  const bool host_out = st.in(a.results, results, n * sizeof(cfear_verify_result));
  st.piece(a.active_rank, n * 4);
  st.piece(a.out_index, n * 4);
  st.piece(a.cands, n * sizeof(cfear_candidate));
  st.piece(a.regs, n * sizeof(cfear_reg_result));
  double* d_cov;
  int32_t* d_ok;
  st.piece(d_cov, n * 36 * sizeof(double));
  st.piece(d_ok, n * 4);
  CovSamplePass pass;
  pass.plan(st, n_list, par->verify.sampling.samples_per_axis, 32);
  CFEAR_CHECK(st.carve());
  a.cov36 = d_cov; a.success = d_ok;
  CFEAR_CHECK(pass.stage(st, &par->verify.sampling));
  int32_t* h_head = (int32_t*)pass.h_extra();
  for (int k = 0; k < 8; k++) h_head[k] = 0;
  h_head[0] = h_head[4] = kNone;                           // [0..4): this route's header; [4..8): CovSamplePass::centre's
  CFEAR_CHECK(pass.upload(st));
  a.head = (int32_t*)pass.d_extra();
  const dim3 block(256);
  {
    ProfScope ps(ctx, "cov_glue");
    hipLaunchKernelGGL(verify_sample_scan_kernel, dim3(1), block, 0, ctx->stream, a);
    hipLaunchKernelGGL(verify_sample_fill_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  int32_t head[4];
  st.fetch(head, a.head, sizeof(head));
  CFEAR_CHECK(st.wait());
  // ---- the device's refusal: nothing has been written to the caller's records yet -----------------------------------------------
  if (head[0] != kNone)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d: its graph, from, to, guess_nr, guess, sc_sim or registered pose are not usable", head[0]);
  const int n_active = head[3];
  if (n_active == 0) return st.finish();
  // RegisterLoopCandidate's problem and parameters (loopclosure.cpp:56-57), as verify_host_chain hands them to the sampling
  cfear_reg_params rp;
  cfear_reg_params_default(&rp);
  rp.cost = CFEAR_P2L; rp.max_itr_association = 4; rp.max_itr_solver = 10;
  CFEAR_CHECK(pass.centre(ctx, g->table, a.cands, a.regs, n_active, &rp, a.head + 4));
  CFEAR_CHECK(pass.sample_and_fit(ctx, g->table, a.cands, n_active, head[1], head[2], &rp, a.regs, &par->verify.sampling, d_cov, d_ok));
  {
    ProfScope ps(ctx, "cov_glue");
    hipLaunchKernelGGL(verify_sample_write_kernel, dim3((unsigned)((n_active + 255) / 256)), block, 0, ctx->stream, a, n_active);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  if (host_out) st.back(results, a.results, n * sizeof(cfear_verify_result));
  return st.finish();
}
