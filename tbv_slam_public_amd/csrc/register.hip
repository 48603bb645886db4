// register.hip -- the host side of the matcher (matcher.hip): what turns the C ABI's handles into job records and
// launches.  Job staging, cfear_register_batch / cfear_register, the scan table and the candidate batches of loop closure
// (with the kernel that expands them into job records), GetCost for batches and covariance by cost sampling.  The launch
// itself (cfear_register_launch) and the cfear_cost object stay with the kernels.
#include <algorithm>
#include <cmath>
#include <memory>

#include "covfit.hpp"
#include "registration.hpp"

int cfear_check_reg_params(cfear_ctx* ctx, const cfear_reg_params* p) {
  if (!p) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null parameters");
  if (p->cost < 0 || p->cost > 2 || p->loss < 0 || p->loss > 5 || p->weight_opt < 0 || p->weight_opt > 4)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad cost/loss/weight option");
  if (p->max_itr_association < 1 || p->max_itr_solver < 0 || !(p->radius > 0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad iteration limits / radius");
  return CFEAR_OK;
}

// ---- the checks of scan handles and jobs ---------------------------------------------------------
namespace {
// "job <job>: " in front of a refusal, or nothing (job < 0)
struct JobPrefix {
  char text[24];
  explicit JobPrefix(int job) { text[0] = 0; if (job >= 0) snprintf(text, sizeof(text), "job %d: ", job); }
};
}  // namespace

int cfear_reg_check_scan(cfear_ctx* ctx, const cfear_scan* scan, int job) {
  if (!scan) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%snull scan handle", JobPrefix(job).text);
  if (scan->ctx != ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%sscan belongs to another context", JobPrefix(job).text);
  return cfear_scan_size(scan);
}

int cfear_reg_check_job(cfear_ctx* ctx, const cfear_scan* const* scans, int n_scans, const double* poses_xyt, int job, bool check_poses,
                        RegJobCells* cells) {
  if (n_scans < 2 || n_scans > kRegMaxScans)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%sn_scans must be in [2,%d]", JobPrefix(job).text, kRegMaxScans);
  if (check_poses && (!scans || !poses_xyt)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%snull scans or poses", JobPrefix(job).text);
  cells->sum_pad = cells->max_pad = 0;
  for (int i = 0; i < n_scans; i++) {
    const int nc = cfear_reg_check_scan(ctx, scans[i], job);
    if (nc < 0) return nc;
    for (int k = 0; check_poses && k < 3; k++)
      if (!std::isfinite(poses_xyt[3 * i + k]))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%spose %d is not finite", JobPrefix(job).text, i);
    cells->n[i] = nc;
    if (i < n_scans - 1) { cells->sum_pad += scan_grid_pad(nc); cells->max_pad = std::max(cells->max_pad, scan_grid_pad(nc)); }
  }
  return CFEAR_OK;
}

int cfear_reg_gather_job(cfear_ctx* ctx, const cfear_scan* const* scans, int n_scans, const double* poses_xyt, unsigned char* dst,
                         JobSizes& sz, RegJobCells* cells) {
  CFEAR_CHECK(cfear_reg_check_job(ctx, scans, n_scans, poses_xyt, -1, false, cells));
  ScanView views[kRegMaxScans];
  for (int i = 0; i < n_scans; i++) views[i] = scans[i]->view;
  sz.add(n_scans, cells->sum_pad, cells->max_pad, cells->n[n_scans - 1]);
  cfear_reg_fill_job(dst, views, n_scans, poses_xyt);
  return CFEAR_OK;
}

namespace {

// A batch of jobs as device records, built in the stage's pinned record with the stride of the batch's longest job, and
// where its n_results results go: used in place when they are device memory, copied back by finish() when the host's.
struct JobBatch {
  explicit JobBatch(const cfear_reg_params* par) : sz(par) {}
  JobSizes sz;
  size_t stride = 0;
  char* d_jobs = nullptr;
  cfear_reg_result* d_res = nullptr;
};
int stage_jobs(cfear_ctx* ctx, HostStage& st, const cfear_reg_job* jobs, int n_jobs, const int32_t* itrs /*nullable: per-job itr_*/,
               cfear_reg_result* results, size_t n_results, JobBatch& b) {
  int max_scans = 2;
  for (int j = 0; j < n_jobs; j++) max_scans = std::max(max_scans, std::min(jobs[j].n_scans, kRegMaxScans));
  b.stride = reg_job_stride(max_scans);
  const size_t jb = (size_t)n_jobs * b.stride;
  unsigned char* hjobs = (unsigned char*)st.pinned(jb);
  if (!hjobs) return CFEAR_ERR_HIP;
  RegJobCells cells;
  for (int j = 0; j < n_jobs; j++) {
    unsigned char* dst = hjobs + (size_t)j * b.stride;
    CFEAR_CHECK(cfear_reg_gather_job(ctx, jobs[j].scans, jobs[j].n_scans, jobs[j].poses_xyt, dst, b.sz, &cells));
    if (itrs) ((RegJob*)dst)->itr = itrs[j];
  }
  st.piece(b.d_jobs, jb);
  st.out(b.d_res, results, n_results * sizeof(cfear_reg_result));
  CFEAR_CHECK(st.carve());
  return st.upload(b.d_jobs, hjobs, jb);
}

}  // namespace

// results on the device stay there, stream-ordered and not synchronised (the sharded entry hands them to the collective)
extern "C" int cfear_register_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs,
                                    const cfear_reg_params* par, cfear_reg_result* results) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !results || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(cfear_check_reg_params(ctx, par));
  if (n_jobs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsRegJobs);
  JobBatch b(par);
  CFEAR_CHECK(stage_jobs(ctx, st, jobs, n_jobs, nullptr, results, (size_t)n_jobs, b));
  char* scr = (char*)cfear_workspace(ctx, kWsRegScratch, reg_scratch_bytes(b.sz.pairs_cap) * (size_t)n_jobs);
  if (!scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  CFEAR_CHECK(cfear_register_launch(ctx, b.d_jobs, n_jobs, par, b.sz.pairs_cap, scr, b.d_res, nullptr, b.stride, b.sz.hint(n_jobs)));
  return st.finish();
}

// ---- candidate pairs among a table of scans (loop closure) ---------------------------------------------------------
// The table holds a reference on every scan (cfear_scan::refs): a scan destroyed while a table still names it keeps its slab
// until the table goes too, so a candidate can never read another scan's cells through a recycled slab.
// (struct cfear_scan_table: registration.hpp)
namespace {
// candidate -> the job record matcher_kernel reads: scans {target, source}, poses {target, source guess}
__global__ __launch_bounds__(256) void expand_candidates_kernel(const ScanView* __restrict__ views, const cfear_candidate* __restrict__ cands,
                                                                int n, char* __restrict__ jobs, size_t stride, int32_t* __restrict__ trailer,
                                                                int trailer_status) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0 && trailer) { trailer[0] = trailer_status; trailer[1] = n; }   // the sharded step's {rank status, records} (shard.hip)
  if (i >= n) return;
  const cfear_candidate c = cands[i];
  RegJob* j = (RegJob*)(jobs + (size_t)i * stride);
  j->n_scans = 2; j->itr = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) { j->poses[0][k] = c.target_xyt[k]; j->poses[1][k] = c.source_xyt[k]; }
  j->scans[0] = views[c.target];
  j->scans[1] = views[c.source];
}
}  // namespace

extern "C" int cfear_scan_table_create(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans, cfear_scan_table** out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!scans || !out || n_scans < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument / empty table");
  *out = nullptr;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsRegJobs);
  const size_t vb = (size_t)n_scans * sizeof(ScanView);
  ScanView* views = (ScanView*)st.record(vb);
  std::unique_ptr<cfear_scan_table> t(new cfear_scan_table());
  t->ctx = ctx;
  t->n_cells.resize((size_t)n_scans);
  for (int i = 0; i < n_scans; i++) {
    const int nc = cfear_reg_check_scan(ctx, scans[i], -1);
    if (nc < 0) return nc;
    views[i] = scans[i]->view;
    t->n_cells[(size_t)i] = nc;
  }
  if (!(t->d_views = dev_alloc<ScanView>(vb))) return cfear_set_error(ctx, CFEAR_ERR_HIP, "scan table: hipMalloc failed");
  if (st.upload(t->d_views.get(), views, vb) != CFEAR_OK || st.finish() != CFEAR_OK)
    return cfear_set_error(ctx, CFEAR_ERR_HIP, "scan table upload failed");
  t->scans.resize((size_t)n_scans);
  for (int i = 0; i < n_scans; i++) { t->scans[(size_t)i] = const_cast<cfear_scan*>(scans[i]); cfear_scan_retain(t->scans[(size_t)i]); }
  *out = t.release();
  return CFEAR_OK;
}

extern "C" int cfear_scan_table_size(const cfear_scan_table* t) { return t ? (int)t->n_cells.size() : CFEAR_ERR_INVALID_ARGUMENT; }

extern "C" int cfear_scan_table_destroy(cfear_scan_table* t) {
  if (!t) return CFEAR_OK;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  for (cfear_scan* s : t->scans) (void)cfear_scan_release(s);          // drops the table's reference
  delete t;
  return CFEAR_OK;
}

// A candidate batch in two halves (cfear_candidate_pipe runs them on different streams; cfear_candidates_enqueue is both in a row).
// expand: validates the candidates while it copies them into `h_stage` (PINNED host memory, n records, owned by the caller until
// the kernel has run) and turns them into job records at d_jobs (n * reg_job_stride(2) bytes) on `stream` -- no upload: pinned
// memory is mapped into the device's address space, the kernel reads the 56-byte records over PCIe itself.  d_trailer
// (optional, device int32[2]) receives {trailer_status, n}: the status trailer of a sharded step travels behind the block
// without an enqueue of its own.  geom receives what the matcher's launch needs to know about the batch.
int cfear_candidates_expand(cfear_ctx* ctx, hipStream_t stream, const cfear_scan_table* table, const cfear_candidate* cands, int32_t n,
                            const cfear_reg_params* par, cfear_candidate* h_stage, char* d_jobs, int32_t* d_trailer, int trailer_status,
                            CandGeometry* geom) {
  if (table->ctx != ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "table belongs to another context");
  const int nt = (int)table->n_cells.size();
  JobSizes sz(par);
  int max_tar = 0, max_src = 0;
  for (int i = 0; i < n; i++) {
    const cfear_candidate& c = cands[i];
    if (c.target < 0 || c.target >= nt || c.source < 0 || c.source >= nt)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d refers to scan %d / %d of a table of %d", i, c.target, c.source, nt);
    max_tar = std::max(max_tar, table->n_cells[(size_t)c.target]);
    max_src = std::max(max_src, table->n_cells[(size_t)c.source]);
    h_stage[i] = c;
  }
  // the launch geometry from the LARGEST target and source of the batch (a pair's needs grow with both: if that pair fits a
  // form, every candidate does) -- one evaluation per batch, not per candidate (4096 candidates: 0.1 ms of host time)
  sz.add(2, scan_grid_pad(max_tar), scan_grid_pad(max_tar), max_src);
  geom->pairs_cap = sz.pairs_cap; geom->hint = sz.hint(n);
  hipLaunchKernelGGL(expand_candidates_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const ScanView*)table->d_views.get(),
                     (const cfear_candidate*)h_stage, n, d_jobs, reg_job_stride(2), d_trailer, trailer_status);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

// match: the matcher over the job records expand left at d_jobs, on the context's stream; records to d_res (device)
int cfear_candidates_match(cfear_ctx* ctx, const char* d_jobs, int32_t n, const cfear_reg_params* par, const CandGeometry* geom,
                           cfear_reg_result* d_res) {
  char* scr = (char*)cfear_workspace(ctx, kWsRegScratch, reg_scratch_bytes(geom->pairs_cap) * (size_t)n);
  if (!scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  return cfear_register_launch(ctx, d_jobs, n, par, geom->pairs_cap, scr, d_res, nullptr, reg_job_stride(2), geom->hint);
}

int cfear_candidates_enqueue(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* cands, int32_t n,
                             const cfear_reg_params* par, cfear_candidate* h_stage, cfear_reg_result* d_res, int32_t* d_trailer,
                             int trailer_status) {
  char* ws = (char*)cfear_workspace(ctx, kWsRegJobs, (size_t)n * reg_job_stride(2) + 512);
  if (!ws) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  CandGeometry geom;
  const int rc = cfear_candidates_expand(ctx, ctx->stream, table, cands, n, par, h_stage, ws, d_trailer, trailer_status, &geom);
  if (rc != CFEAR_OK) return rc;
  return cfear_candidates_match(ctx, ws, n, par, &geom, d_res);
}

extern "C" int cfear_register_candidates(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* cands, int32_t n,
                                         const cfear_reg_params* par, cfear_reg_result* results) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!table || !results || n < 0 || (n > 0 && !cands)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  int rc = cfear_check_reg_params(ctx, par);
  if (rc != CFEAR_OK || n == 0) return rc;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // the candidates are copied into the pinned record and read from there by the expanding kernel (cfear_candidates_expand)
  HostStage st(ctx, kWsCandResults);
  cfear_candidate* hc = (cfear_candidate*)st.pinned((size_t)n * sizeof(cfear_candidate));
  if (!hc) return CFEAR_ERR_HIP;
  cfear_reg_result* d_res;
  st.out(d_res, results, (size_t)n * sizeof(cfear_reg_result));
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(cfear_candidates_enqueue(ctx, table, cands, n, par, hc, d_res, nullptr, 0));
  return st.finish();
}


extern "C" int cfear_register(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans, double* poses_xyt,
                              const cfear_reg_params* par, cfear_reg_result* result) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!scans || !poses_xyt || !result) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  cfear_reg_job job;
  job.scans = scans; job.n_scans = n_scans; job.pad = 0; job.poses_xyt = poses_xyt;
  int rc = cfear_register_batch(ctx, &job, 1, par, result);
  if (rc != CFEAR_OK) return rc;
  // Tsrc.back() = vectorToAffine3d(parameters.back()) whenever a solve was usable (n_scan_normal.cpp:117-119)
  poses_xyt[3 * (n_scans - 1)] = result->pose[0];
  poses_xyt[3 * (n_scans - 1) + 1] = result->pose[1];
  poses_xyt[3 * (n_scans - 1) + 2] = result->pose[2];
  return result->status;
}

// ---- GetCost for batches and covariance by cost sampling ---------------------------------------------
namespace {

// Runs the cost-only mode over `jobs`; results (host or device) receives max(mode.n_samples, 1) records per job.
// itrs (nullable) = per-job leftover itr_; otherwise par->itr applies to every job.
int run_cost_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int n_jobs, const cfear_reg_params* par,
                   const int32_t* itrs, RegCostMode mode, cfear_reg_result* results) {
  CFEAR_CHECK(cfear_check_reg_params(ctx, par));
  if (n_jobs == 0) return CFEAR_OK;
  const int m = mode.n_samples > 0 ? mode.n_samples : 1;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsRegJobs);
  JobBatch b(par);
  CFEAR_CHECK(stage_jobs(ctx, st, jobs, n_jobs, itrs, results, (size_t)n_jobs * m, b));
  // a few workgroups per job when the batch alone cannot fill the GPU; scratch bounded to 1 GiB per launch
  mode.blocks_per_job = std::max(1, std::min(m, (1024 + n_jobs - 1) / n_jobs));
  const size_t per = reg_scratch_bytes(b.sz.pairs_cap) * (size_t)mode.blocks_per_job;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_jobs, ((size_t)1 << 30) / per));
  char* scr = (char*)cfear_workspace(ctx, kWsRegScratch, per * (size_t)chunk);
  if (!scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  for (int j0 = 0; j0 < n_jobs; j0 += chunk) {
    const int nj = std::min(chunk, n_jobs - j0);
    CFEAR_CHECK(cfear_register_launch(ctx, b.d_jobs + (size_t)j0 * b.stride, nj, par, b.sz.pairs_cap, scr, b.d_res + (size_t)j0 * m, &mode,
                                      b.stride, b.sz.hint(nj)));
  }
  return st.finish();
}

}  // namespace

extern "C" int cfear_get_cost_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs,
                                    const cfear_reg_params* par, cfear_reg_result* results) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !results || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  return run_cost_batch(ctx, jobs, n_jobs, par, nullptr, RegCostMode{}, results);
}

extern "C" void cfear_cov_sampling_params_default(cfear_cov_sampling_params* p) {
  if (!p) return;
  p->xy_range = 0.4;                  // odometrykeyframefuser.h:107 (loopclosure.cpp:108: +-0.2)
  p->yaw_range = 0.0043625;           // :108 (loopclosure.cpp:109 uses +-0.0022)
  p->samples_per_axis = 3;            // :109
  p->pad = 0;
  p->covariance_scaler = 4.0;         // :110
}

extern "C" int cfear_covariance_by_sampling_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs,
                                                  const cfear_reg_params* par, const cfear_reg_result* regs,
                                                  const cfear_cov_sampling_params* sp, double* cov36, double* samples,
                                                  int32_t* success) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !regs || !sp || !cov36 || !success || n_jobs < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  const int n = sp->samples_per_axis;
  if (n < 1 || n > 15) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "samples_per_axis must be in [1,15]");
  RegCostMode mode;
  mode.samples_per_axis = n;
  mode.n_samples = n * n * n;
  mode.xy_half = sp->xy_range * 0.5;                       // odometrykeyframefuser.cpp:276-277
  mode.yaw_half = sp->yaw_range * 0.5;
  std::vector<int32_t> itrs(n_jobs);
  for (int j = 0; j < n_jobs; j++) itrs[j] = regs[j].outer_iters;      // GetCost's radius follows the leftover itr_
  const int m = mode.n_samples;
  std::vector<cfear_reg_result> out((size_t)n_jobs * m);
  CFEAR_CHECK(run_cost_batch(ctx, jobs, n_jobs, par, itrs.data(), mode, out.data()));
  CovFit fit;
  fit.prepare(n, mode.xy_half, mode.yaw_half);
  std::vector<double> costs(m);
  for (int j = 0; j < n_jobs; j++) {
    double sample_cost = 0.0;                              // :282; a failed GetCost leaves the previous value (:307)
    for (int s = 0; s < m; s++) {
      const cfear_reg_result& r = out[(size_t)j * m + s];
      if (r.status == CFEAR_OK) sample_cost = r.final_cost;
      costs[s] = sample_cost;
      if (samples) {
        double* o = samples + ((size_t)j * m + s) * 4;
        o[0] = fit.offsets[3 * (size_t)s]; o[1] = fit.offsets[3 * (size_t)s + 1]; o[2] = fit.offsets[3 * (size_t)s + 2];
        o[3] = sample_cost;
      }
    }
    // GetCovarianceScaler (n_scan_normal.cpp:433-439): final_cost / (num_residuals_reduced - num_parameters_reduced)
    bool ok = regs[j].num_residuals - 3 != 0;
    if (ok) {
      const double score_scale = regs[j].final_cost / (double)(regs[j].num_residuals - 3);
      ok = fit.solve(costs.data(), score_scale, sp->covariance_scaler, cov36 + (size_t)j * 36);
    }
    success[j] = ok ? 1 : 0;
    if (!ok) {                                             // caller keeps Register's reg_cov (n_scan_normal.cpp:171-175)
      double* c = cov36 + (size_t)j * 36;
      for (int k = 0; k < 36; k++) c[k] = 0.0;
      c[0] = 0.01; c[7] = 0.01; c[35] = 1e-4;
    }
  }
  return CFEAR_OK;
}

// ---- the same for candidate pairs of a scan table, without the host between the samples and the covariance ------------------
// centre -> expand -> matcher (cost only, RegCostMode::prior = the centres) -> cov_fit_kernel (covfit.hip).  The candidates and
// the registration records may already sit on the device; nothing is read back on the way.
namespace {
constexpr int kCovNone = 0x7fffffff;
// One lane per candidate: where its samples are centred and which radius they use, as a record the matcher's cost-only mode
// takes for `prior`.  A registration that failed is sampled around the candidate's own source pose (what verify_host_chain's
// `posed` does); outer_iters = 0 selects par.itr, as a job record's itr does.
__global__ __launch_bounds__(256) void cov_centre_kernel(const ScanView* __restrict__ views, int n_table,
                                                         const cfear_candidate* __restrict__ cands,
                                                         const cfear_reg_result* __restrict__ regs, int n, int par_itr,
                                                         cfear_reg_result* __restrict__ centre, int32_t* __restrict__ head) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const cfear_candidate c = cands[j];
  if (c.target < 0 || c.target >= n_table || c.source < 0 || c.source >= n_table) { atomicMin(&head[0], j); return; }
  cfear_reg_result r = regs[j];
  if (r.status != CFEAR_OK) { r.pose[0] = c.source_xyt[0]; r.pose[1] = c.source_xyt[1]; r.pose[2] = c.source_xyt[2]; }
  if (r.outer_iters == 0) r.outer_iters = par_itr;
  centre[j] = r;
  atomicMax(&head[1], *views[c.target].n_cells);
  atomicMax(&head[2], *views[c.source].n_cells);
}
}  // namespace

void CovSamplePass::plan(HostStage& st, int n_jobs, int samples_per_axis, size_t extra_bytes) {
  n = n_jobs; spa = samples_per_axis; m = spa * spa * spa; extra = extra_bytes;
  st.piece(d_jobs, (size_t)n * reg_job_stride(2));
  st.piece(d_centre, (size_t)n * sizeof(cfear_reg_result));
  st.piece(d_samples, (size_t)n * m * sizeof(cfear_reg_result));
  st.piece(d_block, pinv_bytes() + extra);
}

int CovSamplePass::stage(HostStage& st, const cfear_cov_sampling_params* sp) {
  h_block = (char*)st.pinned(pinv_bytes() + extra);
  if (!h_block) return CFEAR_ERR_HIP;
  cfear_cov_fit_fill_pinv(sp, (double*)h_block);
  return CFEAR_OK;
}

int CovSamplePass::upload(HostStage& st) { return st.upload(d_block, h_block, pinv_bytes() + extra); }

int CovSamplePass::centre(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* d_cands, const cfear_reg_result* d_regs,
                          int n_jobs, const cfear_reg_params* par, int32_t* d_head) const {
  ProfScope ps(ctx, "cov_glue");
  hipLaunchKernelGGL(cov_centre_kernel, dim3((n_jobs + 255) / 256), dim3(256), 0, ctx->stream, (const ScanView*)table->d_views.get(),
                     (int)table->n_cells.size(), d_cands, d_regs, n_jobs, (int)par->itr, d_centre, d_head);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int CovSamplePass::sample_and_fit(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* d_cands, int n_jobs,
                                  int max_tar_cells, int max_src_cells, const cfear_reg_params* par, const cfear_reg_result* d_regs,
                                  const cfear_cov_sampling_params* sp, double* d_cov36, int32_t* d_success) const {
  const size_t stride = reg_job_stride(2);
  {
    ProfScope ps(ctx, "cov_glue");
    hipLaunchKernelGGL(expand_candidates_kernel, dim3((n_jobs + 255) / 256), dim3(256), 0, ctx->stream, (const ScanView*)table->d_views.get(),
                       d_cands, n_jobs, d_jobs, stride, (int32_t*)nullptr, 0);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  const JobSizes sz = JobSizes(par).add(2, scan_grid_pad(max_tar_cells), scan_grid_pad(max_tar_cells), max_src_cells);
  RegCostMode mode;
  mode.samples_per_axis = spa;
  mode.n_samples = m;
  mode.xy_half = sp->xy_range * 0.5;                       // odometrykeyframefuser.cpp:276-277
  mode.yaw_half = sp->yaw_range * 0.5;
  // as run_cost_batch: a few workgroups per job when the batch alone cannot fill the GPU; scratch bounded to 1 GiB per launch
  mode.blocks_per_job = std::max(1, std::min(m, (1024 + n_jobs - 1) / n_jobs));
  const size_t per = reg_scratch_bytes(sz.pairs_cap) * (size_t)mode.blocks_per_job;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_jobs, ((size_t)1 << 30) / per));
  char* scr = (char*)cfear_workspace(ctx, kWsRegScratch, per * (size_t)chunk);
  if (!scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  for (int j0 = 0; j0 < n_jobs; j0 += chunk) {
    const int nj = std::min(chunk, n_jobs - j0);
    mode.prior = d_centre + j0;
    CFEAR_CHECK(cfear_register_launch(ctx, d_jobs + (size_t)j0 * stride, nj, par, sz.pairs_cap, scr, d_samples + (size_t)j0 * m, &mode, stride,
                                      sz.hint(nj)));
  }
  return cfear_cov_fit_launch(ctx, d_regs, d_samples, n_jobs, m, (const double*)d_block, sp->covariance_scaler, d_cov36, d_success);
}

extern "C" int cfear_covariance_by_sampling_candidates(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* cands, int32_t n,
                                                       const cfear_reg_params* par, const cfear_reg_result* regs,
                                                       const cfear_cov_sampling_params* sp, double* cov36, int32_t* success) {
  if (!table || !regs || !sp || !cov36 || !success || n < 0 || (n > 0 && !cands)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(cfear_cov_check_sampling(ctx, sp));
  if (memory_kind({regs, cov36, success}) < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "regs, cov36 and success must be all host or all device memory");
  CFEAR_CHECK(cfear_check_reg_params(ctx, par));
  if (!ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null context");      // (a table cannot exist without one)
  if (table->ctx != ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "table belongs to another context");
  const bool host_cands = n > 0 && !cfear_is_device_ptr(cands);
  const int nt = (int)table->n_cells.size();
  int max_tar = 0, max_src = 0;
  for (int i = 0; host_cands && i < n; i++) {
    const cfear_candidate& c = cands[i];
    if (c.target < 0 || c.target >= nt || c.source < 0 || c.source >= nt)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d refers to scan %d / %d of a table of %d", i, c.target, c.source, nt);
    max_tar = std::max(max_tar, table->n_cells[(size_t)c.target]);
    max_src = std::max(max_src, table->n_cells[(size_t)c.source]);
  }
  if (n == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsRegJobs);
  CovSamplePass pass;
  const size_t cand_bytes = (size_t)n * sizeof(cfear_candidate);
  pass.plan(st, n, sp->samples_per_axis, 16 + (host_cands ? cand_bytes : 0));
  const cfear_reg_result* d_regs;
  double* d_cov;
  int32_t* d_ok;
  st.in(d_regs, regs, (size_t)n * sizeof(cfear_reg_result));
  st.out(d_cov, cov36, (size_t)n * 36 * sizeof(double));
  st.out(d_ok, success, (size_t)n * sizeof(int32_t));
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(pass.stage(st, sp));
  int32_t* h_head = (int32_t*)pass.h_extra();
  h_head[0] = kCovNone; h_head[1] = h_head[2] = h_head[3] = 0;
  if (host_cands) memcpy(pass.h_extra() + 16, cands, cand_bytes);
  CFEAR_CHECK(pass.upload(st));
  int32_t* d_head = (int32_t*)pass.d_extra();
  const cfear_candidate* d_cands = host_cands ? (const cfear_candidate*)(pass.d_extra() + 16) : cands;
  CFEAR_CHECK(pass.centre(ctx, table, d_cands, d_regs, n, par, d_head));
  if (!host_cands) {                                       // a device list is checked by the kernel that reads it
    int32_t head[4];
    st.fetch(head, d_head, sizeof(head));
    CFEAR_CHECK(st.wait());
    if (head[0] != kCovNone)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %d refers to a scan outside the table of %d", head[0], nt);
    max_tar = head[1]; max_src = head[2];
  }
  CFEAR_CHECK(pass.sample_and_fit(ctx, table, d_cands, n, max_tar, max_src, par, d_regs, sp, d_cov, d_ok));
  return st.finish();
}

extern "C" int cfear_covariance_by_sampling(cfear_ctx* ctx, const cfear_scan* const* scans, int32_t n_scans,
                                            const double* poses_xyt, const cfear_reg_params* par,
                                            const cfear_reg_result* reg, const cfear_cov_sampling_params* sp,
                                            double* cov36, double* samples, int32_t* success) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!scans || !poses_xyt) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  cfear_reg_job job;
  job.scans = scans; job.n_scans = n_scans; job.pad = 0; job.poses_xyt = poses_xyt;
  return cfear_covariance_by_sampling_batch(ctx, &job, 1, par, reg, sp, cov36, samples, success);
}
