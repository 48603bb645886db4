// registration.hpp -- the internal interface of the registration family: the matcher's job record and launch (matcher.hip),
// the host entry points around it (register.hip), and what their callers share (odometry.hip, verify.hip, shard.hip,
// tieaudit.hip).  The launch arithmetic is reg_layout.hpp's, the planar pose algebra pose2d.hpp's.
#pragma once
#include "common.hpp"
#include "pose2d.hpp"
#include "reg_layout.hpp"

// One registration of the matcher.  Kernels only ever touch scans[0 .. n_scans); a batch is stored with reg_job_stride.
struct RegJob {
  int32_t n_scans;
  int32_t itr;                                // cost-only launches: this job's leftover itr_ (0: use par.itr)
  double poses[kRegMaxScans][3];
  ScanView scans[kRegMaxScans];
};
static_assert(offsetof(RegJob, scans) == kRegJobHeadBytes && sizeof(ScanView) == kRegViewBytes, "reg_layout.hpp restates the record");

// Writes the used prefix of a job record: reg_job_stride(n_scans) bytes at dst.
void cfear_reg_fill_job(void* dst, const ScanView* views, int n_scans, const double* poses_xyt);
int cfear_check_reg_params(cfear_ctx* ctx, const cfear_reg_params* par);

// Cost-only launches of the matcher (GetCost / cost sampling): n_samples = 0 evaluates each job
// at its own source pose, n_samples = samples_per_axis^3 at the sampling grid around it; results then holds
// max(n_samples, 1) records per job.  blocks_per_job workgroups share a job's samples (scratch: n_jobs x
// blocks_per_job x reg_scratch_bytes).
struct RegCostMode {
  int n_samples = 0, samples_per_axis = 0, blocks_per_job = 1;
  double xy_half = 0.0, yaw_half = 0.0;
  const cfear_reg_result* prior = nullptr;   // device, [n_jobs]: evaluate around prior[j].pose with itr = prior[j].outer_iters
};
int cfear_register_launch(cfear_ctx* ctx, const void* d_jobs, int n_jobs, const cfear_reg_params* par, int pairs_cap,
                          char* d_scratch, cfear_reg_result* d_results, const RegCostMode* mode = nullptr,
                          size_t job_stride = 0,    // 0: full records (sizeof(RegJob))
                          RegLaunchHint hint = RegLaunchHint());

// The checks every entry point makes of the handles it is given.  job >= 0 words a refusal as "job <job>: ...", -1 without
// the prefix.  A scan handle of `ctx`: its cell count, or the refusal's status (< 0).
int cfear_reg_check_scan(cfear_ctx* ctx, const cfear_scan* scan, int job);
// A cfear_reg_job: n_scans, then scan by scan the handle and (check_poses: the tie audit) a pose that is there and finite --
// the first fault in that order is the one named.  cells receives the cell counts and the fixed scans' padded record counts.
struct RegJobCells { int32_t n[kRegMaxScans]; int sum_pad, max_pad; };
int cfear_reg_check_job(cfear_ctx* ctx, const cfear_scan* const* scans, int n_scans, const double* poses_xyt, int job, bool check_poses,
                        RegJobCells* cells);
// check + the job's record at dst + its sizes into sz
int cfear_reg_gather_job(cfear_ctx* ctx, const cfear_scan* const* scans, int n_scans, const double* poses_xyt, unsigned char* dst,
                         JobSizes& sz, RegJobCells* cells);

// candidate batches in two halves (register.hip; cfear_candidate_pipe in shard.hip runs them on different streams)
struct CandGeometry { int pairs_cap = 1; RegLaunchHint hint; };
// A table of scans (register.hip makes and frees it; verify.hip reads its views as the nodes of batched graphs)
struct cfear_scan_table {
  cfear_ctx* ctx = nullptr;
  DevBuf<ScanView> d_views;             // [n] device
  std::vector<int32_t> n_cells;         // host copy of the cell counts (launch geometry)
  std::vector<cfear_scan*> scans;       // referenced handles
};
int cfear_candidates_expand(cfear_ctx* ctx, hipStream_t stream, const cfear_scan_table* table, const cfear_candidate* cands, int32_t n,
                            const cfear_reg_params* par, cfear_candidate* h_stage, char* d_jobs, int32_t* d_trailer, int trailer_status,
                            CandGeometry* geom);
int cfear_candidates_match(cfear_ctx* ctx, const char* d_jobs, int32_t n, const cfear_reg_params* par, const CandGeometry* geom,
                           cfear_reg_result* d_res);
int cfear_candidates_enqueue(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* cands, int32_t n,
                             const cfear_reg_params* par, cfear_candidate* h_stage, cfear_reg_result* d_res, int32_t* d_trailer,
                             int trailer_status);

// ---- covariance by cost sampling without the host between the samples and the fit (covfit.hip, register.hip) --------------
// The fit: regs [n_jobs], samples [n_jobs][m], pinv [10][m] (CovFit::prepare's, cfear_cov_fit_fill_pinv) -> cov36 [n_jobs][36],
// success [n_jobs]; everything in device memory, enqueued on the context's stream.
size_t cfear_cov_fit_pinv_bytes(int samples_per_axis);
void cfear_cov_fit_fill_pinv(const cfear_cov_sampling_params* sp, double* dst);
int cfear_cov_fit_launch(cfear_ctx* ctx, const cfear_reg_result* d_regs, const cfear_reg_result* d_samples, int n_jobs, int m,
                         const double* d_pinv, double covariance_scaler, double* d_cov36, int32_t* d_success);
int cfear_cov_check_sampling(cfear_ctx* ctx, const cfear_cov_sampling_params* sp);      // samples_per_axis in [1, 15]
// The pass over candidate pairs of a scan table (cfear_covariance_by_sampling_candidates; verify.hip's
// cfear_verify_sample_covariances).  plan() before the stage's carve(): the job records, the sample centres, the samples and
// one block that goes up in one copy from the pinned staging -- the pseudo-inverse, then `extra` bytes of the caller's
// (h_extra() after stage(), d_extra() their place on the device).  centre() enqueues the kernel that reads the candidates:
// centre j = regs[j].pose where regs[j].status is CFEAR_OK, else the candidate's own source pose; the radius follows
// regs[j].outer_iters.  It checks the table indices (a bad candidate writes nothing; the smallest bad index -> head[0]) and
// leaves the largest target and source cell counts in head[1], head[2]; head: device int32[4], {INT_MAX, 0, 0, 0} before.
// sample_and_fit() enqueues expand -> matcher (cost only, around the centres) -> cov_fit_kernel.  Nothing is read back.
struct CovSamplePass {
  int n = 0, m = 0, spa = 0;
  size_t extra = 0;
  char* d_jobs = nullptr;
  cfear_reg_result* d_centre = nullptr;
  cfear_reg_result* d_samples = nullptr;
  char* d_block = nullptr;
  char* h_block = nullptr;
  void plan(HostStage& st, int n_jobs, int samples_per_axis, size_t extra_bytes);
  int stage(HostStage& st, const cfear_cov_sampling_params* sp);
  int upload(HostStage& st);
  size_t pinv_bytes() const { return (cfear_cov_fit_pinv_bytes(spa) + 255) / 256 * 256; }
  char* h_extra() const { return h_block + pinv_bytes(); }
  char* d_extra() const { return d_block + pinv_bytes(); }
  int centre(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* d_cands, const cfear_reg_result* d_regs, int n_jobs,
             const cfear_reg_params* par, int32_t* d_head) const;
  int sample_and_fit(cfear_ctx* ctx, const cfear_scan_table* table, const cfear_candidate* d_cands, int n_jobs, int max_tar_cells,
                     int max_src_cells, const cfear_reg_params* par, const cfear_reg_result* d_regs,
                     const cfear_cov_sampling_params* sp, double* d_cov36, int32_t* d_success) const;
};
