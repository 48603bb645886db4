// tieaudit.hip -- which registrations hang on a nearest-neighbour tie: a diagnostic, not a stage.
//
// Replays the association step of n_scan_normal_reg::AddScanPairCost (n_scan_normal.cpp:213-261) for a batch of jobs at
// the poses it is given and keeps ALL minimisers of every 1-NN query, where MapPointNormal::GetClosestIdx
// (pointnormal.cpp:238-254) -- FLANN's nearestKSearch(k = 1) -- returns one of them and the matcher the lowest index.
//   tie_audit_kernel     one workgroup per (job, fixed target scan): counters per job, optionally the tie group of every query
//   closest_ties_kernel  the same inner loop for caller-supplied queries against one scan: the tie-aware GetClosestIdx
// The search is brute force over the target's float means, tile by tile through LDS: the audit must not share the grid
// search it audits (matcher.hip, mt_associate), and a scan holds a few hundred cells.
#include <algorithm>
#include <cmath>

#include "fastmath.hpp"
#include "registration.hpp"

namespace {

constexpr int kTieThreads = 256;
constexpr int kTieTile = CFEAR_TIE_TILE;      // target means per LDS tile (8 KB)

// One job: the sizes the host read from the handles (cfear_scan_size), where its per-query block starts, the status
// cfear_get_cost_batch would refuse it with, then poses and scan views -- the views LAST, so that a batch is stored with
// the stride of its longest job (as reg_job_stride does for the matcher's records).
struct TieJob {
  int32_t n_scans;
  int32_t cap_status;                         // CFEAR_OK, or CFEAR_ERR_CAPACITY: a cost-only launch cannot hold the job
  int64_t q_off;                              // first per-query entry of the job
  int32_t n_cells[kRegMaxScans];
  double poses[kRegMaxScans][3];
  ScanView scans[kRegMaxScans];
};
size_t tie_job_stride(int max_scans) { return reg_record_stride(offsetof(TieJob, scans), max_scans); }

// Tsrctotar = Ttar^-1 * Tsrc (n_scan_normal.cpp:222) with the matcher's two rotations: libm for the fixed scan
// (mt_stage_once), the polynomial sincos of the evaluation points for the source (mt_associate)
__device__ __forceinline__ Aff2 tie_src_to_tar(const double* tar, const double* src) {
  double st, ct, ss, cs;
  sincos(tar[2], &st, &ct);
  if (fabs(src[2]) <= 1e5) sincos_reduced<true>(src[2], &ss, &cs);
  else sincos(src[2], &ss, &cs);
  return aff_mul(aff_inv(aff_from_cs(ct, st, tar[0], tar[1])), aff_from_cs(cs, ss, src[0], src[1]));
}

// cells a and b differ in something the residual or the weight reads (mean, normal, cov, scale, nsamples), bit for bit
__device__ __forceinline__ bool tie_cells_differ(const ScanView& v, int a, int b) {
  typedef unsigned long long g_u64x2 __attribute__((ext_vector_type(2)));
  typedef unsigned long long g_u64x4 __attribute__((ext_vector_type(4)));
  const g_u64x2 ma = gload<g_u64x2>(v.mean + a), mb = gload<g_u64x2>(v.mean + b);
  const g_u64x2 na = gload<g_u64x2>(v.normal + a), nb = gload<g_u64x2>(v.normal + b);
  const g_u64x4 ca = gload<g_u64x4>(v.cov + a), cb = gload<g_u64x4>(v.cov + b);
  const unsigned long long sa = gload<unsigned long long>(v.scale + a), sb = gload<unsigned long long>(v.scale + b);
  const int ka = gload<int>(v.nsamples + a), kb = gload<int>(v.nsamples + b);
  return ((ma.x ^ mb.x) | (ma.y ^ mb.y) | (na.x ^ nb.x) | (na.y ^ nb.y) | (ca.x ^ cb.x) | (ca.y ^ cb.y) | (ca.z ^ cb.z) |
          (ca.w ^ cb.w) | (sa ^ sb)) != 0ull || ka != kb;
}

// All minimisers of one query: the nearest float distance, the lowest and the highest cell that has it, how many do.
struct TieGroup {
  float best = 0.f;
  int lo = -1, hi = -1, count = 0;
  bool differs = false;
};

// The workgroup sweeps the n cells of `v` for one query per thread (L2_Simple in float: d = dx * dx, d += dy * dy, unfused:
// -ffp-contract=off).  Every thread of the workgroup calls it -- the tile staging has barriers; a thread without a query
// passes live = false.  DIFF: also compare tied cells with the lowest one.
template <bool DIFF>
__device__ __forceinline__ TieGroup tie_sweep(const ScanView& v, const int n, const float qx, const float qy, const bool live,
                                              float2* tile, bool& staged) {
  TieGroup g;
  for (int t0 = 0; t0 < n; t0 += kTieTile) {
    const int m = min(kTieTile, n - t0);
    if (!(staged && n <= kTieTile)) {           // a target of one tile stays in LDS across the workgroup's queries
      __syncthreads();
      for (int j = threadIdx.x; j < m; j += kTieThreads) {
        const g_f32x2 c = gload<g_f32x2>(v.mean_f + t0 + j);
        tile[j] = make_float2(c.x, c.y);
      }
      __syncthreads();
      staged = true;
    }
    if (!live) continue;
    for (int j = 0; j < m; j++) {
      const float2 c = tile[j];
      const float dx = qx - c.x, dy = qy - c.y;
      float d = dx * dx;
      d += dy * dy;
      if (g.count == 0 || d < g.best) { g.best = d; g.lo = g.hi = t0 + j; g.count = 1; g.differs = false; }
      else if (d == g.best) {
        g.hi = t0 + j; g.count++;
        if (DIFF && !g.differs) g.differs = tie_cells_differ(v, t0 + j, g.lo);
      }
    }
  }
  return g;
}

__global__ __launch_bounds__(kTieThreads) void tie_audit_kernel(const char* __restrict__ jobs, const size_t job_stride, const double radius,
                                                                const int itr, const double angle_outlier,
                                                                cfear_tie_record* __restrict__ records, int32_t* __restrict__ per_query) {
  __shared__ float2 tile[kTieTile];
  const TieJob& job = *(const TieJob*)(jobs + (size_t)blockIdx.x * job_stride);
  const int last = job.n_scans - 1, t = blockIdx.y;
  if (t >= last) return;                                   // (block-uniform: the grid's y is the batch's longest job)
  const ScanView& tar = job.scans[t];
  const ScanView& src = job.scans[last];
  const int n_tar = job.n_cells[t], n_src = job.n_cells[last];
  const Aff2 T = tie_src_to_tar(job.poses[t], job.poses[last]);
  const double r = (itr == 1) ? 2 * radius : radius;       // n_scan_normal.cpp:220
  const double r2 = r * r;
  int32_t* pq = per_query ? per_query + 3 * (job.q_off + (int64_t)t * n_src) : nullptr;
  int c_in = 0, c_assoc = 0, c_tied = 0, c_eff = 0, c_max = 0, c_q = 0;
  bool staged = false;
  for (int s0 = 0; s0 < n_src; s0 += kTieThreads) {        // this thread's source cells: tid, tid + 256, ...
    const int s = s0 + (int)threadIdx.x;
    const bool live = s < n_src;
    float qx = 0.f, qy = 0.f;
    if (live) {
      const double2 u = gload_d2(src.mean + s);
      qx = (float)(T.l0 * u.x + T.l1 * u.y + T.t0);        // pointnormal.cpp:240-242
      qy = (float)(T.l2 * u.x + T.l3 * u.y + T.t1);
    }
    const TieGroup g = tie_sweep<true>(tar, n_tar, qx, qy, live, tile, staged);
    if (!live) continue;
    const bool in_r = g.count > 0 && (double)g.best < r2;  // pointnormal.cpp:250 (a NaN distance is never inside)
    c_q++;
    if (in_r) {
      const double2 ns = gload_d2(src.normal + s), nt = gload_d2(tar.normal + g.lo);
      const double nsx = T.l0 * ns.x + T.l1 * ns.y, nsy = T.l2 * ns.x + T.l3 * ns.y;
      c_in++;
      c_assoc += fmax(nsx * nt.x + nsy * nt.y, 0.0) > angle_outlier;     // n_scan_normal.cpp:244-245, on the lowest winner
      c_tied += g.count >= 2;
      c_eff += g.count >= 2 && g.differs;
      c_max = max(c_max, g.count);
    }
    if (pq) { pq[3 * s] = in_r ? g.lo : -1; pq[3 * s + 1] = in_r ? g.hi : -1; pq[3 * s + 2] = in_r ? g.count : 0; }
  }
  // the wavefront's sums, then one vector atomic per counter: integer sums, so the record does not depend on the order
  c_q = wave_sum_i32(c_q); c_in = wave_sum_i32(c_in); c_assoc = wave_sum_i32(c_assoc);
  c_tied = wave_sum_i32(c_tied); c_eff = wave_sum_i32(c_eff);
  c_max = __builtin_amdgcn_readlane(wave_incl_scan_max_i32(c_max), 63);
  if ((threadIdx.x & 63) == 0) {
    cfear_tie_record* rec = records + blockIdx.x;
    atomicAdd(&rec->n_queries, c_q); atomicAdd(&rec->n_in_radius, c_in); atomicAdd(&rec->n_associated, c_assoc);
    atomicAdd(&rec->n_tied, c_tied); atomicAdd(&rec->n_tied_effective, c_eff); atomicMax(&rec->max_group, c_max);
  }
}

// behind the audit: a job's status is what cfear_get_cost_batch would report (n_scan_normal.cpp:200-203 on the blocks counted)
__global__ __launch_bounds__(kTieThreads) void tie_status_kernel(const char* __restrict__ jobs, const size_t job_stride, const int n_jobs,
                                                                 const int residuals_per_block, cfear_tie_record* __restrict__ records) {
  const int j = blockIdx.x * kTieThreads + threadIdx.x;
  if (j >= n_jobs) return;
  const TieJob& job = *(const TieJob*)(jobs + (size_t)j * job_stride);
  const bool few = records[j].n_associated * residuals_per_block <= 1;
  records[j].status = job.cap_status != CFEAR_OK ? job.cap_status : (few ? CFEAR_ERR_TOO_FEW_RESIDUALS : CFEAR_OK);
  records[j].pad = 0;
}

__global__ __launch_bounds__(kTieThreads) void closest_ties_kernel(const ScanView v, const int n_cells, const double2* __restrict__ q,
                                                                   const int nq, const double d2, int32_t* __restrict__ lo,
                                                                   int32_t* __restrict__ hi, int32_t* __restrict__ count) {
  __shared__ float2 tile[kTieTile];
  const int i = blockIdx.x * kTieThreads + threadIdx.x;
  const bool live = i < nq;
  float qx = 0.f, qy = 0.f;
  if (live) { const double2 p = q[i]; qx = (float)p.x; qy = (float)p.y; }     // pnt.x = p(0): double -> float
  bool staged = false;
  const TieGroup g = tie_sweep<false>(v, n_cells, qx, qy, live, tile, staged);
  if (!live) return;
  const bool in_r = g.count > 0 && (double)g.best < d2;
  lo[i] = in_r ? g.lo : -1;
  if (hi) hi[i] = in_r ? g.hi : -1;
  if (count) count[i] = in_r ? g.count : 0;
}

}  // namespace

extern "C" int cfear_association_ties_batch(cfear_ctx* ctx, const cfear_reg_job* jobs, int32_t n_jobs, const cfear_reg_params* par,
                                            int32_t itr, cfear_tie_record* records, int32_t* per_query, int64_t per_query_len) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !records || !par) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_jobs < 0 || itr < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_jobs and itr must not be negative");
  CFEAR_CHECK(cfear_check_reg_params(ctx, par));
  if (n_jobs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int max_scans = 2;
  for (int j = 0; j < n_jobs; j++) max_scans = std::max(max_scans, std::min((int)jobs[j].n_scans, kRegMaxScans));
  HostStage st(ctx, kWsTieAudit);
  const size_t stride = tie_job_stride(max_scans), jb_bytes = (size_t)n_jobs * stride;
  char* hjobs = (char*)st.pinned(jb_bytes);
  if (!hjobs) return CFEAR_ERR_HIP;
  int64_t total = 0;
  for (int j = 0; j < n_jobs; j++) {
    const cfear_reg_job& jb = jobs[j];
    RegJobCells cells;
    CFEAR_CHECK(cfear_reg_check_job(ctx, jb.scans, jb.n_scans, jb.poses_xyt, j, true, &cells));
    TieJob* tj = (TieJob*)(hjobs + (size_t)j * stride);
    const int last = jb.n_scans - 1;
    tj->n_scans = jb.n_scans;
    tj->q_off = total;
    for (int i = 0; i < jb.n_scans; i++) {
      tj->n_cells[i] = cells.n[i];
      tj->scans[i] = jb.scans[i]->view;
      for (int k = 0; k < 3; k++) tj->poses[i][k] = jb.poses_xyt[3 * i + k];
    }
    tj->cap_status = cfear_reg_cost_fits(par, jb.n_scans, cells.sum_pad, cells.max_pad, cells.n[last]) ? CFEAR_OK : CFEAR_ERR_CAPACITY;
    total += (int64_t)cells.n[last] * last;
  }
  if (per_query && per_query_len < total)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "per_query holds %lld entries, the batch has %lld queries", (long long)per_query_len,
                           (long long)total);
  char* d_jobs;
  cfear_tie_record* d_rec;
  int32_t* d_pq = nullptr;
  st.piece(d_jobs, jb_bytes);
  st.out(d_rec, records, (size_t)n_jobs * sizeof(cfear_tie_record));
  if (per_query && total > 0) st.out(d_pq, per_query, (size_t)total * 12);
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "records and per_query must both be host or both be device memory");
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(st.upload(d_jobs, hjobs, jb_bytes));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(d_rec, 0, (size_t)n_jobs * sizeof(cfear_tie_record), ctx->stream));
  {
    ProfScope ps(ctx, "tie_audit");
    hipLaunchKernelGGL(tie_audit_kernel, dim3(n_jobs, max_scans - 1), dim3(kTieThreads), 0, ctx->stream, d_jobs, stride, par->radius, (int)itr,
                       std::cos(M_PI / 6.0), d_rec, d_pq);                 // n_scan_normal.cpp:217
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(tie_status_kernel, dim3((n_jobs + kTieThreads - 1) / kTieThreads), dim3(kTieThreads), 0, ctx->stream, d_jobs, stride,
                       (int)n_jobs, par->cost == CFEAR_P2L ? 1 : 2, d_rec);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  return st.finish();
}

extern "C" int cfear_scan_closest_ties(const cfear_scan* scan, const double* queries_xy, int32_t n_queries, double d, int32_t* lo,
                                       int32_t* hi, int32_t* count) {
  if (!scan) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = scan->ctx;
  if (!queries_xy || !lo || n_queries < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (!(d > 0)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "d must be greater than 0");
  if (n_queries == 0) return CFEAR_OK;
  const int n = cfear_scan_size(scan);
  if (n < 0) return n;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsTieAudit);
  const double2* dq;
  int32_t *dlo, *dhi = nullptr, *dcnt = nullptr;
  st.in(dq, (const double2*)queries_xy, (size_t)n_queries * 16);
  st.out(dlo, lo, (size_t)n_queries * 4);
  if (hi) st.out(dhi, hi, (size_t)n_queries * 4);
  if (count) st.out(dcnt, count, (size_t)n_queries * 4);
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "queries, lo, hi and count must all be host or all be device memory");
  CFEAR_CHECK(st.carve());
  hipLaunchKernelGGL(closest_ties_kernel, dim3((n_queries + kTieThreads - 1) / kTieThreads), dim3(kTieThreads), 0, ctx->stream, scan->view, n,
                     dq, (int)n_queries, d * d, dlo, dhi, dcnt);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}
