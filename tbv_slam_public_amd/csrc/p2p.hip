// p2p.hip -- point-to-point alignment quality and keypoint repeatability of two point clouds on gfx950.
//
// Replaces p2pQuality and keypointRepetability (coral_alignment_quality/src/alignment_checker/AlignmentQuality.cpp:235-328):
//   Tchange = Tref.inverse() * Tsrc * Toffset, src->GetCloudCopy(Tchange)          :260-264 (composed on the host: T[6])
//   pcl::KdTreeFLANN<PointXYZI>::radiusSearch over the reference cloud, sorted      :273-286, :303-318
//   residuals_ = nearest squared distance of every source point that has one        :283-285
//   GetQualityMeasure: mean over residuals_, which starts as {0, 0, 0}              :235-248, AlignmentQuality.h:92
//
// Kernel design: ONE persistent 1024-thread workgroup per reference cloud.  It sorts the cloud once into a uniform grid
// of radius * 1.0001 cells over its bounding box (gridsort.hpp's GridIndex, which coral.hip uses too: cell table, sorted points
// and an occupancy bitmap in LDS) and then serves every job that names the cloud -- the perturbations of a scan pair share
// both clouds, so the sort is paid once per pair.  Per job each lane takes one source point, transforms it
// (pcl::transformPointCloud's rounding), and takes the float minimum of FLANN's L2_Simple distance over the cells the
// ball can reach.  The cells are found from the interval [q - r_up, q + r_up] itself, not from "the 3 x 3 block": the cell
// function floorf(v * inv_cell) is monotone, so every reference coordinate inside the interval falls into a cell between
// the cells of its ends, whatever the rounding of v * inv_cell does.  matched and the per-point minima
// are exact; sum is reduced per thread in source order with stride 1024, then over a fixed tree.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <map>
#include <vector>

#include "common.hpp"
#include "gridsort.hpp"

namespace {

constexpr int kP2pThreads = kGridSortThreads;
constexpr int kP2pMaxRef = kGridSortMaxPoints;           // CFEAR_P2P_MAX_REF_POINTS
constexpr int kP2pMaxSrc = 1 << 20;                      // CFEAR_P2P_MAX_SRC_POINTS
constexpr float kP2pMaxCellIndex = 4194304.0f;           // |floorf(v * inv_cell)| below 2^22: exact in float, safe as int
static_assert(kP2pMaxRef == CFEAR_P2P_MAX_REF_POINTS && kP2pMaxSrc == CFEAR_P2P_MAX_SRC_POINTS, "limits stated in cfear_hip.h");

struct P2pJobDev {                    // one job, in the order of its group
  const float4* src;
  int32_t n_src;
  int32_t out;                        // index of the caller's job: results[out]
  long long pp_off;                   // first float of the job's per_point row
  double T[6];
};
struct P2pGroupDev {                  // one workgroup: a reference cloud and the jobs [job0, job1) that share it
  const float4* ref;
  int32_t n_ref, job0, job1, pad;
};
struct P2pCommon {
  float r2, inv_cell, r_up;
  int32_t cap;                        // reference points the per-workgroup scratch holds
  char* scratch;
  cfear_p2p_result* results;
  float* per_point;                   // nullable
};

typedef float v4f __attribute__((ext_vector_type(4)));
#define CFEAR_LDS __attribute__((address_space(3)))

__device__ __forceinline__ void write_record(const P2pCommon& cm, int out, double sum, int matched, int n_src, int status, int path = 0) {
  cfear_p2p_result r;
  r.sum = sum; r.mean = sum / (double)(matched + 3);     // residuals_ = {0, 0, 0} + the matches (AlignmentQuality.h:92)
  r.matched = matched; r.n_src = n_src; r.status = status; r.pad = path;           // path: CFEAR_CORAL_PATH_* of a served job (diagnostic)
  cm.results[out] = r;
}

__global__ __launch_bounds__(kP2pThreads) void p2p_kernel(const P2pGroupDev* __restrict__ groups, const P2pJobDev* __restrict__ jobs,
                                                          const P2pCommon cm) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  double* red_d = (double*)(smem + kGridSmallOff + 384);                // [2][16]
  int* red_m = (int*)(smem + kGridSmallOff + 640);                      // [2][16]
  int* red_b = (int*)(smem + kGridSmallOff + 768);                      // [2][16]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const P2pGroupDev g = groups[blockIdx.x];
  const int n = g.n_ref;
  // a reference cloud that cannot be served fails every job that names it; an empty source cloud is still "empty"
  auto fail_group = [&](int status) {
    for (int j = g.job0 + tid; j < g.job1; j += kP2pThreads) {
      const int ns = gload<int32_t>(&jobs[j].n_src);
      write_record(cm, gload<int32_t>(&jobs[j].out), 0.0, 0, max(ns, 0), ns <= 0 ? CFEAR_ERR_EMPTY_CLOUD : status);
    }
  };
  if (n <= 0) {                                                          // kdtree_.setInputCloud of an empty cloud
    if (cm.per_point)
      for (int j = g.job0; j < g.job1; j++)
        for (int i = tid; i < jobs[j].n_src; i += kP2pThreads) cm.per_point[jobs[j].pp_off + i] = -1.0f;
    fail_group(CFEAR_ERR_EMPTY_CLOUD);
    return;
  }
  if (n > cm.cap || n > kP2pMaxRef) { fail_group(CFEAR_ERR_CAPACITY); return; }
  // ---- 1. bounding box of the reference cloud (x, y); a NaN in x, y or z refuses the cloud -------------------------
  float mnx = FLT_MAX, mny = FLT_MAX, mxx = -FLT_MAX, mxy = -FLT_MAX;
  int nan_ref = 0;
  for (int i = tid; i < n; i += kP2pThreads) {
    const float4 p = gload_f4(g.ref + i);
    nan_ref |= (p.x != p.x) | (p.y != p.y) | (p.z != p.z);
    mnx = fminf(mnx, p.x); mxx = fmaxf(mxx, p.x);
    mny = fminf(mny, p.y); mxy = fmaxf(mxy, p.y);
  }
  block_bbox_f32(smem, mnx, mxx, mny, mxy, [&] { nan_ref = __syncthreads_or(nan_ref); });
  const float f_min_bx = floorf(mnx * cm.inv_cell), f_max_bx = floorf(mxx * cm.inv_cell);
  const float f_min_by = floorf(mny * cm.inv_cell), f_max_by = floorf(mxy * cm.inv_cell);
  // (written so that an infinite extent fails the test as well)
  const bool in_range = fabsf(f_min_bx) < kP2pMaxCellIndex && fabsf(f_max_bx) < kP2pMaxCellIndex &&
                        fabsf(f_min_by) < kP2pMaxCellIndex && fabsf(f_max_by) < kP2pMaxCellIndex;
  if (nan_ref || !in_range) { fail_group(CFEAR_ERR_CAPACITY); return; }
  const int min_bx = (int)f_min_bx, min_by = (int)f_min_by;
  const long long div_bx = (long long)f_max_bx - min_bx + 1, div_by = (long long)f_max_by - min_by + 1;
  if (div_bx * div_by > 0x7fffffffLL || div_by > kGridMaxRows) { fail_group(CFEAR_ERR_CAPACITY); return; }
  const int dbx = (int)div_bx, dby = (int)div_by;
  // the cell of a coordinate, relative to the grid's first cell and clamped to one cell outside it: monotone in v
  auto cell_x = [&](float v) { return (int)(fminf(fmaxf(floorf(v * cm.inv_cell), f_min_bx - 1.0f), f_max_bx + 1.0f) - f_min_bx); };
  auto cell_y = [&](float v) { return (int)(fminf(fmaxf(floorf(v * cm.inv_cell), f_min_by - 1.0f), f_max_by + 1.0f) - f_min_by); };
  auto ref_cell = [&](int i, int& ix, int& iy) {
    ix = cell_x(gload<float>(&g.ref[i].x));
    iy = cell_y(gload<float>(&g.ref[i].y));
  };
  // ---- 2, 3. the grid index (gridsort.hpp): sort by (cell, index), cell table, sorted points (x, y, z, 0) in LDS or in
  //      the scratch, bitmap or row table -------------------------------------------------------------------------------
  const GridIndex grid = grid_index_build(smem, n, dbx, dby, cm.scratch ? (float4*)(cm.scratch + (size_t)blockIdx.x * cm.cap * 16) : nullptr,
                                          ref_cell, [&](int, int idx) {
                                            const float4 p = gload_f4(g.ref + idx);
                                            return make_float4(p.x, p.y, p.z, 0.0f);
                                          });
  // ---- 4. the jobs of this cloud, one after the other; one source point per lane -----------------------------------
  auto serve = [&](auto* SP) {
    for (int j = g.job0; j < g.job1; j++) {
      const P2pJobDev* jb = jobs + j;
      const float4* src = (const float4*)gload<unsigned long long>(&jb->src);
      const int ns = gload<int32_t>(&jb->n_src);
      const long long pp_off = gload<long long>(&jb->pp_off);
      const double T0 = gload<double>(&jb->T[0]), T1 = gload<double>(&jb->T[1]), T2 = gload<double>(&jb->T[2]);
      const double T3 = gload<double>(&jb->T[3]), T4 = gload<double>(&jb->T[4]), T5 = gload<double>(&jb->T[5]);
      double sum = 0.0;
      int cnt = 0, bad = 0;
      for (int i = tid; i < ns; i += kP2pThreads) {
        const float4 p = gload_f4(src + i);
        // pcl::transformPointCloud<PointXYZI, double> (PCL 1.10 common/impl/transforms.hpp): float(((t0 x + t1 y) + t2 z) + t3)
        const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
        const float qx = (float)(((T0 * x + T1 * y) + 0.0 * z) + T2);
        const float qy = (float)(((T3 * x + T4 * y) + 0.0 * z) + T5);
        const float qz = p.z;
        bad |= (qx != qx) | (qy != qy) | (qz != qz);
        // the cells the ball can reach: [q - r_up, q + r_up] widened by more than the subtraction's rounding
        const float mx = (fabsf(qx) + cm.r_up) * 2.384185791015625e-07f, my = (fabsf(qy) + cm.r_up) * 2.384185791015625e-07f;
        const int x0 = max(cell_x((qx - cm.r_up) - mx), 0), x1 = min(cell_x((qx + cm.r_up) + mx), dbx - 1);
        const int y0 = max(cell_y((qy - cm.r_up) - my), 0), y1 = min(cell_y((qy + cm.r_up) + my), dby - 1);
        // a query at infinity (or NaN) has no neighbour -- d is never < r2 -- and its interval is not one: it scans nothing
        const bool finite = fabsf(qx) <= FLT_MAX && fabsf(qy) <= FLT_MAX;
        float best = FLT_MAX;
        bool found = false;
        auto visit = [&](const v4f c) {
          const float dx = __fsub_rn(qx, c.x), dy = __fsub_rn(qy, c.y), dz = __fsub_rn(qz, c.z);
          const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));   // FLANN L2_Simple
          if (d < cm.r2) {                                                                                 // RadiusResultSet: strict <
            found = true;
            best = fminf(best, d);
          }
        };
        if (finite && x0 <= x1)
          for (int yy = y0; yy <= y1; yy++) {
            int a, b;
            grid.run(yy, yy * dbx + x0, yy * dbx + x1 + 1, a, b);
            for (; a + 1 < b; a += 2) {
              const v4f c0 = SP[a], c1 = SP[a + 1];
              visit(c0);
              visit(c1);
            }
            if (a < b) visit(SP[a]);
          }
        if (cm.per_point) gstore<float>(cm.per_point + pp_off + i, found ? best : -1.0f);
        if (found) { sum += (double)best; cnt++; }
      }
      sum = wave_sum_lane63_f64(sum);
      cnt = wave_sum_i32(cnt);
      const int anybad = __ballot(bad != 0) != 0ull;
      const int buf = (j & 1) * 16;
      if (lane == 63) { red_d[buf + wave] = sum; red_m[buf + wave] = cnt; red_b[buf + wave] = anybad; }
      __syncthreads();
      if (tid == 0) {
        double s = 0.0;
        int m = 0, b = 0;
        for (int wv = 0; wv < 16; wv++) { s += red_d[buf + wv]; m += red_m[buf + wv]; b |= red_b[buf + wv]; }
        const int out = gload<int32_t>(&jb->out);
        if (ns <= 0) write_record(cm, out, 0.0, 0, 0, CFEAR_ERR_EMPTY_CLOUD);
        else if (b) write_record(cm, out, 0.0, 0, ns, CFEAR_ERR_CAPACITY);
        else write_record(cm, out, s, m, ns, CFEAR_OK, grid.path);
      }
    }
  };
  if (grid.spt_in_lds) serve((CFEAR_LDS const v4f*)grid.spt);
  else serve((const v4f*)grid.spt);
}

}  // namespace

extern "C" int cfear_p2p_quality_batch(cfear_ctx* ctx, const cfear_p2p_job* jobs, int32_t n_jobs, double radius,
                                       cfear_p2p_result* results, float* per_point) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !results || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (!(radius > 0.0) || !(radius <= DBL_MAX)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "radius must be > 0 and finite");
  if (n_jobs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsP2p);
  // jobs grouped by reference cloud, groups in the order of their first job, jobs of a group in the caller's order
  std::map<std::pair<const float*, int>, int> group_of;
  std::vector<std::vector<int>> members;
  size_t pp_total = 0;
  int cap = 1;
  for (int j = 0; j < n_jobs; j++) {
    const cfear_p2p_job& jb = jobs[j];
    if (jb.n_ref < 0 || jb.n_src < 0 || (jb.n_ref > 0 && !jb.ref_xyzi) || (jb.n_src > 0 && !jb.src_xyzi))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: null cloud", j);   // empty clouds are a per-job status
    if (jb.n_ref > kP2pMaxRef || jb.n_src > kP2pMaxSrc)
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "job %d: %d reference / %d source points exceed %d / %d", j, jb.n_ref, jb.n_src,
                             kP2pMaxRef, kP2pMaxSrc);
    for (int k = 0; k < 6; k++)
      if (!(std::fabs(jb.T[k]) <= DBL_MAX)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: T is not finite", j);
    cap = std::max(cap, jb.n_ref);
    st.cloud_in(jb.ref_xyzi, jb.n_ref);
    st.cloud_in(jb.src_xyzi, jb.n_src);
    const auto key = std::make_pair(jb.n_ref > 0 ? jb.ref_xyzi : (const float*)nullptr, jb.n_ref);
    auto it = group_of.find(key);
    if (it == group_of.end()) { it = group_of.emplace(key, (int)members.size()).first; members.emplace_back(); }
    members[it->second].push_back(j);
    pp_total += (size_t)jb.n_src;
  }
  // A cloud named by many jobs is split over several workgroups (each sorts it again) once there are fewer clouds than
  // compute units; a job's record does not depend on the split.
  const int n_clouds = (int)members.size();
  const int per_wg = n_clouds >= ctx->n_cu ? INT_MAX : std::max(4, (n_jobs + 2 * ctx->n_cu - 1) / (2 * ctx->n_cu));
  size_t n_groups = 0;
  for (const auto& m : members) n_groups += (m.size() + (size_t)per_wg - 1) / (size_t)per_wg;
  const size_t grp_bytes = (n_groups * sizeof(P2pGroupDev) + 255) / 256 * 256, job_bytes = (size_t)n_jobs * sizeof(P2pJobDev);
  char* d_rec;
  cfear_p2p_result* d_res;
  float* d_pp = nullptr;
  st.piece(d_rec, grp_bytes + job_bytes);
  st.out(d_res, results, (size_t)n_jobs * sizeof(cfear_p2p_result));
  if (per_point && pp_total) st.out(d_pp, per_point, pp_total * sizeof(float));
  // the sorted cloud of a workgroup leaves the LDS above ~5460 points (24 bytes a point with its cell table)
  const size_t scratch_stride = (size_t)cap * 16;
  const bool need_scratch = (size_t)cap * 24 + 64 > kGridRowbegOff;
  // with a scratch, a launch holds two workgroups per compute unit: the slot is grow-only, and more than the resident
  // workgroups' worth of it buys nothing (at most 2 n_cu x 256 KiB)
  const size_t chunk = need_scratch ? std::max<size_t>(1, std::min<size_t>(n_groups, 2 * (size_t)std::max(ctx->n_cu, 1))) : n_groups;
  char* scr = need_scratch ? (char*)cfear_workspace(ctx, kWsP2pScratch, scratch_stride * chunk) : nullptr;
  if (need_scratch && !scr) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  CFEAR_CHECK(st.carve());
  char* h_rec = (char*)st.pinned(grp_bytes + job_bytes);
  if (!h_rec) return CFEAR_ERR_HIP;
  P2pGroupDev* hg = (P2pGroupDev*)h_rec;
  P2pJobDev* hj = (P2pJobDev*)(h_rec + grp_bytes);
  {
    std::vector<long long> pp_off((size_t)n_jobs);
    long long run = 0;
    for (int j = 0; j < n_jobs; j++) { pp_off[j] = run; run += jobs[j].n_src; }
    size_t gi = 0;
    int ji = 0;
    for (const auto& m : members)
      for (size_t b = 0; b < m.size(); b += (size_t)per_wg) {
        const size_t e = std::min(m.size(), b + (size_t)per_wg);
        const cfear_p2p_job& first = jobs[m[b]];
        hg[gi++] = P2pGroupDev{first.n_ref > 0 ? st.cloud(first.ref_xyzi) : nullptr, first.n_ref, ji, ji + (int)(e - b), 0};
        for (size_t k = b; k < e; k++) {
          const cfear_p2p_job& jb = jobs[m[k]];
          P2pJobDev& o = hj[ji++];
          o.src = jb.n_src > 0 ? st.cloud(jb.src_xyzi) : nullptr;
          o.n_src = jb.n_src; o.out = m[k]; o.pp_off = pp_off[m[k]];
          for (int t = 0; t < 6; t++) o.T[t] = jb.T[t];
        }
      }
  }
  CFEAR_CHECK(st.upload(d_rec, h_rec, grp_bytes + job_bytes));
  P2pCommon cm;
  cm.r2 = (float)(radius * radius);                      // radiusSearch passes float(radius * radius) to FLANN
  cm.inv_cell = (float)(1.0 / (radius * 1.0001));
  cm.r_up = std::nextafterf((float)(radius * 1.0001), FLT_MAX);
  cm.cap = cap;
  cm.results = d_res;
  cm.per_point = d_pp;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)p2p_kernel, kGridLdsTotal));   // (+ the static word of __syncthreads_or)
  {
    ProfScope ps(ctx, "p2p_quality");
    for (size_t g0 = 0; g0 < n_groups; g0 += chunk) {
      const size_t ng = std::min(chunk, n_groups - g0);
      cm.scratch = scr;
      hipLaunchKernelGGL(p2p_kernel, dim3((unsigned)ng), dim3(kP2pThreads), kGridLdsTotal, ctx->stream,
                         (const P2pGroupDev*)d_rec + g0, (const P2pJobDev*)(d_rec + grp_bytes), cm);
    }
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  CFEAR_CHECK(st.finish());
  if (!cfear_is_device_ptr(results))                     // records in device memory are the caller's to read: the call stays asynchronous
    for (int j = 0; j < n_jobs; j++)
      if (results[j].status != CFEAR_OK && results[j].status != CFEAR_ERR_EMPTY_CLOUD)
        return cfear_set_error(ctx, results[j].status, "job %d: %s", j, cfear_status_string(results[j].status));
  return CFEAR_OK;
}

extern "C" int cfear_p2p_quality(cfear_ctx* ctx, const cfear_p2p_job* job, double radius, cfear_p2p_result* result, float* per_point) {
  return cfear_p2p_quality_batch(ctx, job, 1, radius, result, per_point);
}
