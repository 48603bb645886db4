// coral.hip -- CorAl alignment quality of two radar peak clouds on gfx950.
//
// Replaces CorAlRadarQuality (coral_alignment_quality/src/alignment_checker/AlignmentQuality.cpp:8-230)
// as TBV calls it for loop-closure verification and classifier training
// (alignmentinterface.cpp:296-347, 437-456: kstrongStructuredRadar scans from the stored peak clouds,
// radius 1.0, ent_cfg = any -> ComputeEntropy, output_overlap = true):
//   PoseScan::GetCloudCopy + pcl3dto2d            ScanType.cpp:211-215, Utils.cpp:200-212
//   GetNearby (two pcl::KdTreeFLANN radius searches)  AlignmentQuality.cpp:8-29
//   Covariance / ComputeEntropy                   :30-53, :80-98
//   per-point loops and aggregation               :132-204
// The ent_cfg = kl branch (ComputeKLDiv, :54-78) is never selected by TBV and is not built.
//
// Kernel design: ONE 1024-thread workgroup per (ref, src, Toffset) job, one launch per batch.  The two
// kd-trees are replaced by ONE sort-based uniform grid over the merged cloud (cell >= radius, so every
// neighbour of a query lies in the 3 x 3 cells around it; gridsort.hpp): each merged point is a query
// once and accumulates, in a single pass over the contiguous runs of the sorted array, the fp64 moments
// of its source-cloud and reference-cloud neighbours separately -- the joint neighbourhood is their sum,
// so the reference's two radius searches + three matrix copies per point become one sweep.  The float
// squared distance test is FLANN's L2_Simple (`dist < r^2`, strict).  Per-point entropies are written by
// original index and reduced in index order (fixed tree), so results do not depend on scheduling.
// Working set per job: a few hundred KB in LDS + L2; nothing here is HBM-bound.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.hpp"
#include "gridsort.hpp"
#include "pose2d.hpp"

namespace {

constexpr int kCoralThreads = kGridSortThreads;
constexpr int kCoralMaxPoints = kGridSortMaxPoints;      // merged points per job

// (struct CoralJob: common.hpp -- verify.hip's kernels write job records too)

struct CoralCommon {
  double radius;
  float r2, inv_cell;
  int32_t weight_res_intensity;
  int32_t cap;                        // merged-point capacity of the per-job scratch
  char* scratch;
  size_t scratch_stride;
  cfear_coral_result* results;
  double* per_point;                  // nullable: [n_jobs][cap][3] joint_res, sep_res, valid
};

__host__ __device__ inline size_t coral_scratch_bytes(int cap) {
  // sorted points float4 | joint_res f64 | sep_res f64 | weight f64 (0 = invalid) | valid i32 | work list i32
  return ((size_t)cap * (16 + 8 + 8 + 8 + 4 + 4) + 255) / 256 * 256;
}

// pcl::transformPointCloud<PointXYZI, double> (PCL 1.10 common/impl/transforms.hpp): float(((t0 x + t1 y) + t2 z) + t3)
__device__ __forceinline__ float2 tf_point(const float4 p, const Aff2& T) {
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  return make_float2((float)(((T.l0 * x + T.l1 * y) + 0.0 * z) + T.t0), (float)(((T.l2 * x + T.l3 * y) + 0.0 * z) + T.t1));
}

struct Moments { int n; double sx, sy, sxx, sxy, syy; };
typedef float v4f __attribute__((ext_vector_type(4)));
#define CFEAR_LDS __attribute__((address_space(3)))

// CorAlRadarQuality::Covariance (:30-53) from the moments of d = p - q about the query q: the mean shift
// cancels in the covariance, |d| < radius keeps the one-pass form accurate to a few ulp.
__device__ __forceinline__ bool cov_from_moments(const Moments& m, double& c00, double& c01, double& c11) {
  if (m.n <= 2) return false;                                                  // x.rows() <= 2
  const double n = (double)m.n;
  const double mx = m.sx / n, my = m.sy / n;
  const double den = (double)(float)m.n - 1.0;                                 // `float n = x.rows()`; cov = covSum*1.0/(n-1.0)
  c00 = (m.sxx - n * mx * mx) * 1.0 / den;
  c01 = (m.sxy - n * mx * my) * 1.0 / den;
  c11 = (m.syy - n * my * my) * 1.0 / den;
  return true;
}

__device__ __forceinline__ void fail_job(const CoralCommon& cm, int status) {
  if (threadIdx.x == 0) {
    cfear_coral_result& r = cm.results[blockIdx.x];
    r.joint = r.sep = r.overlap = 0.0; r.valid = 0; r.count_valid = 0; r.status = status; r.pad = 0;
  }
}

__global__ __launch_bounds__(kCoralThreads) void coral_kernel(const CoralJob* __restrict__ jobs, const CoralCommon cm) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int* red_i = (int*)(smem + kGridSmallOff + 256);                      // [16] (the index builder's; free afterwards)
  double* red_d = (double*)(smem + kGridSmallOff + 384);                // [16][3] + counts
  int* red_c = (int*)(smem + kGridSmallOff + 384 + 16 * 3 * 8);         // [16]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const CoralJob job = jobs[blockIdx.x];
  const int n_src = job.n_src_ptr ? *job.n_src_ptr : job.n_src;
  const int n_ref = job.n_ref_ptr ? *job.n_ref_ptr : job.n_ref;
  const int n = n_src + n_ref;
  if (n_src <= 0 || n_ref <= 0) { fail_job(cm, CFEAR_ERR_EMPTY_CLOUD); return; }         // assert(size() > 0) (:118)
  if (n > cm.cap || n > kCoralMaxPoints) { fail_job(cm, CFEAR_ERR_CAPACITY); return; }
  char* scr = cm.scratch + (size_t)blockIdx.x * cm.scratch_stride;
  float4* scr_pts = (float4*)scr;                              // the sorted merged points, when they do not fit the LDS
  double* jres = (double*)(scr_pts + cm.cap);
  double* sres = jres + cm.cap;
  double* wres = sres + cm.cap;
  int32_t* vres = (int32_t*)(wres + cm.cap);
  int32_t* work = vres + cm.cap;                               // sorted positions of the points that overlap the other cloud

#ifdef CFEAR_CORAL_TIMING
  long long tq[8]; tq[0] = __builtin_readcyclecounter();
#define CORAL_T(k) tq[k] = __builtin_readcyclecounter()
#else
#define CORAL_T(k)
#endif
  const Aff2 Tref = aff_from_xyt(job.ref_pose);
  const Aff2 Tsrc = aff_mul(aff_from_xyt(job.src_pose), aff_from_xyt(job.offset));            // src->GetAffine() * Toffset (:101)
  auto point = [&](int i) -> float2 {                          // merged index: source points first (:132, :155)
    const bool s = i < n_src;                                  // (the transform selected field by field: both stay in registers)
    const Aff2 T{s ? Tsrc.l0 : Tref.l0, s ? Tsrc.l1 : Tref.l1, s ? Tsrc.l2 : Tref.l2, s ? Tsrc.l3 : Tref.l3, s ? Tsrc.t0 : Tref.t0, s ? Tsrc.t1 : Tref.t1};
    return tf_point(gload_f4(s ? job.src + i : job.ref + (i - n_src)), T);   // (global_load: gload's comment in common.hpp)
  };
  // ---- 1. bounding box of the merged cloud ------------------------------------------------------
  float mnx = FLT_MAX, mny = FLT_MAX, mxx = -FLT_MAX, mxy = -FLT_MAX;
  for (int i = tid; i < n; i += kCoralThreads) {
    const float2 p = point(i);
    mnx = fminf(mnx, p.x); mxx = fmaxf(mxx, p.x);
    mny = fminf(mny, p.y); mxy = fmaxf(mxy, p.y);
  }
  block_bbox_f32(smem, mnx, mxx, mny, mxy, [] { __syncthreads(); });
  const int min_bx = (int)floorf(mnx * cm.inv_cell), max_bx = (int)floorf(mxx * cm.inv_cell);
  const int min_by = (int)floorf(mny * cm.inv_cell), max_by = (int)floorf(mxy * cm.inv_cell);
  const long long div_bx = (long long)max_bx - min_bx + 1, div_by = (long long)max_by - min_by + 1;
  if (!(mnx == mnx) || !(mny == mny) || div_bx * div_by > 0x7fffffffLL || div_by > kGridMaxRows) {
    fail_job(cm, CFEAR_ERR_CAPACITY);
    return;
  }
  const int dbx = (int)div_bx, dby = (int)div_by;
  auto cell_xy = [&](float2 p, int& ix, int& iy) {
    ix = (int)(floorf(p.x * cm.inv_cell) - (float)min_bx);
    iy = (int)(floorf(p.y * cm.inv_cell) - (float)min_by);
  };
  CORAL_T(1);
  // ---- 2, 3. the grid index (gridsort.hpp): sort by (cell, index), cell table, sorted points (x, y, intensity, original
  //      index) in LDS or in the scratch, bitmap or row table.  g.path: cfear_coral_result.pad (diagnostic) -------------
  const GridIndex g = grid_index_build(
      smem, n, dbx, dby, scr_pts, [&](int i, int& ix, int& iy) { cell_xy(point(i), ix, iy); },
      [&](int, int idx) {
        const float2 p = point(idx);
        const float inten = idx < n_src ? gload<float>(&job.src[idx].w) : gload<float>(&job.ref[idx - n_src].w);
        return make_float4(p.x, p.y, inten, __int_as_float(idx));
      }
#ifdef CFEAR_CORAL_TIMING
      , &tq[2]
#endif
  );
  // the three candidate runs of a query in cell (ix, iy): rows iy - 1 .. iy + 1, columns ix - 1 .. ix + 1 (empty outside the grid)
  auto runs_of = [&](int ix, int iy, int* r0, int* r1) {
    const int x0 = max(ix - 1, 0), x1 = min(ix + 1, dbx - 1);
#pragma unroll
    for (int d = 0; d < 3; d++) {
      const int yy = iy - 1 + d;
      const bool in = yy >= 0 && yy < dby;
      const int cy = in ? yy : 0;
      int a, b;
      g.run(cy, cy * dbx + x0, cy * dbx + x1 + 1, a, b);
      r0[d] = in ? a : 0; r1[d] = in ? b : 0;
    }
  };
  CORAL_T(3);
  int* n_work = red_i;                                          // LDS counter
  if (tid == 0) *n_work = 0;
  __syncthreads();
  // ---- 4. moments of the source / reference neighbours of every point -> entropies -----------------------------
  // Both passes are instantiated per address space of the sorted points (ds_read_b128 when they sit in LDS) and visit the
  // candidates in one order whatever the lookup, so the fp64 sums do not depend on the path.
  // Pass A (cheap, every point): does the point have ANY neighbour of the other cloud within the radius (overlap_req_ = 1,
  // :138, :160)?  Float distance tests only, first hit ends the search.  Points without one are final (100, 100,
  // invalid); the others go to a work list.  Pass B (expensive, work list only): fp64 moments and entropies -- typically
  // a quarter to a half of the points, spread evenly over the workgroup.
  auto find_overlap = [&](auto* SP) {
    for (int e0 = 0; e0 < n; e0 += kCoralThreads) {
      const int e = e0 + tid;
      bool hit = false;
      if (e < n) {
        const v4f q = SP[e];
        const int idx = __float_as_int(q.w);
        const bool q_is_src = idx < n_src;
        int ix, iy, r0[3], r1[3];
        cell_xy(make_float2(q.x, q.y), ix, iy);
        runs_of(ix, iy, r0, r1);
        auto test = [&](const v4f c) {
          const float dxf = __fsub_rn(q.x, c.x), dyf = __fsub_rn(q.y, c.y);
          const float d2 = __fadd_rn(__fmul_rn(dxf, dxf), __fmul_rn(dyf, dyf));
          return (d2 < cm.r2) && ((__float_as_int(c.w) < n_src) != q_is_src);
        };
        // the three runs as ONE sequence, the point's own row first (the nearest returns of the other cloud usually share
        // it); four independent loads per exit test
        const int n0 = r1[1] - r0[1], n01 = n0 + (r1[0] - r0[0]), C = n01 + (r1[2] - r0[2]);
        auto at = [&](int j) { return j < n0 ? r0[1] + j : (j < n01 ? r0[0] + (j - n0) : r0[2] + (j - n01)); };
        for (int j = 0; j < C && !hit; j += 4) {
          const v4f c0 = SP[at(j)], c1 = SP[at(min(j + 1, C - 1))], c2 = SP[at(min(j + 2, C - 1))], c3 = SP[at(min(j + 3, C - 1))];
          hit = ((int)test(c0) | (int)test(c1) | (int)test(c2) | (int)test(c3)) != 0;
        }
        if (!hit) { gstore<double>(jres + idx, 100.0); gstore<double>(sres + idx, 100.0); gstore<double>(wres + idx, 0.0); gstore<int32_t>(vres + idx, 0); }
      }
      const unsigned long long m = __ballot(hit);                // wave-aggregated append
      int base = 0;
      if (lane == 0 && m) base = atomicAdd(n_work, __popcll(m));
      base = __shfl(base, 0);
      if (hit) gstore<int32_t>(work + base + __popcll(m & ((1ull << lane) - 1ull)), e);
    }
  };
  // Pass B: one lane per point of the work list.  (Lane groups for the heavy neighbourhoods -- sixteen lanes per point with
  // more than 48 candidates, four above 12, DPP all-reduces of the partial moments -- were measured in round 4: the jobs
  // that take 2.5 x the sweep time of the rest are not held up by a few heavy lanes, they simply visit more candidates; the
  // classification pass cost more than the balance gained: 55 k cycles against 50 k per job.  Two lanes per point: equal.)
  auto sweep = [&](auto* SP, const int W) {
    for (int k = tid; k < W; k += kCoralThreads) {
      const int e = gload<int32_t>(work + k);
      const v4f q = SP[e];
      const int idx = __float_as_int(q.w);
      const bool q_is_src = idx < n_src;
      int ix, iy, r0[3], r1[3];
      cell_xy(make_float2(q.x, q.y), ix, iy);
      runs_of(ix, iy, r0, r1);
      Moments ms{0, 0, 0, 0, 0, 0}, mr{0, 0, 0, 0, 0, 0};
      const double qx = (double)q.x, qy = (double)q.y;
      auto visit = [&](const v4f c) {
        const float dxf = __fsub_rn(q.x, c.x), dyf = __fsub_rn(q.y, c.y);
        const float d2 = __fadd_rn(__fmul_rn(dxf, dxf), __fmul_rn(dyf, dyf));  // FLANN L2_Simple
        if (d2 < cm.r2) {                                                       // RadiusResultSet: strict <
          const double dx = (double)c.x - qx, dy = (double)c.y - qy;
          if (__float_as_int(c.w) < n_src) {
            ms.n++; ms.sx += dx; ms.sy += dy; ms.sxx += dx * dx; ms.sxy += dx * dy; ms.syy += dy * dy;
          } else {
            mr.n++; mr.sx += dx; mr.sy += dy; mr.sxx += dx * dx; mr.sxy += dx * dy; mr.syy += dy * dy;
          }
        }
      };
      {                                                          // the three runs as ONE sequence, rows in order, two loads in flight
        const int n0 = r1[0] - r0[0], n01 = n0 + (r1[1] - r0[1]), C = n01 + (r1[2] - r0[2]);
        auto at = [&](int j) { return j < n0 ? r0[0] + j : (j < n01 ? r0[1] + (j - n0) : r0[2] + (j - n01)); };
        for (int j = 0; j < C; j += 2) {
          const bool two = j + 1 < C;
          const v4f c0 = SP[at(j)], c1 = SP[at(two ? j + 1 : j)];
          visit(c0);
          if (two) visit(c1);
        }
      }
      double jr = 100.0, sr = 100.0, w = 0.0;
      int valid = 0;
      const Moments& own = q_is_src ? ms : mr;
      const Moments& other = q_is_src ? mr : ms;
      if (other.n >= 1) {                                                         // overlap_req_ = 1 (:138, :160)
        const Moments mj{ms.n + mr.n, ms.sx + mr.sx, ms.sy + mr.sy, ms.sxx + mr.sxx, ms.sxy + mr.sxy, ms.syy + mr.syy};
        double s00, s01, s11, j00, j01, j11;
        if (cov_from_moments(own, s00, s01, s11) && cov_from_moments(mj, j00, j01, j11)) {
          const double det_j = j00 * j11 - j01 * j01;                             // ComputeEntropy (:80-98)
          const double det_s = s00 * s11 - s01 * s01;
          if (!(isnan(det_s) || isnan(det_j))) {
            const double sep_entropy = 1.0 / 2.0 * log(2.0 * M_PI * exp(1.0) * det_s + 0.00000001);
            const double joint_entropy = 1.0 / 2.0 * log(2.0 * M_PI * exp(1.0) * det_j + 0.00000001);
            if (!(isnan(sep_entropy) || isnan(joint_entropy))) {
              w = cm.weight_res_intensity ? (double)q.z : 1.0;                    // :180
              jr = w * joint_entropy; sr = w * sep_entropy; valid = 1;
            }
          }
        }
      }
      gstore<double>(jres + idx, jr); gstore<double>(sres + idx, sr); gstore<double>(wres + idx, valid ? w : 0.0); gstore<int32_t>(vres + idx, valid);
    }
  };
  if (g.spt_in_lds) find_overlap((CFEAR_LDS const v4f*)g.spt);
  else find_overlap((const v4f*)g.spt);
  __threadfence_block();
  __syncthreads();
  const int W = *n_work;
  CORAL_T(4);
  if (g.spt_in_lds) sweep((CFEAR_LDS const v4f*)g.spt, W);
  else sweep((const v4f*)g.spt, W);
  __threadfence_block();
  __syncthreads();
  CORAL_T(5);
  // ---- 5. aggregation in index order (:178-204): contiguous chunk per thread, then a fixed tree ------
  {
    const int chunk = (n + kCoralThreads - 1) / kCoralThreads;
    double sj = 0.0, ss = 0.0, sw = 0.0;
    int cnt = 0;
    for (int i = tid * chunk; i < min(n, (tid + 1) * chunk); i++)
      if (gload<int32_t>(vres + i)) { sw += gload<double>(wres + i); sj += gload<double>(jres + i); ss += gload<double>(sres + i); cnt++; }
    sj = wave_sum_lane63_f64(sj); ss = wave_sum_lane63_f64(ss); sw = wave_sum_lane63_f64(sw);
    cnt = wave_sum_i32(cnt);
    if (lane == 63) { red_d[wave * 3] = sj; red_d[wave * 3 + 1] = ss; red_d[wave * 3 + 2] = sw; red_c[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
      double joint = 0.0, sep = 0.0, w_sum = 0.0;
      int count_valid = 0;
      for (int wv = 0; wv < 16; wv++) { joint += red_d[wv * 3]; sep += red_d[wv * 3 + 1]; w_sum += red_d[wv * 3 + 2]; count_valid += red_c[wv]; }
      if (count_valid > 0) { sep /= w_sum; joint /= w_sum; }
      const double overlap = count_valid / ((double)n);
      cfear_coral_result& r = cm.results[blockIdx.x];
      r.joint = joint; r.sep = sep; r.overlap = overlap;                        // quality_ = {joint_, sep_, overlap_}
      r.valid = overlap < 0.1 ? 0 : 1;                                          // :197-204
      r.count_valid = count_valid; r.status = CFEAR_OK; r.pad = g.path;
    }
  }
#ifdef CFEAR_CORAL_TIMING
  CORAL_T(6);
  if (tid == 0 && (blockIdx.x % 997) == 0)
    printf("coral job %d n %d W %d: bbox %lld | sort %lld | table %lld | overlap %lld | sweep %lld | reduce %lld | total %lld\n", blockIdx.x, n, *n_work,
           tq[1] - tq[0], tq[2] - tq[1], tq[3] - tq[2], tq[4] - tq[3], tq[5] - tq[4], tq[6] - tq[5], tq[6] - tq[0]);
#endif
  if (cm.per_point) {
    double* pp = cm.per_point + (size_t)blockIdx.x * cm.cap * 3;
    for (int i = tid; i < n; i += kCoralThreads) { pp[3 * i] = jres[i]; pp[3 * i + 1] = sres[i]; pp[3 * i + 2] = (double)vres[i]; }
  }
}

}  // namespace

int cfear_coral_max_points() { return kCoralMaxPoints; }

// The launch both entry points share: the kernel's constants, the per-job scratch (bounded to 1 GiB per launch, so a large
// batch takes several launches) and the LDS allowance.  d_per_point: nullable, [n_jobs][cap][3].
static int coral_launch(cfear_ctx* ctx, const CoralJob* d_jobs, int n_jobs, int cap, const cfear_coral_params* par,
                        cfear_coral_result* d_results, double* d_per_point) {
  CoralCommon cm;
  cm.radius = par->radius;
  cm.r2 = (float)(par->radius * par->radius);            // radiusSearch passes float(radius * radius) to FLANN
  cm.inv_cell = (float)(1.0 / (par->radius * 1.0001));   // cell a hair wider than the radius: float rounding of
                                                         // x * inv_cell can never put a neighbour two cells away
  cm.weight_res_intensity = par->weight_res_intensity;
  cm.cap = std::max(cap, 1);
  cm.scratch_stride = coral_scratch_bytes(cm.cap);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_jobs, ((size_t)1 << 30) / cm.scratch_stride));
  cm.scratch = (char*)cfear_workspace(ctx, kWsCoralScratch, cm.scratch_stride * (size_t)chunk);
  if (!cm.scratch) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)coral_kernel, kGridLdsTotal));
  {
    ProfScope ps(ctx, "coral_quality");
    for (int j0 = 0; j0 < n_jobs; j0 += chunk) {
      const int nj = std::min(chunk, n_jobs - j0);
      cm.results = d_results + j0;
      cm.per_point = d_per_point ? d_per_point + (size_t)j0 * cm.cap * 3 : nullptr;
      hipLaunchKernelGGL(coral_kernel, dim3(nj), dim3(kCoralThreads), kGridLdsTotal, ctx->stream, d_jobs + j0, cm);
    }
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

int cfear_coral_launch_device(cfear_ctx* ctx, const CoralJob* d_jobs, int n_jobs, int cap, const cfear_coral_params* par,
                              cfear_coral_result* d_results) {
  if (!(par->radius > 0.0)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "radius must be > 0");
  if (n_jobs <= 0) return CFEAR_OK;
  if (cap > kCoralMaxPoints) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "a job's %d points exceed %d", cap, kCoralMaxPoints);
  return coral_launch(ctx, d_jobs, n_jobs, cap, par, d_results, nullptr);
}

extern "C" void cfear_coral_params_default(cfear_coral_params* p) {
  if (!p) return;
  p->radius = 1.0;                    // alignmentinterface.cpp:444
  p->weight_res_intensity = 0;
  p->pad = 0;
}

// The batch in two halves, so that a caller with host work of its own (verify.hip) can do it while the kernel runs:
// cfear_coral_enqueue stages the clouds, uploads the jobs and launches; cfear_coral_collect reads the results back and
// synchronises.  `pend` carries what must outlive the launch; its stage drains the stream if collect() does not complete.
int cfear_coral_enqueue(cfear_ctx* ctx, const cfear_coral_job* jobs, int32_t n_jobs, const cfear_coral_params* par, bool want_per_point,
                        CoralPending& pend) {
  pend.n_jobs = 0;
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !par || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (!(par->radius > 0.0)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "radius must be > 0");
  if (n_jobs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage& st = pend.stage;                            // host clouds staged once each (perturbation sets and candidate lists share clouds)
  int cap = 1;
  for (int j = 0; j < n_jobs; j++) {
    const cfear_coral_job& jb = jobs[j];
    if (jb.n_ref < 0 || jb.n_src < 0 || (jb.n_ref > 0 && !jb.ref_xyzi) || (jb.n_src > 0 && !jb.src_xyzi))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "job %d: null cloud", j);   // empty clouds are a per-job status
    if ((long long)jb.n_ref + jb.n_src > kCoralMaxPoints)
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "job %d: %d + %d points exceed %d", j, jb.n_ref, jb.n_src, kCoralMaxPoints);
    cap = std::max(cap, jb.n_ref + jb.n_src);
    st.cloud_in(jb.ref_xyzi, jb.n_ref);
    st.cloud_in(jb.src_xyzi, jb.n_src);
  }
  const size_t jb_bytes = (size_t)n_jobs * sizeof(CoralJob);
  CoralJob* d_jobs;
  cfear_coral_result* d_res;
  double* d_pp = nullptr;
  st.piece(d_jobs, jb_bytes);
  st.piece(d_res, (size_t)n_jobs * sizeof(cfear_coral_result));
  if (want_per_point) st.piece(d_pp, (size_t)n_jobs * cap * 3 * sizeof(double));
  CFEAR_CHECK(st.carve());
  CoralJob* hj = (CoralJob*)st.record(jb_bytes);
  for (int j = 0; j < n_jobs; j++) {
    const cfear_coral_job& jb = jobs[j];
    CoralJob& o = hj[j];
    o.ref = st.cloud(jb.ref_xyzi);
    o.src = st.cloud(jb.src_xyzi);
    o.n_ref_ptr = o.n_src_ptr = nullptr;
    o.n_ref = jb.n_ref; o.n_src = jb.n_src;
    for (int k = 0; k < 3; k++) { o.ref_pose[k] = jb.ref_pose[k]; o.src_pose[k] = jb.src_pose[k]; o.offset[k] = jb.offset[k]; }
  }
  CFEAR_CHECK(st.upload(d_jobs, hj, jb_bytes));
  CFEAR_CHECK(coral_launch(ctx, d_jobs, n_jobs, cap, par, d_res, d_pp));
  pend.n_jobs = n_jobs; pend.cap = cap; pend.d_res = d_res; pend.d_pp = d_pp;
  return CFEAR_OK;
}

int cfear_coral_collect(cfear_ctx* ctx, const cfear_coral_job* jobs, CoralPending& pend, cfear_coral_result* results, double* per_point) {
  const int n_jobs = pend.n_jobs, cap = pend.cap;
  if (n_jobs == 0) return CFEAR_OK;
  pend.stage.back(results, pend.d_res, (size_t)n_jobs * sizeof(cfear_coral_result));
  std::vector<double> hpp;
  if (per_point) {
    hpp.resize((size_t)n_jobs * cap * 3);
    pend.stage.back(hpp.data(), pend.d_pp, hpp.size() * sizeof(double));
  }
  CFEAR_CHECK(pend.stage.finish());                    // (drains on failure: hpp outlives every copy into it)
  if (per_point) {                                       // compact [job][n_src + n_ref][3]
    size_t o = 0;
    for (int j = 0; j < n_jobs; j++) {
      const size_t nn = (size_t)jobs[j].n_ref + jobs[j].n_src;
      std::copy(hpp.begin() + (size_t)j * cap * 3, hpp.begin() + (size_t)j * cap * 3 + nn * 3, per_point + o);
      o += nn * 3;
    }
  }
  for (int j = 0; j < n_jobs; j++)
    if (results[j].status != CFEAR_OK && results[j].status != CFEAR_ERR_EMPTY_CLOUD)
      return cfear_set_error(ctx, results[j].status, "job %d: %s", j, cfear_status_string(results[j].status));
  return CFEAR_OK;
}

extern "C" int cfear_coral_quality_batch(cfear_ctx* ctx, const cfear_coral_job* jobs, int32_t n_jobs,
                                         const cfear_coral_params* par, cfear_coral_result* results, double* per_point) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!results) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CoralPending pend(ctx);
  const int rc = cfear_coral_enqueue(ctx, jobs, n_jobs, par, per_point != nullptr, pend);
  if (rc != CFEAR_OK) return rc;
  return cfear_coral_collect(ctx, jobs, pend, results, per_point);
}

extern "C" int cfear_coral_quality(cfear_ctx* ctx, const cfear_coral_job* job, const cfear_coral_params* par,
                                   cfear_coral_result* result, double* per_point) {
  return cfear_coral_quality_batch(ctx, job, 1, par, result, per_point);
}
