// loopeval.hip -- scoring the loop detector (gfx950, wave64, fp64 and integers).
//
// cfear_loop_stats_batch restates PoseGraph::UpdateStatistics (tbv_slam/src/tbv_slam/posegraph.cpp:332-371) and
// EvaluationManager::getCandidateLoopStatus (place_recognition_radar/src/place_recognition_radar/EvaluationManager.cpp:
// 12-27) for every candidate of a batch of graphs.  The reference walks all earlier nodes once per candidate on the host;
// loop_stats_kernel gives a candidate one wavefront: the lanes stride the earlier nodes, each keeps its own nearest (the
// strict `<` over ascending k keeps the lowest k), and a butterfly over the pair (distance, index) -- the lower index
// winning equal distances -- leaves the reference's answer in every lane.  Lane 0 does the pose arithmetic and writes.
//
// cfear_loop_curves_batch restates what the reference's scripts ask of sklearn (metrics.roc_curve, metrics.auc,
// precision_recall_curve, ComputeClassifierStatistics) for a batch of experiments, one workgroup each (loop_curves_kernel):
//   1. counts: labels, NaN scores, the confusion matrix at p_threshold -- and the experiment's own refusal;
//   2. an order-preserving 64-bit key per score (ascending key = descending score, -0.0 read as 0.0) and the label in a
//      byte beside it, sorted by a bitonic network: in LDS up to CFEAR_LOOPEVAL_LDS_ROWS rows; beyond, in global memory,
//      every stage whose partner distance is below a chunk of that many rows running on the chunk in LDS;
//   3. block scans of the labels and of the run ends compact (tps, index) per distinct score into global scratch;
//   4. a second scan keeps the ROC points (drop_intermediate), the PR points are written reversed, then the trapezoid sum.
// Everything is an integer until the final divisions, and every sum has a fixed order, so an experiment's arrays and record
// depend on its rows alone.  tests/loopeval_cpu.py restates both calls in NumPy.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kStatsThreads = 256, kStatsWaves = kStatsThreads / CFEAR_WAVE;
constexpr int kCurveThreads = 1024, kCurveWaves = kCurveThreads / CFEAR_WAVE;
constexpr int kLdsRows = CFEAR_LOOPEVAL_LDS_ROWS;
constexpr size_t kCurveLds = (size_t)kLdsRows * 9;                 // keys, then labels
constexpr int64_t kCurveMaxRows = (int64_t)1 << 30;
static_assert((kLdsRows & (kLdsRows - 1)) == 0 && kLdsRows >= 2 * kCurveThreads, "a chunk is a power of two and a pair per thread at least");
static_assert(kCurveLds + 4096 <= 160 * 1024, "keys and labels of a chunk, and the scan scratch, fit the LDS of a workgroup");

__host__ __device__ inline bool fin(double v) { return v - v == 0.0; }
__host__ __device__ inline bool fin3(const double* p) { return fin(p[0]) && fin(p[1]) && fin(p[2]); }

// ---- loop rows ---------------------------------------------------------------------------------------------------------------
// 0 = fine; the codes index kCandFault
__host__ __device__ inline int loop_cand_fault(const cfear_loop_candidate& c, const int64_t* off, int32_t n_graphs, const double* gt) {
  if (c.graph < 0 || c.graph >= n_graphs) return 1;
  const int64_t n0 = off[c.graph], n = off[c.graph + 1] - n0;
  if (c.from < 0 || c.from >= n || c.to < 0 || c.to >= n) return 2;
  if (c.guess_nr < 0) return 3;
  if (!fin3(c.guess_xyt)) return 4;
  if (!fin3(gt + 3 * (n0 + c.from)) || !fin3(gt + 3 * (n0 + c.to))) return 5;
  return 0;
}
const char* const kCandFault[] = {"", "its graph does not exist", "from or to lies outside its graph", "guess_nr is negative",
                                  "its guess is not finite", "the pose of from or to is not finite"};

struct StatsArgs {
  const int64_t* offsets;
  const double* gt;
  const uint8_t* has;
  const cfear_loop_candidate* cands;
  cfear_loop_row* rows;
  unsigned long long* flags;          // [0] lowest faulty node, [1] lowest faulty candidate (device buffers only)
  int64_t n_nodes, n_cand;
  int32_t n_graphs;
  cfear_loop_stats_params par;
};

__global__ __launch_bounds__(kStatsThreads) void loop_stats_check_kernel(const StatsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x;
  if (i < a.n_nodes && a.has[i] && !fin3(a.gt + 3 * i)) atomicMin(a.flags, (unsigned long long)i);
  if (i < a.n_cand && loop_cand_fault(a.cands[i], a.offsets, a.n_graphs, a.gt)) atomicMin(a.flags + 1, (unsigned long long)i);
}

__global__ __launch_bounds__(kStatsThreads) void loop_stats_kernel(const StatsArgs a) {
  const int lane = threadIdx.x & (CFEAR_WAVE - 1);
  const int64_t ci = (int64_t)blockIdx.x * kStatsWaves + threadIdx.x / CFEAR_WAVE;
  if (ci >= a.n_cand) return;                                   // the whole wavefront
  const cfear_loop_candidate c = a.cands[ci];
  const int64_t n0 = a.offsets[c.graph];
  const double* gt = a.gt + 3 * n0;
  const uint8_t* has = a.has + n0;
  const double fx = gt[3 * (size_t)c.from], fy = gt[3 * (size_t)c.from + 1];
  double best = a.par.no_loop_distance;
  int idx = c.from;
  const bool from_gt = has[c.from] != 0;
  if (from_gt) {
    const int64_t lim = (int64_t)c.from - a.par.min_index_gap;  // from - k > gap
    for (int64_t k = lane; k < lim; k += CFEAR_WAVE) {
      if (!has[k]) continue;
      const double dx = fx - gt[3 * k], dy = fy - gt[3 * k + 1];
      const double d = sqrt((dx * dx + dy * dy) + 0.0);
      if (d < best) { best = d; idx = (int)k; }
    }
    for (int m = 1; m < CFEAR_WAVE; m <<= 1) {
      const double od = __shfl_xor(best, m);
      const int oi = __shfl_xor(idx, m);
      if (od < best || (od == best && oi < idx)) { best = od; idx = oi; }
    }
  }
  if (lane != 0) return;
  const double ft = gt[3 * (size_t)c.from + 2];
  const double tx = gt[3 * (size_t)c.to], ty = gt[3 * (size_t)c.to + 1], tt = gt[3 * (size_t)c.to + 2];
  const double dx = tx - fx, dy = ty - fy;
  const double cf = cos(ft), sf = sin(ft), ct = cos(tt), st = sin(tt), cg = cos(c.guess_xyt[2]), sg = sin(c.guess_xyt[2]);
  const double cgd = cf * ct + sf * st, sgd = cf * st - sf * ct;
  const double xgd = cf * dx + sf * dy, ygd = cf * dy - sf * dx;
  const double cd = cg * cgd + sg * sgd, sd = cg * sgd - sg * cgd;
  const double ex = xgd - c.guess_xyt[0], ey = ygd - c.guess_xyt[1];
  cfear_loop_row r;
  r.diff[0] = cg * ex + sg * ey;
  r.diff[1] = cg * ey - sg * ex;
  r.diff[2] = atan2(sd, cd);
  r.closest_loop_distance = best;
  r.candidate_loop_distance = from_gt && has[c.to] ? sqrt((dx * dx + dy * dy) + 0.0) : -1.0;
  r.transl_error = sqrt(r.diff[0] * r.diff[0] + r.diff[1] * r.diff[1]);
  r.rot_error = 180.0 / M_PI * fabs(r.diff[2]);
  r.close_xy[0] = gt[3 * (size_t)idx];
  r.close_xy[1] = gt[3 * (size_t)idx + 1];
  r.id_close = idx;
  r.is_loop = best < a.par.max_distance;
  r.candidate_close = r.transl_error < a.par.max_registration_translation && r.rot_error < a.par.max_registration_rotation_deg;
  r.prediction_pos_ok = !r.is_loop || r.candidate_close;
  a.rows[ci] = r;
}

// ---- curves --------------------------------------------------------------------------------------------------------------------
struct CurveJob {
  int64_t row0;             // the experiment's first row
  int64_t out0;             // its first entry in the six curve arrays
  int64_t pad0;             // global route: its first element in the padded key and label scratch
  int32_t n, npad;          // rows; the power of two the sort runs over
  int32_t exp, pad;
};
static_assert(sizeof(CurveJob) == 40, "job table record");

struct CurveArgs {
  const CurveJob* jobs;
  const uint8_t* y;
  const double* score;
  const uint8_t* pos_ok;
  double *roc_fpr, *roc_tpr, *roc_thr, *pr_precision, *pr_recall, *pr_thr;
  cfear_loop_curves_result* res;
  unsigned long long* gkeys;
  uint8_t* glabs;
  int32_t *ctps, *cidx;     // per distinct score, at the experiment's row0: tps and the run's last sorted position
  cfear_loop_curves_params par;
};

// ascending key = descending score
__device__ __forceinline__ unsigned long long score_key(double s) {
  s = s == 0.0 ? 0.0 : s;
  const unsigned long long u = (unsigned long long)__double_as_longlong(s);
  return ~((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}
__device__ __forceinline__ double key_score(unsigned long long k) {
  const unsigned long long o = ~k;
  return __longlong_as_double((long long)((o >> 63) ? (o & 0x7fffffffffffffffull) : ~o));
}

struct CurveShared {
  int wsum[2 * kCurveWaves];
  double dsum[kCurveWaves];
};

// the workgroup's total, in every thread; ends with a barrier
__device__ int block_sum_i32(int v, int* sh) {
  const int s = wave_sum_i32(v);
  if ((threadIdx.x & (CFEAR_WAVE - 1)) == 0) sh[threadIdx.x / CFEAR_WAVE] = s;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < kCurveWaves; w++) t += sh[w];
  __syncthreads();
  return t;
}
// inclusive scans of a and b over the workgroup (in place) and their totals; ends with a barrier
__device__ void block_scan2(int& a, int& b, int& tot_a, int& tot_b, int* sh) {
  const int lane = threadIdx.x & (CFEAR_WAVE - 1), wave = threadIdx.x / CFEAR_WAVE;
  a = wave_incl_scan_i32(a);
  b = wave_incl_scan_i32(b);
  if (lane == CFEAR_WAVE - 1) { sh[wave] = a; sh[kCurveWaves + wave] = b; }
  __syncthreads();
  int oa = 0, ob = 0, ta = 0, tb = 0;
  for (int w = 0; w < kCurveWaves; w++) {
    const int xa = sh[w], xb = sh[kCurveWaves + w];
    if (w < wave) { oa += xa; ob += xb; }
    ta += xa; tb += xb;
  }
  a += oa; b += ob; tot_a = ta; tot_b = tb;
  __syncthreads();
}

// the compare-exchange stages j = j0, j0 / 2, ..., 1 of the merges of size k over cnt elements whose first has index g0
// in the whole network; each stage ends with a barrier
__device__ void bitonic_stages(unsigned long long* ks, uint8_t* ls, int cnt, int64_t g0, int64_t k, int j0) {
  for (int j = j0; j > 0; j >>= 1) {
    for (int t = threadIdx.x; t < cnt / 2; t += kCurveThreads) {
      const int i = 2 * t - (t & (j - 1)), p = i + j;
      const bool up = ((g0 + i) & k) == 0;
      const unsigned long long x = ks[i], z = ks[p];
      if ((x > z) == up) {
        ks[i] = z; ks[p] = x;
        const uint8_t lx = ls[i];
        ls[i] = ls[p]; ls[p] = lx;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kCurveThreads) void loop_curves_kernel(const CurveArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ CurveShared sh;
  unsigned long long* lkeys = (unsigned long long*)lds;
  uint8_t* llabs = lds + (size_t)kLdsRows * 8;
  const CurveJob job = a.jobs[blockIdx.x];
  const int tid = threadIdx.x, n = job.n;
  const uint8_t* y = a.y + job.row0;
  const double* score = a.score + job.row0;
  const uint8_t* pos_ok = a.pos_ok ? a.pos_ok + job.row0 : nullptr;
  cfear_loop_curves_result* out = a.res + job.exp;

  // ---- 1. counts and the experiment's own refusal ------------------------------------------------------------------------------
  int c_bad = 0, c_pos = 0, c_tn = 0, c_fp = 0, c_fn = 0, c_tp = 0;
  for (int i = tid; i < n; i += kCurveThreads) {
    const int yi = y[i];
    const double s = score[i];
    c_bad += yi > 1 || s != s;
    c_pos += yi == 1;
    const bool pred = s >= a.par.p_threshold;
    const bool yc = yi == 1 && !(pred && pos_ok && !pos_ok[i]);
    c_tn += !yc && !pred; c_fp += !yc && pred; c_fn += yc && !pred; c_tp += yc && pred;
  }
  c_bad = block_sum_i32(c_bad, sh.wsum);
  c_pos = block_sum_i32(c_pos, sh.wsum);
  if (n == 0 || c_bad || c_pos == 0 || c_pos == n) {
    if (tid == 0) {
      cfear_loop_curves_result r{};
      r.status = CFEAR_ERR_INVALID_ARGUMENT;
      *out = r;
    }
    return;
  }
  c_tn = block_sum_i32(c_tn, sh.wsum); c_fp = block_sum_i32(c_fp, sh.wsum);
  c_fn = block_sum_i32(c_fn, sh.wsum); c_tp = block_sum_i32(c_tp, sh.wsum);

  // ---- 2. keys and labels, sorted -------------------------------------------------------------------------------------------------
  const int npad = job.npad;
  const bool in_lds = npad <= kLdsRows;
  unsigned long long* ks = in_lds ? lkeys : a.gkeys + job.pad0;
  uint8_t* ls = in_lds ? llabs : a.glabs + job.pad0;
  for (int i = tid; i < npad; i += kCurveThreads) {
    ks[i] = i < n ? score_key(score[i]) : ~0ull;                // no score has this key: it would be a NaN
    ls[i] = i < n ? y[i] : 0;
  }
  __syncthreads();
  if (in_lds) {
    for (int k = 2; k <= npad; k <<= 1) bitonic_stages(ks, ls, npad, 0, k, k / 2);
  } else {
    for (int64_t k = 2; k <= npad; k <<= 1) {
      for (int64_t j = k / 2; j >= kLdsRows; j >>= 1) {
        for (int t = tid; t < npad / 2; t += kCurveThreads) {
          const int i = 2 * t - (t & ((int)j - 1)), p = i + (int)j;
          const bool up = (i & k) == 0;
          const unsigned long long x = ks[i], z = ks[p];
          if ((x > z) == up) {
            ks[i] = z; ks[p] = x;
            const uint8_t lx = ls[i];
            ls[i] = ls[p]; ls[p] = lx;
          }
        }
        __syncthreads();
      }
      // the stages below a chunk, chunk by chunk in LDS; for k <= kLdsRows these are whole merges, run once at k = kLdsRows
      if (k < kLdsRows) continue;
      for (int g0 = 0; g0 < npad; g0 += kLdsRows) {
        for (int i = tid; i < kLdsRows; i += kCurveThreads) { lkeys[i] = ks[g0 + i]; llabs[i] = ls[g0 + i]; }
        __syncthreads();
        if (k == kLdsRows) for (int kk = 2; kk < kLdsRows; kk <<= 1) bitonic_stages(lkeys, llabs, kLdsRows, g0, kk, kk / 2);
        bitonic_stages(lkeys, llabs, kLdsRows, g0, k, kLdsRows / 2);
        for (int i = tid; i < kLdsRows; i += kCurveThreads) { ks[g0 + i] = lkeys[i]; ls[g0 + i] = llabs[i]; }
        __syncthreads();
      }
    }
  }

  // ---- 3. tps and the last position of every run of equal scores ---------------------------------------------------------------
  int32_t* ctps = a.ctps + job.row0;
  int32_t* cidx = a.cidx + job.row0;
  int carry_l = 0, carry_b = 0;
  for (int base = 0; base < n; base += kCurveThreads) {
    const int i = base + tid;
    const bool in = i < n;
    const bool bnd = in && (i == n - 1 || ks[i] != ks[i + 1]);
    int il = in ? ls[i] : 0, ib = bnd, tl, tb;
    block_scan2(il, ib, tl, tb, sh.wsum);
    if (bnd) { ctps[carry_b + ib - 1] = carry_l + il; cidx[carry_b + ib - 1] = i; }
    carry_l += tl; carry_b += tb;
  }
  __syncthreads();
  const int n_thr = carry_b;
  const double P = (double)c_pos, N = (double)(n - c_pos);

  // ---- 4. the curves --------------------------------------------------------------------------------------------------------------
  double* fpr = a.roc_fpr + job.out0;
  double* tpr = a.roc_tpr + job.out0;
  double* rthr = a.roc_thr + job.out0;
  double* prec = a.pr_precision + job.out0;
  double* rec = a.pr_recall + job.out0;
  double* pthr = a.pr_thr + job.out0;
  const bool drop = a.par.drop_intermediate && n_thr > 2;
  int kept = 0;
  for (int base = 0; base < n_thr; base += kCurveThreads) {
    const int m = base + tid;
    const bool in = m < n_thr;
    long long t1 = 0, f1 = 0;
    double thr = 0.0;
    bool keep = in;
    if (in) {
      const int i1 = cidx[m];
      t1 = ctps[m]; f1 = 1 + (long long)i1 - t1;
      thr = key_score(ks[i1]);
      if (drop && m > 0 && m < n_thr - 1) {
        const long long t0 = ctps[m - 1], t2 = ctps[m + 1];
        const long long f0 = 1 + (long long)cidx[m - 1] - t0, f2 = 1 + (long long)cidx[m + 1] - t2;
        keep = (t2 - 2 * t1 + t0) != 0 || (f2 - 2 * f1 + f0) != 0;
      }
      const int j = n_thr - 1 - m;                               // the PR arrays run from the lowest threshold up
      prec[j] = (double)t1 / (double)(t1 + f1);                  // t1 + f1 = 1 + i1 > 0: sklearn's 0 / 0 case cannot occur
      rec[j] = (double)t1 / P;
      pthr[j] = thr;
    }
    int ik = keep, unused = 0, tk, tu;
    block_scan2(ik, unused, tk, tu, sh.wsum);
    if (keep) {
      const int r = kept + ik;                                   // entry 0 is the point (0, 0, +inf)
      fpr[r] = (double)f1 / N;
      tpr[r] = (double)t1 / P;
      rthr[r] = thr;
    }
    kept += tk;
  }
  const int n_roc = kept + 1, n_pr = n_thr + 1;
  if (tid == 0) {
    fpr[0] = 0.0; tpr[0] = 0.0; rthr[0] = INFINITY;
    prec[n_thr] = 1.0; rec[n_thr] = 0.0;
  }
  __syncthreads();
  if (a.par.reference_endpoints && tid == 0) {
    tpr[n_roc - 1] = tpr[n_roc - 2];
    rec[0] = rec[1];
    prec[0] = prec[1];
  }
  __syncthreads();
  double acc = 0.0;
  for (int i = tid; i < n_roc - 1; i += kCurveThreads) acc += (fpr[i + 1] - fpr[i]) * (tpr[i + 1] + tpr[i]) / 2.0;
  acc = wave_sum_f64(acc);
  if ((tid & (CFEAR_WAVE - 1)) == 0) sh.dsum[tid / CFEAR_WAVE] = acc;
  __syncthreads();
  if (tid == 0) {
    double auc = sh.dsum[0];
    for (int w = 1; w < kCurveWaves; w++) auc += sh.dsum[w];
    cfear_loop_curves_result r{};
    r.auc = auc;
    r.accuracy = (double)(c_tn + c_tp) / (double)n;
    r.precision = c_tp + c_fp ? (double)c_tp / (double)(c_tp + c_fp) : 0.0;
    r.recall = c_tp + c_fn ? (double)c_tp / (double)(c_tp + c_fn) : 0.0;
    r.n_pos = c_pos; r.n_neg = n - c_pos;
    r.confusion[0] = c_tn; r.confusion[1] = c_fp; r.confusion[2] = c_fn; r.confusion[3] = c_tp;
    r.n_thresholds = n_thr; r.n_roc = n_roc; r.n_pr = n_pr;
    r.status = CFEAR_OK;
    *out = r;
  }
}

int next_pow2(int64_t n) {
  int p = CFEAR_WAVE * 2;                                        // a pair per lane of a wavefront at least
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

extern "C" void cfear_loop_stats_params_default(cfear_loop_stats_params* p) {
  if (!p) return;
  p->max_distance = 6.0;                        // EvaluationManager.cpp:14-16
  p->max_registration_translation = 4.0;
  p->max_registration_rotation_deg = 2.5;
  p->no_loop_distance = 100000.0;               // posegraph.cpp:334
  p->min_index_gap = 10;                        // posegraph.cpp:358
  p->pad = 0;
}

extern "C" int cfear_loop_stats_batch(cfear_ctx* ctx, const int64_t* node_offsets, const double* gt_xyt, const uint8_t* has_gt, int64_t n_nodes,
                                      int32_t n_graphs, const cfear_loop_candidate* candidates, int64_t n_cand, const cfear_loop_stats_params* par,
                                      cfear_loop_row* rows, int64_t* failed_candidate) {
  if (failed_candidate) *failed_candidate = -1;
  // ---- everything that can be checked on the host is, before a context is needed and before anything is written ---------
  if (n_graphs < 0 || n_nodes < 0 || n_cand < 0 || !par || !node_offsets)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null or negative argument (node_offsets holds n_graphs + 1 entries)");
  if ((n_nodes > 0 && (!gt_xyt || !has_gt)) || (n_cand > 0 && (!candidates || !rows)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (std::isnan(par->max_distance) || std::isnan(par->max_registration_translation) || std::isnan(par->max_registration_rotation_deg) ||
      std::isnan(par->no_loop_distance) || par->min_index_gap < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "a parameter is NaN, or min_index_gap is negative");
  if (cfear_is_device_ptr(node_offsets)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node_offsets must be host memory");
  const int kind = memory_kind({gt_xyt, has_gt, candidates, rows});
  if (kind < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "gt_xyt, has_gt, candidates and rows must be all host or all device memory");
  const int bad_graph = (int)check_offsets(node_offsets, n_graphs, n_nodes).first_fault();
  if (bad_graph != -2)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: node_offsets must run from 0 to n_nodes over n_graphs + 1 entries without descending", bad_graph);
  for (int32_t g = 0; g < n_graphs; g++)
    if (node_offsets[g + 1] - node_offsets[g] > INT32_MAX)
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "graph %d: more than 2^31 - 1 nodes", g);
  if ((n_cand + kStatsWaves - 1) / kStatsWaves > INT32_MAX || (n_nodes + kStatsThreads - 1) / kStatsThreads > INT32_MAX)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more candidates or nodes than one launch addresses");
  if (kind == 0) {
    for (int64_t i = 0; i < n_nodes; i++)
      if (has_gt[i] && !fin3(gt_xyt + 3 * i))
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node %lld (flat index) has ground truth that is not finite", (long long)i);
    for (int64_t i = 0; i < n_cand; i++) {
      const int f = loop_cand_fault(candidates[i], node_offsets, n_graphs, gt_xyt);
      if (f) {
        if (failed_candidate) *failed_candidate = i;
        return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %lld: %s", (long long)i, kCandFault[f]);
      }
    }
  }
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n_cand == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsLoopEval);
  StatsArgs a{};
  st.in(a.offsets, node_offsets, (size_t)(n_graphs + 1) * 8);
  st.in(a.gt, gt_xyt, (size_t)n_nodes * 24);
  st.in(a.has, has_gt, (size_t)n_nodes);
  st.in(a.cands, candidates, (size_t)n_cand * sizeof(cfear_loop_candidate));
  st.out(a.rows, rows, (size_t)n_cand * sizeof(cfear_loop_row));
  st.piece(a.flags, 16);
  CFEAR_CHECK(st.carve());
  a.n_nodes = n_nodes; a.n_cand = n_cand; a.n_graphs = n_graphs; a.par = *par;
  if (kind == 1) {
    unsigned long long* h = (unsigned long long*)st.record(16);
    h[0] = h[1] = ~0ull;
    CFEAR_CHECK(st.upload(a.flags, h, 16));
    const int64_t n_check = std::max(n_nodes, n_cand);
    {
      ProfScope ps(ctx, "loop_stats_check");
      hipLaunchKernelGGL(loop_stats_check_kernel, dim3((unsigned)((n_check + kStatsThreads - 1) / kStatsThreads)), dim3(kStatsThreads), 0,
                         ctx->stream, a);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    unsigned long long got[2];
    st.fetch(got, a.flags, 16);
    CFEAR_CHECK(st.wait());
    if (got[0] != ~0ull)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node %lld (flat index) has ground truth that is not finite", (long long)got[0]);
    if (got[1] != ~0ull) {
      if (failed_candidate) *failed_candidate = (int64_t)got[1];
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "candidate %lld: its graph, from, to, guess_nr, guess or poses are not usable", (long long)got[1]);
    }
  }
  {
    ProfScope ps(ctx, "loop_stats");
    hipLaunchKernelGGL(loop_stats_kernel, dim3((unsigned)((n_cand + kStatsWaves - 1) / kStatsWaves)), dim3(kStatsThreads), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}

extern "C" void cfear_loop_curves_params_default(cfear_loop_curves_params* p) {
  if (!p) return;
  p->p_threshold = 0.9;                         // LoopClosureEval.py:88
  p->drop_intermediate = 1;                     // sklearn.metrics.roc_curve's default
  p->reference_endpoints = 1;                   // 3_loop_closure.py:157,164-165
}

extern "C" int cfear_loop_curves_batch(cfear_ctx* ctx, const int64_t* row_offsets, const uint8_t* y, const double* score, const uint8_t* pos_ok,
                                       int64_t n_rows, int32_t n_exp, const cfear_loop_curves_params* par, double* roc_fpr, double* roc_tpr,
                                       double* roc_thr, double* pr_precision, double* pr_recall, double* pr_thr,
                                       cfear_loop_curves_result* results, int32_t* failed_experiment) {
  if (failed_experiment) *failed_experiment = -1;
  if (n_exp < 0 || n_rows < 0 || !par || !row_offsets)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null or negative argument (row_offsets holds n_exp + 1 entries)");
  if (n_exp > 0 && (!roc_fpr || !roc_tpr || !roc_thr || !pr_precision || !pr_recall || !pr_thr || !results))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null output");
  if (n_rows > 0 && (!y || !score)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "y or score is null");
  if (std::isnan(par->p_threshold)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "p_threshold is NaN");
  if (cfear_is_device_ptr(row_offsets) || cfear_is_device_ptr(results))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "row_offsets and results must be host memory");
  if (memory_kind({y, score, pos_ok, roc_fpr, roc_tpr, roc_thr, pr_precision, pr_recall, pr_thr}) < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "y, score, pos_ok and the six curve arrays must be all host or all device memory");
  const int bad_exp = (int)check_offsets(row_offsets, n_exp, n_rows).first_fault();
  if (bad_exp != -2) {
    if (failed_experiment) *failed_experiment = bad_exp;
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "experiment %d: row_offsets must run from 0 to n_rows over n_exp + 1 entries without descending", bad_exp);
  }
  for (int32_t e = 0; e < n_exp; e++)
    if (row_offsets[e + 1] - row_offsets[e] > kCurveMaxRows) {
      if (failed_experiment) *failed_experiment = e;
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "experiment %d: more than 2^30 rows", e);
    }
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n_exp == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // ---- the job table: the experiments that sort in LDS first, then those that sort in global memory --------------------------
  std::vector<CurveJob> jobs;
  jobs.reserve(n_exp);
  int64_t pad_total = 0;
  int n_lds = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int32_t e = 0; e < n_exp; e++) {
      const int64_t n = row_offsets[e + 1] - row_offsets[e];
      if ((n > kLdsRows) != (pass == 1)) continue;
      CurveJob j{};
      j.row0 = row_offsets[e]; j.out0 = row_offsets[e] + e; j.n = (int32_t)n; j.npad = next_pow2(n); j.exp = e;
      if (pass == 1) { j.pad0 = pad_total; pad_total += j.npad; }
      else n_lds++;
      jobs.push_back(j);
    }
  HostStage st(ctx, kWsLoopEval);
  CurveArgs a{};
  const size_t curve_bytes = (size_t)(n_rows + n_exp) * 8, tab_bytes = jobs.size() * sizeof(CurveJob);
  char* d_tab;
  st.in(a.y, y, (size_t)n_rows);
  st.in(a.score, score, (size_t)n_rows * 8);
  st.in(a.pos_ok, pos_ok, (size_t)n_rows);
  // host arrays go up as well as down: the entries the call does not write keep what the caller had there
  st.in(a.roc_fpr, roc_fpr, curve_bytes, true);
  st.in(a.roc_tpr, roc_tpr, curve_bytes, true);
  st.in(a.roc_thr, roc_thr, curve_bytes, true);
  st.in(a.pr_precision, pr_precision, curve_bytes, true);
  st.in(a.pr_recall, pr_recall, curve_bytes, true);
  st.in(a.pr_thr, pr_thr, curve_bytes, true);
  st.out(a.res, results, (size_t)n_exp * sizeof(cfear_loop_curves_result));
  st.piece(d_tab, tab_bytes);
  st.piece(a.gkeys, (size_t)pad_total * 8);
  st.piece(a.glabs, (size_t)pad_total);
  st.piece(a.ctps, (size_t)n_rows * 4);
  st.piece(a.cidx, (size_t)n_rows * 4);
  CFEAR_CHECK(st.carve());
  void* h = st.record(tab_bytes);
  memcpy(h, jobs.data(), tab_bytes);
  CFEAR_CHECK(st.upload(d_tab, h, tab_bytes));
  a.par = *par;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)loop_curves_kernel, kCurveLds));
  if (n_lds) {
    a.jobs = (const CurveJob*)d_tab;
    ProfScope ps(ctx, "loop_curves_lds");
    hipLaunchKernelGGL(loop_curves_kernel, dim3(n_lds), dim3(kCurveThreads), kCurveLds, ctx->stream, a);
  }
  if (n_exp - n_lds) {
    a.jobs = (const CurveJob*)d_tab + n_lds;
    ProfScope ps(ctx, "loop_curves_global");
    hipLaunchKernelGGL(loop_curves_kernel, dim3(n_exp - n_lds), dim3(kCurveThreads), kCurveLds, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}
