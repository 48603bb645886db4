// evaluate.hip -- the KITTI odometry metric for a batch of (estimate, ground truth) trajectory pairs: what the
// reference's run scripts end in, radar_kitti_benchmark/python/eval_odom.py --align 6dof, i.e. KittiEvalOdom.eval of
// radar_kitti_benchmark/python/kitti_odometry.py (cited below as :line).  DESIGN.md section 4.8.
//
// Everything is fp64.  The pose algebra (pose_rows.hpp) has ONE operation order, shared with tests/kitti_eval_cpu.py,
// because the segment ends are decided by comparing sums of rounded distances (:182-195).
// Reductions are a fixed tree (a thread's strided serial sum, the wave's DPP butterfly, the four waves in order), one
// workgroup per trajectory: a trajectory's figures do not depend on the batch it is evaluated in.  No atomics.
//
// Kernels (poses stay [pose][12], the 96-byte records a KITTI line holds: a segment reads four poses at unrelated frames):
//   eval_normalise    thread per pose (flat grid over the batch's poses)   inv(first pose) * pose for both trajectories (:708-714)
//   eval_align_sums   workgroup per pair    means and the 3 x 3 covariance of umeyama_alignment (:49-61); the SVD of the
//                                           covariance is host code (cfear_align_from_sums)
//   eval_apply_align  thread per pose       [r | t] * estimate (:730-737)
//   eval_distance     wavefront per pair    the serial sum dist[i+1] = dist[i] + |p_i - p_{i+1}| (:123-141): the segment
//                                           lengths are computed 64 at a time, the running sum is carried through readlane
//   eval_counts       thread per (pair, length)   how many start frames have a segment of that length
//   eval_segments     workgroup per pair    binary search of last_frame, the three products of :228-239, the row table,
//                                           the per-length and overall means (:264-287, :442-475)
//   eval_frames       workgroup per pair    ATE (:477-505) and RPE (:508-583)
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pose_rows.hpp"

namespace {
constexpr int kEvalThreads = kAlignThreads;
constexpr int kEvalLengths = CFEAR_EVAL_NUM_LENGTHS;
static_assert(sizeof(cfear_eval_params) == 72, "cfear_eval_params is 72 bytes (include/cfear_hip.h)");
static_assert(sizeof(cfear_eval_summary) == 360, "cfear_eval_summary is 360 bytes (include/cfear_hip.h)");
static_assert(sizeof(cfear_eval_row) == 48, "cfear_eval_row is 48 bytes (include/cfear_hip.h)");

struct EvalTraj {          // one pair: where its poses are in the caller's arrays and in the workspace
  int64_t src;             // first pose in est / gt
  int64_t off;             // first pose in the normalised copies and in dist
  int32_t n;               // poses
  int32_t starts;          // start frames: ceil(n / step_size)
};
struct EvalPost {          // what the host adds between the two halves of the call
  double align[12];        // [r | t] of the 6dof alignment (identity for `none`)
  int64_t row_base;        // first row of the pair in the row table
  int32_t status, pad;
};
struct EvalArgs {
  const EvalTraj* traj;
  const EvalPost* post;
  const int2* blocks;      // per-pose kernels: (pair, first pose of the pair) of every workgroup -- a flat grid over the poses
  double2* frame;          // [total]: (translation, rotation) error of frame i -> i + 1, kept for the deviation's second pass
  const double* est;       // caller's poses [..][12]
  const double* gt;
  double* E;               // normalised (then aligned) estimate, [total][12]
  double* G;               // normalised ground truth
  double* dist;            // [total]
  double* sums;            // [n_traj][16]: mean x (3), mean y (3), covariance (9, row-major y x^T)
  int32_t* counts;         // [n_traj][8]
  cfear_eval_summary* summaries;
  cfear_eval_row* rows;    // nullable
  int64_t row_cap;
  int32_t n_traj, step;
  double lengths[kEvalLengths];
};

__global__ __launch_bounds__(kEvalThreads) void eval_normalise_kernel(EvalArgs a) {
  const int2 blk = a.blocks[blockIdx.x];
  const EvalTraj tr = a.traj[blk.x];
  const int i = blk.y + threadIdx.x;
  if (i >= tr.n) return;
  const Pose e0 = pose_inv(pose_load(a.est + tr.src * 12)), g0 = pose_inv(pose_load(a.gt + tr.src * 12));
  pose_store(a.E + (tr.off + i) * 12, pose_mul(e0, pose_load(a.est + (tr.src + i) * 12)));
  pose_store(a.G + (tr.off + i) * 12, pose_mul(g0, pose_load(a.gt + (tr.src + i) * 12)));
}

// umeyama_alignment(x = estimate, y = ground truth), :49-61: the means, then 1/n sum (y_i - my)(x_i - mx)^T
struct EvalAlignSrc {
  static constexpr bool kSkips = false;
  const double *E, *G;
  int n;
  __device__ bool counts(int) const { return true; }
  __device__ double x(int i, int k) const { return E[(size_t)i * 12 + 4 * k + 3]; }
  __device__ double y(int i, int k) const { return G[(size_t)i * 12 + 4 * k + 3]; }
  __device__ double mean_div(double) const { return (double)n; }
  __device__ double cov(double sum) const { return sum / (double)n; }
};
__global__ __launch_bounds__(kEvalThreads) void eval_align_sums_kernel(EvalArgs a) {
  __shared__ double red[4];
  const EvalTraj tr = a.traj[blockIdx.x];
  align_sums(EvalAlignSrc{a.E + tr.off * 12, a.G + tr.off * 12, tr.n}, a.sums + (size_t)blockIdx.x * 16, red);
}

__global__ __launch_bounds__(kEvalThreads) void eval_apply_align_kernel(EvalArgs a) {
  const int2 blk = a.blocks[blockIdx.x];
  const EvalTraj tr = a.traj[blk.x];
  const int i = blk.y + threadIdx.x;
  if (i >= tr.n) return;
  const Pose T = pose_load(a.post[blk.x].align);
  double* p = a.E + (tr.off + i) * 12;
  pose_store(p, pose_mul(T, pose_load(p)));
}

// trajectory_distances, :123-141, over the (normalised) ground truth.  One wavefront per pair: lane k computes the length
// of segment base + k, then the 64 lengths are added to the running sum one after the other, in frame order -- the
// devkit's serial sum, rounding for rounding.  A scan would be faster and would change the sums.
__global__ __launch_bounds__(64) void eval_distance_kernel(EvalArgs a) {
  const EvalTraj tr = a.traj[blockIdx.x];
  const int lane = threadIdx.x;
  const double* G = a.G + tr.off * 12;
  double* dist = a.dist + tr.off;
  if (lane == 0) dist[0] = 0.0;
  double run = 0.0;
  for (int base = 0; base < tr.n - 1; base += 64) {
    const int i = base + lane;
    double d = 0.0;                                  // past the end: run + 0 = run (the lengths are never negative)
    if (i < tr.n - 1) {
      const double* p1 = G + (size_t)i * 12;
      const double* p2 = p1 + 12;
      d = norm3(p1[3] - p2[3], p1[7] - p2[7], p1[11] - p2[11]);
    }
    double mine = 0.0;
#pragma unroll
    for (int k = 0; k < 64; k++) {
      run = run + readlane_f64(d, k);
      if (lane == k) mine = run;
    }
    if (i < tr.n - 1) dist[i + 1] = mine;
  }
}

// Start frame s * step has a segment of length L iff some dist[i] > dist[first] + L (:182-195, strict), i.e. iff the last
// one is: dist never decreases.  The threshold never decreases with s either, so those starts are a prefix [0, count).
__device__ __forceinline__ bool has_segment(const double* dist, int n, int first, double L) { return dist[n - 1] > dist[first] + L; }

__global__ __launch_bounds__(kEvalThreads) void eval_counts_kernel(EvalArgs a) {
  const int item = blockIdx.x * kEvalThreads + threadIdx.x;
  if (item >= a.n_traj * kEvalLengths) return;
  const int t = item / kEvalLengths, l = item % kEvalLengths;
  const EvalTraj tr = a.traj[t];
  const double* dist = a.dist + tr.off;
  int lo = 0, hi = tr.starts;                        // first start without a segment
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (has_segment(dist, tr.n, mid * a.step, a.lengths[l])) lo = mid + 1; else hi = mid;
  }
  a.counts[item] = lo;
}

// calc_sequence_errors, :197-249.  Item (s, l) of a pair = start frame s * step, length l; the workgroup's stride is a
// multiple of 8, so a thread keeps one length.  The rows of a pair are ordered by start frame, then length (the devkit's
// loop order); the lengths ascend, so the lengths a start has are a prefix too, and row (s, l) sits at
// sum_l' min(s, count[l']) + l.
__global__ __launch_bounds__(kEvalThreads) void eval_segments_kernel(EvalArgs a) {
  __shared__ double red[4];
  __shared__ int cnt[kEvalLengths];
  const int t = blockIdx.x;
  const EvalTraj tr = a.traj[t];
  const double* dist = a.dist + tr.off;
  const double* E = a.E + tr.off * 12;
  const double* G = a.G + tr.off * 12;
  if (threadIdx.x < kEvalLengths) cnt[threadIdx.x] = a.counts[t * kEvalLengths + threadIdx.x];
  __syncthreads();
  const int l = threadIdx.x & (kEvalLengths - 1);
  const double L = a.lengths[l];
  const int64_t row_base = a.rows ? a.post[t].row_base : 0;
  double r_sum = 0.0, t_sum = 0.0;
  for (int s = threadIdx.x >> 3; s < cnt[l]; s += kEvalThreads / kEvalLengths) {
    const int first = s * a.step;
    const double thr = dist[first] + L;
    int lo = first, hi = tr.n - 1;                   // dist[n - 1] > thr: s < cnt[l]
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (dist[mid] > thr) hi = mid; else lo = mid + 1;
    }
    const int last = lo;
    const Pose dG = pose_mul(pose_inv(pose_load(G + (size_t)first * 12)), pose_load(G + (size_t)last * 12));
    const Pose dE = pose_mul(pose_inv(pose_load(E + (size_t)first * 12)), pose_load(E + (size_t)last * 12));
    const Pose err = pose_mul(pose_inv(dE), dG);
    const double r_err = rotation_error(err) / L;
    const double t_err = norm3(err.m[3], err.m[7], err.m[11]) / L;
    r_sum += r_err;
    t_sum += t_err;
    if (a.rows) {
      int64_t pos = row_base + l;
#pragma unroll
      for (int k = 0; k < kEvalLengths; k++) pos += min(s, cnt[k]);
      if (pos < a.row_cap) {
        cfear_eval_row row;
        row.trajectory = t; row.first_frame = first; row.last_frame = last; row.pad = 0;
        row.length = L;
        row.r_err = r_err;
        row.t_err = t_err;
        row.speed = L / (0.1 * ((double)(last - first) + 1.0));   // :245-246
        a.rows[pos] = row;
      }
    }
  }
  double tot_r = 0.0, tot_t = 0.0;
  int64_t m = 0;
  cfear_eval_summary* out = a.summaries + t;
  for (int k = 0; k < kEvalLengths; k++) {
    const double sr = block_sum(l == k ? r_sum : 0.0, red), st = block_sum(l == k ? t_sum : 0.0, red);
    tot_r += sr;
    tot_t += st;
    m += cnt[k];
    if (threadIdx.x == 0) {
      out->seg_count[k] = cnt[k];
      out->seg_r_err[k] = cnt[k] ? sr / (double)cnt[k] : 0.0;
      out->seg_t_err[k] = cnt[k] ? st / (double)cnt[k] : 0.0;
    }
  }
  if (threadIdx.x == 0) {
    out->n_rows = m;
    out->ave_t_err = m ? tot_t / (double)m : 0.0;    // :279-287
    out->ave_r_err = m ? tot_r / (double)m : 0.0;
  }
}

// compute_ATE (:477-505) and compute_RPE (:508-583): rel_err = inv(inv(G_i) G_i+1) * (inv(E_i) E_i+1)
__device__ __forceinline__ Pose rel_err(const double* E, const double* G, int i) {
  const Pose g = pose_mul(pose_inv(pose_load(G + (size_t)i * 12)), pose_load(G + (size_t)(i + 1) * 12));
  const Pose e = pose_mul(pose_inv(pose_load(E + (size_t)i * 12)), pose_load(E + (size_t)(i + 1) * 12));
  return pose_mul(pose_inv(g), e);
}

__global__ __launch_bounds__(kEvalThreads) void eval_frames_kernel(EvalArgs a) {
  __shared__ double red[4];
  const int t = blockIdx.x;
  const EvalTraj tr = a.traj[t];
  const double* E = a.E + tr.off * 12;
  const double* G = a.G + tr.off * 12;
  double2* frame = a.frame + tr.off;
  double s_ate = 0.0, s_tr = 0.0, s_sq = 0.0, s_rot = 0.0, s_x = 0.0, s_y = 0.0, s_eul = 0.0;
  for (int i = threadIdx.x; i < tr.n; i += kEvalThreads) {
    const double* pe = E + (size_t)i * 12;
    const double* pg = G + (size_t)i * 12;
    const double e = norm3(pg[3] - pe[3], pg[7] - pe[7], pg[11] - pe[11]);     // sqrt(sum(align_err ** 2)), squared again at :504
    s_ate += e * e;
    if (i < tr.n - 1) {
      const Pose r = rel_err(E, G, i);
      const double tr_abs = norm3(r.m[3], r.m[7], r.m[11]), rot_abs = rotation_error(r);
      frame[i] = make_double2(tr_abs, rot_abs);      // read back by this same thread below
      s_tr += tr_abs;
      s_sq += (r.m[3] * r.m[3] + r.m[7] * r.m[7]) + r.m[11] * r.m[11];
      s_rot += rot_abs;
      s_x += r.m[3];
      s_y += r.m[7];
      // rot2eul(rotmat)[0], :14-18 and :550-551: the angle about x, as the devkit computes its "bias_theta"
      const double beta = -asin(r.m[8]);
      s_eul += atan2(r.m[9] / cos(beta), r.m[10] / cos(beta));
    }
  }
  const double nf = (double)tr.n, nr = (double)(tr.n - 1);
  const double ate = __dsqrt_rn(block_sum(s_ate, red) / nf);
  const double rpe_trans = block_sum(s_tr, red) / nr, rmse = __dsqrt_rn(block_sum(s_sq, red) / nr);
  const double rpe_rot = block_sum(s_rot, red) / nr;
  const double bias_x = block_sum(s_x, red) / nr, bias_y = block_sum(s_y, red) / nr, bias_theta = block_sum(s_eul, red) / nr;
  // np.std: the population deviation about the mean, in a second pass
  double d_tr = 0.0, d_rot = 0.0;
  for (int i = threadIdx.x; i < tr.n - 1; i += kEvalThreads) {
    const double2 f = frame[i];
    const double u = f.x - rpe_trans, v = f.y - rpe_rot;
    d_tr += u * u;
    d_rot += v * v;
  }
  const double dev_tr = __dsqrt_rn(block_sum(d_tr, red) / nr), dev_rot = __dsqrt_rn(block_sum(d_rot, red) / nr);
  if (threadIdx.x == 0) {
    cfear_eval_summary* out = a.summaries + t;       // eval_segments_kernel wrote the segment figures before this launch
    out->ate = ate;
    out->rpe_trans = rpe_trans; out->rpe_trans_dev = dev_tr;
    out->rpe_rot = rpe_rot; out->rpe_rot_dev = dev_rot;
    out->bias_x = bias_x; out->bias_y = bias_y; out->bias_theta = bias_theta;
    out->rmse_trans = rmse;
    out->n_poses = tr.n;
    const EvalPost& post = a.post[t];
    for (int k = 0; k < 12; k++) out->align[k] = post.align[k];
    const double all = ((((out->ave_t_err + out->ave_r_err) + ate) + (rpe_trans + dev_tr)) + ((rpe_rot + dev_rot) + (bias_x + bias_y))) +
                       (bias_theta + rmse);
    out->status = post.status != CFEAR_OK ? post.status : (all - all == 0.0 ? CFEAR_OK : CFEAR_ERR_SOLVER);   // a NaN / inf figure
  }
}

}  // namespace

// ---- host: the 3 x 3 SVD of umeyama_alignment (:63-77) ------------------------------------------------------------
// One-sided Jacobi: the columns of C V are rotated until they are orthogonal, C V = U S.  r = u diag(1, 1, det u det v) v^T
// is formed from the two leading singular pairs alone, u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T: the third pair of a
// planar trajectory belongs to the singular value 0 and is arbitrary in sign, and this form never reads it.
// Returns false when the second singular value vanishes (all positions on one line): the rotation is then undetermined.
// cfear_graph_align_batch (graphfinish.hip) solves its own s[15] with it.
bool cfear_align_from_sums(const double* s /*[15]*/, double align[12]) {
  double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) A[r][c] = s[6 + 3 * r + c];
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double al = 0, be = 0, ga = 0;
        for (int i = 0; i < 3; i++) { al += A[i][p] * A[i][p]; be += A[i][q] * A[i][q]; ga += A[i][p] * A[i][q]; }
        // columns whose computed dot product is rounding noise are orthogonal: below that a rotation only moves noise
        if (ga == 0.0 || std::fabs(ga) <= 2.0 * DBL_EPSILON * std::sqrt(al * be)) continue;
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double tn = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + tn * tn), sn = cs * tn;
        for (int i = 0; i < 3; i++) {
          const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
          A[i][p] = cs * ap - sn * aq; A[i][q] = sn * ap + cs * aq;
          V[i][p] = cs * vp - sn * vq; V[i][q] = sn * vp + cs * vq;
        }
      }
    if (!rotated) break;
  }
  double sv[3];
  int order[3] = {0, 1, 2};
  for (int c = 0; c < 3; c++) sv[c] = std::sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
  std::sort(order, order + 3, [&](int x, int y) { return sv[x] > sv[y]; });
  const int c1 = order[0], c2 = order[1];
  double r[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const bool ok = sv[c1] > 0.0 && sv[c2] > 1e-12 * sv[c1] && std::isfinite(sv[c1]);
  if (ok) {
    double u1[3], u2[3], v1[3], v2[3];
    for (int i = 0; i < 3; i++) { u1[i] = A[i][c1] / sv[c1]; u2[i] = A[i][c2] / sv[c2]; v1[i] = V[i][c1]; v2[i] = V[i][c2]; }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r[i][j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) align[4 * i + j] = r[i][j];
    align[4 * i + 3] = s[3 + i] - ((r[i][0] * s[0] + r[i][1] * s[1]) + r[i][2] * s[2]);      // t = mean_y - r mean_x, :77
  }
  return ok;
}

namespace {
int check_eval_params(const cfear_eval_params* par) {
  if (!par || par->step_size < 1) return CFEAR_ERR_INVALID_ARGUMENT;
  if (par->alignment != CFEAR_EVAL_ALIGN_NONE && par->alignment != CFEAR_EVAL_ALIGN_6DOF) return CFEAR_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < kEvalLengths; k++) {
    if (!(par->lengths[k] > 0.0) || !std::isfinite(par->lengths[k])) return CFEAR_ERR_INVALID_ARGUMENT;
    if (k > 0 && !(par->lengths[k] > par->lengths[k - 1])) return CFEAR_ERR_INVALID_ARGUMENT;
  }
  return CFEAR_OK;
}
}  // namespace

extern "C" void cfear_eval_params_default(cfear_eval_params* p) {
  p->step_size = 10;                                 // eval_odom.py's default --step_size
  p->alignment = CFEAR_EVAL_ALIGN_6DOF;              // every run script of the reference
  for (int k = 0; k < kEvalLengths; k++) p->lengths[k] = 100.0 * (k + 1);   // :90
}

extern "C" int cfear_eval_check(const cfear_eval_params* par, const int32_t* est_lengths, const int32_t* gt_lengths, int32_t n_traj) {
  CFEAR_CHECK(check_eval_params(par));
  if (n_traj < 0 || (n_traj > 0 && (!est_lengths || !gt_lengths))) return CFEAR_ERR_INVALID_ARGUMENT;
  for (int t = 0; t < n_traj; t++)
    if (est_lengths[t] != gt_lengths[t] || est_lengths[t] < 2) return CFEAR_ERR_INVALID_ARGUMENT;
  return CFEAR_OK;
}

extern "C" int cfear_eval_trajectories(cfear_ctx* ctx, const double* est, const double* gt, const int64_t* offsets,
                                       const int32_t* lengths, int32_t n_traj, const cfear_eval_params* par,
                                       cfear_eval_summary* summaries, cfear_eval_row* rows, int64_t row_cap, int64_t* n_rows) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (check_eval_params(par) != CFEAR_OK)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT,
                           "evaluation parameters: step_size >= 1, alignment none or 6dof (scale, 7dof and scale_7dof are not "
                           "supported), 8 ascending positive lengths");
  if (n_traj < 0 || (n_traj > 0 && (!est || !gt || !lengths || !summaries)) || row_cap < 0 || (row_cap > 0 && !rows))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if ((n_traj > 0 && (cfear_is_device_ptr(offsets) || cfear_is_device_ptr(lengths))) || (n_rows && cfear_is_device_ptr(n_rows)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "offsets, lengths and n_rows must be host memory");
  if (cfear_eval_check(par, lengths, lengths, n_traj) != CFEAR_OK)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "a trajectory has fewer than 2 poses");
  if (n_rows) *n_rows = 0;
  if (n_traj == 0) return CFEAR_OK;
  if (((uintptr_t)est | (uintptr_t)gt) & 15) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "est and gt must be 16-byte aligned");
  if (!row_cap) rows = nullptr;
  // the pairs: where they are, the workspace prefix, the launch extents
  std::vector<EvalTraj> traj(n_traj);
  std::vector<double> h_sums((size_t)n_traj * 16);
  std::vector<int32_t> h_counts((size_t)n_traj * kEvalLengths);
  std::vector<int2> blocks;                          // the per-pose kernels' flat grid: a ragged batch launches no empty workgroups
  int64_t total = 0, span = 0;
  bool grid_ok = true;
  for (int t = 0; t < n_traj; t++) {
    const int64_t src = offsets ? offsets[t] : total;
    if (src < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "trajectory %d: negative offset", t);
    traj[t] = EvalTraj{src, total, lengths[t], (int32_t)(((int64_t)lengths[t] + par->step_size - 1) / par->step_size)};
    total += lengths[t];
    span = std::max(span, src + lengths[t]);
    grid_ok = flat_grid_add(blocks, t, lengths[t], kEvalThreads) && grid_ok;
  }
  if (!grid_ok) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 x 256 poses in one call");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsEval);
  EvalArgs a{};
  st.in(a.est, est, (size_t)span * 96);
  st.in(a.gt, gt, (size_t)span * 96);
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "est and gt must both be host or both be device memory");
  StagedTables tab(st, (size_t)n_traj * sizeof(EvalTraj), blocks.size() * sizeof(int2), (size_t)n_traj * sizeof(EvalPost));
  st.piece(a.E, (size_t)total * 96);
  st.piece(a.G, (size_t)total * 96);
  st.piece(a.dist, (size_t)total * 8);
  st.piece(a.frame, (size_t)total * 16);
  st.piece(a.sums, (size_t)n_traj * 16 * 8);
  st.piece(a.counts, (size_t)n_traj * kEvalLengths * 4);
  st.out(a.summaries, summaries, (size_t)n_traj * sizeof(cfear_eval_summary));
  if (rows) st.out(a.rows, rows, (size_t)row_cap * sizeof(cfear_eval_row));
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(tab.upload(traj.data(), blocks.data()));
  a.traj = tab.records<EvalTraj>();
  a.blocks = tab.blocks<int2>();
  a.post = tab.second<EvalPost>();
  a.row_cap = rows ? row_cap : 0;
  a.n_traj = n_traj;
  a.step = par->step_size;
  for (int k = 0; k < kEvalLengths; k++) a.lengths[k] = par->lengths[k];
  const bool align = par->alignment == CFEAR_EVAL_ALIGN_6DOF;
  const dim3 per_pose((unsigned)blocks.size());
  {
    ProfScope ps(ctx, "eval_normalise");
    hipLaunchKernelGGL(eval_normalise_kernel, per_pose, dim3(kEvalThreads), 0, ctx->stream, a);
  }
  if (align) {
    ProfScope ps(ctx, "eval_align_sums");
    hipLaunchKernelGGL(eval_align_sums_kernel, dim3(n_traj), dim3(kEvalThreads), 0, ctx->stream, a);
  }
  {
    ProfScope ps(ctx, "eval_distance");
    hipLaunchKernelGGL(eval_distance_kernel, dim3(n_traj), dim3(64), 0, ctx->stream, a);
  }
  {
    ProfScope ps(ctx, "eval_counts");
    hipLaunchKernelGGL(eval_counts_kernel, dim3((n_traj * kEvalLengths + kEvalThreads - 1) / kEvalThreads), dim3(kEvalThreads), 0,
                       ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  // host half: the row table's prefix and the alignment of every pair
  st.fetch(h_counts.data(), a.counts, h_counts.size() * 4);
  if (align) st.fetch(h_sums.data(), a.sums, h_sums.size() * 8);
  CFEAR_CHECK(st.wait());
  EvalPost* post = tab.host_second<EvalPost>();
  int64_t row_total = 0;
  for (int t = 0; t < n_traj; t++) {
    memcpy(post[t].align, kIdentityRows, sizeof(kIdentityRows));
    post[t].status = CFEAR_OK;
    post[t].pad = 0;
    if (align && !cfear_align_from_sums(h_sums.data() + (size_t)t * 16, post[t].align)) post[t].status = CFEAR_ERR_SOLVER;
    post[t].row_base = row_total;
    for (int k = 0; k < kEvalLengths; k++) row_total += h_counts[(size_t)t * kEvalLengths + k];
  }
  if (n_rows) *n_rows = row_total;
  CFEAR_CHECK(tab.upload_second());
  if (align) {
    ProfScope ps(ctx, "eval_apply_align");
    hipLaunchKernelGGL(eval_apply_align_kernel, per_pose, dim3(kEvalThreads), 0, ctx->stream, a);
  }
  {
    ProfScope ps(ctx, "eval_segments");
    hipLaunchKernelGGL(eval_segments_kernel, dim3(n_traj), dim3(kEvalThreads), 0, ctx->stream, a);
  }
  {
    ProfScope ps(ctx, "eval_frames");
    hipLaunchKernelGGL(eval_frames_kernel, dim3(n_traj), dim3(kEvalThreads), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  CFEAR_CHECK(st.finish());
  if (rows && row_total > row_cap)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "%lld rows, the table holds %lld (the summaries are complete)", (long long)row_total,
                           (long long)row_cap);
  return CFEAR_OK;
}

// ---- host helpers, no context ---------------------------------------------------------------------------------------
// load_poses_from_txt, :93-121: 12 numbers per line (a 3 x 4 matrix, row by row), or 13 with the frame index first
extern "C" int cfear_kitti_read(const char* path, double* poses, int64_t cap, int64_t* n_out) {
  if (!path || !n_out || cap < 0 || (cap > 0 && !poses)) return CFEAR_ERR_INVALID_ARGUMENT;
  FILE* f = fopen(path, "r");
  if (!f) return CFEAR_ERR_IO;
  std::string line;
  int64_t n = 0;
  int rc = CFEAR_OK;
  char buf[4096];
  while (rc == CFEAR_OK && fgets(buf, sizeof(buf), f)) {
    line = buf;
    while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof(buf), f)) line += buf;
    double v[14];
    int m = 0;
    const char* p = line.c_str();
    while (m < 14) {
      char* end;
      const double x = strtod(p, &end);
      if (end == p) break;
      v[m++] = x;
      p = end;
    }
    while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
    if (m == 0 && !*p) continue;                     // an empty line
    // the devkit keys its dictionaries by the index of a 13-number line; only a gapless file has a defined evaluation
    if (*p || (m != 12 && m != 13) || (m == 13 && v[0] != (double)n)) { rc = CFEAR_ERR_FORMAT; break; }
    if (n < cap) memcpy(poses + n * 12, v + (m - 12), 96);
    n++;
  }
  fclose(f);
  if (rc != CFEAR_OK) return rc;
  *n_out = n;
  return n > cap && poses ? CFEAR_ERR_CAPACITY : CFEAR_OK;
}

// EvalTrajectory::Write, eval_trajectory.cpp:169-183: std::fixed with the stream's 6 decimals, one space between numbers
extern "C" int cfear_kitti_write(const char* path, const double* poses, int64_t n) {
  if (!path || n < 0 || (n > 0 && !poses)) return CFEAR_ERR_INVALID_ARGUMENT;
  FILE* f = fopen(path, "w");
  if (!f) return CFEAR_ERR_IO;
  bool ok = true;
  for (int64_t i = 0; i < n && ok; i++) ok = kitti_row_write(f, poses + i * 12, "\n");
  ok = fclose(f) == 0 && ok;
  return ok ? CFEAR_OK : CFEAR_ERR_IO;
}

// planar (x, y, theta) -> [cos -sin 0 x; sin cos 0 y; 0 0 1 0]; stride in doubles between poses (3 for packed triples,
// sizeof(cfear_frame_info) / 8 to read the pose of every record of one stream's history)
extern "C" int cfear_kitti_from_xyt(const double* xyt, int64_t n, int64_t stride, double* poses) {
  if (n < 0 || stride < 3 || (n > 0 && (!xyt || !poses))) return CFEAR_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; i++) {
    const double* p = xyt + i * stride;
    const double c = std::cos(p[2]), s = std::sin(p[2]);
    const double m[12] = {c, -s, 0.0, p[0], s, c, 0.0, p[1], 0.0, 0.0, 1.0, 0.0};
    memcpy(poses + i * 12, m, sizeof(m));
  }
  return CFEAR_OK;
}
