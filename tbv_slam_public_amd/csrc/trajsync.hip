// trajsync.hip -- synchronising estimate and ground-truth trajectories by time, for a batch of pairs in one call: what every
// executable of the reference ends in, EvalTrajectory::Save() -> One2OneCorrespondance()
// (cfear_radarodometry/src/cfear_radarodometry/eval_trajectory.cpp:400-423, cited below as :line), and the one-stamp
// Interpolate(t, out) of eval_trajectory.h:141-144.  DESIGN.md section 4.16.
//
// Per estimate the reference walks the ground truth interval by interval from a carried position (SearchByTime, :424-442)
// and interpolates in the first interval [t_j, t_j+1] that contains the stamp (pose_interp, :461-491).  On a ground truth
// whose stamps do not descend the intervals that contain a stamp are a contiguous range [a, b], so the walk is
//     x' = max(x, a) <= b ? max(x, a) : 0          (kept iff max(x, a) <= b; a miss resets the position, :412)
// and only this recurrence is serial.  All comparisons are on ros::Time::toSec() doubles, as in the reference.
//
// Kernels:
//   sync_check    workgroups per pair         device buffers only: the stamps' range and the ground truth's order
//   sync_search   thread per estimate         toSec and two binary searches -> [a, b]
//   sync_chain    wavefront per pair          the recurrence, 64 ranges at a time through readlane; the exclusive prefix of
//                                             the kept flags (ballot + popcount); independent mode skips the recurrence
//   sync_interp   thread per estimate         pose_interp of the kept estimates, written compacted
// Everything is fp64 without contraction (-ffp-contract=off).  The three Eigen 3.3 routines pose_interp calls (matrix ->
// quaternion and toRotationMatrix in eigen_quat.hpp, slerp here) and roscpp's toSec are restated operation by operation; neither Eigen nor ROS
// is part of the reference tree or of this build ("restated, not pinned").
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

#include "pose_rows.hpp"    // Pose; eigen_quat.hpp: quat_from_rows (Eigen 3.3 Quaternion(Matrix3d), no normalisation), quat_to_rows

namespace {
constexpr int kSyncThreads = 256;
constexpr int64_t kNsPerSec = 1000000000ll;
constexpr int64_t kMaxSec = 4294967295ll;          // ros::Time::sec is a uint32
static_assert(sizeof(cfear_sync_row) == 16, "cfear_sync_row is 16 bytes (include/cfear_hip.h)");

struct SyncPair {          // one pair: where its poses and stamps are in the caller's arrays and in the workspace
  int64_t est_src;         // first estimate in est / est_stamps, and first kept row in the four outputs
  int64_t gt_src;          // first ground-truth pose in gt / gt_stamps
  int64_t ws;              // first estimate in `range`
  int32_t n_est, n_gt;
};
struct SyncArgs {
  const SyncPair* pairs;
  const int2* blocks;      // per-estimate kernels: (pair, first estimate of the pair) of every workgroup
  const double* est;       // nullable
  const int64_t* est_stamps;
  const double* gt;
  const int64_t* gt_stamps;
  int2* range;             // [total estimates]: (a, b) after sync_search, (gt index or -1, row within the pair) after sync_chain
  double* est_out;
  double* gt_out;
  int64_t* stamps_out;
  cfear_sync_row* rows;
  int32_t* counts;         // [n_traj]
  unsigned long long* flags;   // [3]: first (pair << 32 | index) with a bad estimate stamp, a bad ground-truth stamp, a descent; null: host buffers, checked on the host
  int32_t n_traj, mode;
};

// roscpp's TimeBase::toSec(): (double)sec + 1e-9 * (double)nsec, with sec = ns / 10^9 (what toNSec() inverts)
__host__ __device__ __forceinline__ double to_sec(int64_t ns) {
  const int64_t sec = ns / kNsPerSec;
  return (double)sec + 1e-9 * (double)(ns - sec * kNsPerSec);
}
__host__ __device__ __forceinline__ bool stamp_ok(int64_t ns) { return ns >= 0 && ns / kNsPerSec <= kMaxSec; }

// pose_interp, :461-491
__device__ __forceinline__ Pose pose_interp(double alpha, const Pose& A, const Pose& B) {
  double qa[4], qb[4], q[4];
  quat_from_rows(A.m, qa);
  quat_from_rows(B.m, qb);
  // QuaternionBase::slerp (Eigen 3.3).  dot() is the 2-wide packet reduction of the four products: (xx + zz) + (yy + ww)
  const double d = (qa[0] * qb[0] + qa[2] * qb[2]) + (qa[1] * qb[1] + qa[3] * qb[3]);
  const double abs_d = fabs(d);
  double scale0, scale1;
  if (abs_d >= 1.0 - DBL_EPSILON) {
    scale0 = 1.0 - alpha;
    scale1 = alpha;
  } else {
    const double theta = acos(abs_d);
    const double sin_theta = sin(theta);
    scale0 = sin((1.0 - alpha) * theta) / sin_theta;
    scale1 = sin(alpha * theta) / sin_theta;
  }
  if (d < 0.0) scale1 = -scale1;
#pragma unroll
  for (int k = 0; k < 4; k++) q[k] = scale0 * qa[k] + scale1 * qb[k];
  Pose R;
  quat_to_rows(q, R.m);
  R.m[3] = (1.0 - alpha) * A.m[3] + alpha * B.m[3];
  R.m[7] = (1.0 - alpha) * A.m[7] + alpha * B.m[7];
  R.m[11] = 0.0;                                       // result.translation()(2) = 0, :488
  return R;
}

__device__ __forceinline__ void flag_min(unsigned long long* flag, int pair, int index) {
  atomicMin(flag, ((unsigned long long)(unsigned)pair << 32) | (unsigned)index);
}

// sync_check_kernel found a stamp the call refuses: the kernels behind it on the stream write nothing, and the host reads the
// flags together with the counts, behind the one synchronisation of the call
__device__ __forceinline__ bool sync_refused(const SyncArgs& a) {
  return a.flags && (gload<unsigned long long>(a.flags) & gload<unsigned long long>(a.flags + 1) & gload<unsigned long long>(a.flags + 2)) != ~0ull;
}

__global__ __launch_bounds__(kSyncThreads) void sync_check_kernel(SyncArgs a) {
  const int t = blockIdx.x;
  const SyncPair p = a.pairs[t];
  const int first = blockIdx.y * kSyncThreads + threadIdx.x, stride = gridDim.y * kSyncThreads;   // gridDim.y workgroups share a long pair
  for (int i = first; i < p.n_est; i += stride)
    if (!stamp_ok(gload<int64_t>(a.est_stamps + p.est_src + i))) { flag_min(a.flags, t, i); break; }
  for (int i = first; i < p.n_gt; i += stride) {
    const int64_t s = gload<int64_t>(a.gt_stamps + p.gt_src + i);
    if (!stamp_ok(s)) flag_min(a.flags + 1, t, i);
    if (i > 0 && s < gload<int64_t>(a.gt_stamps + p.gt_src + i - 1)) flag_min(a.flags + 2, t, i);
  }
}

// The intervals j in [0, n - 2] with t_j <= ts <= t_j+1: t_j <= ts holds up to the last stamp <= ts, ts <= t_j+1 from the
// interval before the first stamp >= ts.  An empty range has a > b.  SearchByTime finds nothing in 2 poses or fewer (:426).
__global__ __launch_bounds__(kSyncThreads) void sync_search_kernel(SyncArgs a) {
  if (sync_refused(a)) return;
  const int2 blk = a.blocks[blockIdx.x];
  const SyncPair p = a.pairs[blk.x];
  const int i = blk.y + threadIdx.x;
  if (i >= p.n_est) return;
  int2 r = make_int2(1, 0);
  if (p.n_gt > 2) {
    const double ts = to_sec(gload<int64_t>(a.est_stamps + p.est_src + i));
    const int64_t* g = a.gt_stamps + p.gt_src;
    int lo = 0, hi = p.n_gt;                           // first stamp >= ts
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (to_sec(gload<int64_t>(g + mid)) < ts) lo = mid + 1; else hi = mid;
    }
    const int first_ge = lo;
    hi = p.n_gt;                                       // first stamp > ts: not before first_ge
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (to_sec(gload<int64_t>(g + mid)) <= ts) lo = mid + 1; else hi = mid;
    }
    r = make_int2(max(first_ge - 1, 0), min(lo - 1, p.n_gt - 2));
  }
  a.range[p.ws + i] = r;
}

// One wavefront per pair.  The carried position is wave-uniform; lane k keeps the outcome of estimate base + k.  Lanes past
// the end hold the range [0, INT_MAX], which leaves the position as it is.
__global__ __launch_bounds__(CFEAR_WAVE) void sync_chain_kernel(SyncArgs a) {
  if (sync_refused(a)) return;
  const int t = blockIdx.x;
  const SyncPair p = a.pairs[t];
  const int lane = threadIdx.x;
  int2* range = a.range + p.ws;
  int x = 0, kept_before = 0;
  for (int base = 0; base < p.n_est; base += CFEAR_WAVE) {
    const int i = base + lane;
    const int2 r = i < p.n_est ? range[i] : make_int2(0, INT_MAX);
    int mine = r.x <= r.y ? r.x : -1;                  // Interpolate(t, out): every stamp searches from the first pose
    if (a.mode == CFEAR_SYNC_CHAINED) {
#pragma unroll
      for (int k = 0; k < CFEAR_WAVE; k++) {
        const int c = max(x, __builtin_amdgcn_readlane(r.x, k));
        const bool hit = c <= __builtin_amdgcn_readlane(r.y, k);
        x = hit ? c : 0;
        if (lane == k) mine = hit ? c : -1;
      }
    }
    const bool kept = i < p.n_est && mine >= 0;
    const unsigned long long mask = __ballot(kept);
    const int pos = kept_before + __popcll(mask & ((1ull << lane) - 1ull));
    kept_before += __popcll(mask);
    if (i < p.n_est) range[i] = make_int2(mine, kept ? pos : -1);
  }
  if (lane == 0) a.counts[t] = kept_before;
}

__global__ __launch_bounds__(kSyncThreads) void sync_interp_kernel(SyncArgs a) {
  if (sync_refused(a)) return;
  const int2 blk = a.blocks[blockIdx.x];
  const SyncPair p = a.pairs[blk.x];
  const int i = blk.y + threadIdx.x;
  if (i >= p.n_est) return;
  const int2 r = a.range[p.ws + i];
  if (r.x < 0) return;
  const int64_t stamp = gload<int64_t>(a.est_stamps + p.est_src + i);
  const double ts = to_sec(stamp);
  const double t1 = to_sec(gload<int64_t>(a.gt_stamps + p.gt_src + r.x)), t2 = to_sec(gload<int64_t>(a.gt_stamps + p.gt_src + r.x + 1));
  double alpha = 0.0;
  if (t2 != t1) alpha = (ts - t1) / (t2 - t1);
  const double* g = a.gt + (p.gt_src + r.x) * 12;
  const int64_t o = p.est_src + r.y;
  pose_store(a.gt_out + o * 12, pose_interp(alpha, pose_load(g), pose_load(g + 12)));
  if (a.est) pose_store(a.est_out + o * 12, pose_load(a.est + (p.est_src + i) * 12));
  a.stamps_out[o] = stamp;
  cfear_sync_row row;
  row.est_index = i; row.gt_index = r.x; row.alpha = alpha;
  a.rows[o] = row;
}
void split_flag(unsigned long long f, int* pair, int* index) { *pair = (int)(f >> 32); *index = (int)(f & 0xffffffffu); }
const char kBadStamp[] = "is negative or past 2^32 - 1 seconds";

bool write_stamp(FILE* f, int64_t ns) {                // `sec.` + nsec zero-padded to 9 digits + ` ` (:192, :221)
  return fprintf(f, "%lld.%09lld ", (long long)(ns / kNsPerSec), (long long)(ns % kNsPerSec)) > 0;
}
}  // namespace

extern "C" int cfear_sync_trajectories(cfear_ctx* ctx, int32_t mode, const double* est, const int64_t* est_stamps, const int64_t* est_offsets,
                                       const int32_t* est_lengths, const double* gt, const int64_t* gt_stamps, const int64_t* gt_offsets,
                                       const int32_t* gt_lengths, int32_t n_traj, double* est_out, double* gt_out, int64_t* stamps_out,
                                       cfear_sync_row* rows, int32_t* counts) {
  // ---- everything that can be checked on the host is, before a context is needed and before anything is written ---------
  if (mode != CFEAR_SYNC_CHAINED && mode != CFEAR_SYNC_INDEPENDENT)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "unknown mode %d", (int)mode);
  if (n_traj < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_traj is negative");
  if (n_traj > 0 && (!est_lengths || !gt_lengths || !counts)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_traj > 0 && (cfear_is_device_ptr(est_lengths) || cfear_is_device_ptr(gt_lengths) || cfear_is_device_ptr(counts) ||
                     cfear_is_device_ptr(est_offsets) || cfear_is_device_ptr(gt_offsets)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "offsets, lengths and counts must be host memory");
  std::vector<SyncPair> pairs((size_t)n_traj);
  std::vector<int2> blocks;
  int64_t total_est = 0, total_gt = 0, span_est = 0, span_gt = 0;
  bool grid_ok = true;
  for (int t = 0; t < n_traj; t++) {
    if (est_lengths[t] < 0 || gt_lengths[t] < 0)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: negative length", t);
    const int64_t es = est_offsets ? est_offsets[t] : total_est, gs = gt_offsets ? gt_offsets[t] : total_gt;
    if (es < 0 || gs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: negative offset", t);
    pairs[t] = SyncPair{es, gs, total_est, est_lengths[t], gt_lengths[t]};
    total_est += est_lengths[t];
    total_gt += gt_lengths[t];
    span_est = std::max(span_est, es + est_lengths[t]);
    span_gt = std::max(span_gt, gs + gt_lengths[t]);
    grid_ok = flat_grid_add(blocks, t, est_lengths[t], kSyncThreads) && grid_ok;
  }
  if (total_est > 0 && (!est_stamps || !stamps_out || !gt_out || !rows || (est && !est_out)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (total_gt > 0 && (!gt || !gt_stamps)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  const int kind = memory_kind({total_est ? est : nullptr, total_est ? est_stamps : nullptr, total_gt ? gt : nullptr,
                                total_gt ? gt_stamps : nullptr, total_est && est ? est_out : nullptr, total_est ? gt_out : nullptr,
                                total_est ? stamps_out : nullptr, total_est ? rows : nullptr});
  if (kind < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT,
                           "est, est_stamps, gt, gt_stamps and the four outputs must be all host or all device memory");
  const bool host = kind == 0;
  if (host) {
    for (int t = 0; t < n_traj; t++) {
      const SyncPair& p = pairs[t];
      for (int i = 0; i < p.n_est; i++)
        if (!stamp_ok(est_stamps[p.est_src + i]))
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: estimate stamp %d %s", t, i, kBadStamp);
      for (int i = 0; i < p.n_gt; i++)
        if (!stamp_ok(gt_stamps[p.gt_src + i]))
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: ground-truth stamp %d %s", t, i, kBadStamp);
      for (int i = 1; i < p.n_gt; i++)
        if (gt_stamps[p.gt_src + i] < gt_stamps[p.gt_src + i - 1])
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: ground-truth stamp %d is earlier than the one before it", t, i);
    }
  } else if ((((uintptr_t)est | (uintptr_t)gt | (uintptr_t)est_out | (uintptr_t)gt_out) & 15) ||
             (((uintptr_t)est_stamps | (uintptr_t)gt_stamps | (uintptr_t)stamps_out | (uintptr_t)rows) & 7)) {
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "device poses must be 16-byte aligned, device stamps and rows 8-byte aligned");
  }
  if (!grid_ok) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 x 256 estimates in one call");
  if (!ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null context");
  if (n_traj == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (total_est == 0 && host) {                        // nothing to search, nothing to launch
    for (int t = 0; t < n_traj; t++) counts[t] = 0;
    return CFEAR_OK;
  }
  HostStage st(ctx, kWsTrajSync);
  SyncArgs a{};
  st.in(a.est, est, (size_t)span_est * 96);
  st.in(a.est_stamps, est_stamps, (size_t)span_est * 8);
  st.in(a.gt, gt, (size_t)span_gt * 96);
  st.in(a.gt_stamps, gt_stamps, (size_t)span_gt * 8);
  // a host caller's outputs are staged and only the kept rows of every pair are copied back, once the counts are known
  if (host) {
    if (est) st.piece(a.est_out, (size_t)span_est * 96);
    st.piece(a.gt_out, (size_t)span_est * 96);
    st.piece(a.stamps_out, (size_t)span_est * 8);
    st.piece(a.rows, (size_t)span_est * sizeof(cfear_sync_row));
  } else {
    a.est_out = est_out; a.gt_out = gt_out; a.stamps_out = stamps_out; a.rows = rows;
  }
  StagedTables tab(st, (size_t)n_traj * sizeof(SyncPair), blocks.size() * sizeof(int2), 32);   // second piece: the check's flags
  st.piece(a.range, (size_t)total_est * sizeof(int2));
  st.piece(a.counts, (size_t)n_traj * 4);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(tab.upload(pairs.data(), blocks.data()));
  a.pairs = tab.records<SyncPair>();
  a.blocks = tab.blocks<int2>();
  a.n_traj = n_traj;
  a.mode = mode;
  unsigned long long* const d_flags = tab.second<unsigned long long>();
  if (!host) {                                         // also without a single estimate: the ground truth is checked as a host caller's is
    unsigned long long* hf = tab.host_second<unsigned long long>();
    hf[0] = hf[1] = hf[2] = hf[3] = ~0ull;
    CFEAR_CHECK(tab.upload_second());
    a.flags = d_flags;
    ProfScope ps(ctx, "sync_check");
    const int64_t longest = std::max<int64_t>(*std::max_element(est_lengths, est_lengths + n_traj), *std::max_element(gt_lengths, gt_lengths + n_traj));
    const unsigned share = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, longest / (16 * kSyncThreads)));   // >= 16 stamps per thread
    hipLaunchKernelGGL(sync_check_kernel, dim3(n_traj, share), dim3(kSyncThreads), 0, ctx->stream, a);
  }
  if (total_est > 0) {
    const dim3 per_estimate((unsigned)blocks.size());
    {
      ProfScope ps(ctx, "sync_search");
      hipLaunchKernelGGL(sync_search_kernel, per_estimate, dim3(kSyncThreads), 0, ctx->stream, a);
    }
    {
      ProfScope ps(ctx, "sync_chain");
      hipLaunchKernelGGL(sync_chain_kernel, dim3(n_traj), dim3(CFEAR_WAVE), 0, ctx->stream, a);
    }
    {
      ProfScope ps(ctx, "sync_interp");
      hipLaunchKernelGGL(sync_interp_kernel, per_estimate, dim3(kSyncThreads), 0, ctx->stream, a);
    }
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  // the one synchronisation: the flags of the check and the counts
  unsigned long long got[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  std::vector<int32_t> h_counts((size_t)n_traj, 0);
  if (!host) st.fetch(got, d_flags, 32);
  if (total_est > 0) st.fetch(h_counts.data(), a.counts, (size_t)n_traj * 4);
  CFEAR_CHECK(st.wait());
  int first = -1;                                      // the first pair at fault; within it the order of the host checks
  for (int k = 0; k < 3; k++)
    if (got[k] != ~0ull && (first < 0 || (got[k] >> 32) < (got[first] >> 32))) first = k;
  if (first >= 0) {
    int t, i;
    split_flag(got[first], &t, &i);
    if (first == 2) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: ground-truth stamp %d is earlier than the one before it", t, i);
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d: %s stamp %d %s", t, first == 0 ? "estimate" : "ground-truth", i, kBadStamp);
  }
  memcpy(counts, h_counts.data(), (size_t)n_traj * 4);
  if (host)
    for (int t = 0; t < n_traj; t++) {
      const size_t o = (size_t)pairs[t].est_src, n = (size_t)counts[t];
      if (!n) continue;
      if (est) st.back(est_out + o * 12, a.est_out + o * 12, n * 96);
      st.back(gt_out + o * 12, a.gt_out + o * 12, n * 96);
      st.back(stamps_out + o, a.stamps_out + o, n * 8);
      st.back(rows + o, a.rows + o, n * sizeof(cfear_sync_row));
    }
  return st.finish();
}

// ---- host writers, no context -----------------------------------------------------------------------------------------
// EvalTrajectory::WriteTUM, :185-211: the stamp, the translation std::fixed with 4 decimals, the quaternion x y z w under
// std::defaultfloat with the precision still 4 (%.4g), from the matrix -> quaternion conversion above
extern "C" int cfear_tum_write(const char* path, const double* poses, const int64_t* stamps, int64_t n) {
  if (!path || n < 0 || (n > 0 && (!poses || !stamps))) return CFEAR_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; i++)
    if (!stamp_ok(stamps[i])) return CFEAR_ERR_INVALID_ARGUMENT;
  FILE* f = fopen(path, "w");
  if (!f) return CFEAR_ERR_IO;
  bool ok = true;
  for (int64_t i = 0; i < n && ok; i++) {
    const double* m = poses + i * 12;
    double q[4];
    quat_from_rows(m, q);
    ok = write_stamp(f, stamps[i]) && fprintf(f, "%.4f %.4f %.4f %.4g %.4g %.4g %.4g\n", m[3], m[7], m[11], q[0], q[1], q[2], q[3]) > 0;
  }
  ok = fclose(f) == 0 && ok;
  return ok ? CFEAR_OK : CFEAR_ERR_IO;
}

// EvalTrajectory::WriteCov, :214-232: the stamp, then the 6 x 6 covariance row-major through Eigen::IOFormat(StreamPrecision,
// DontAlignCols, " ", " "): the stream's default precision of 6 under defaultfloat, %g
extern "C" int cfear_cov_write(const char* path, const double* cov, const int64_t* stamps, int64_t n) {
  if (!path || n < 0 || (n > 0 && (!cov || !stamps))) return CFEAR_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; i++)
    if (!stamp_ok(stamps[i])) return CFEAR_ERR_INVALID_ARGUMENT;
  FILE* f = fopen(path, "w");
  if (!f) return CFEAR_ERR_IO;
  bool ok = true;
  for (int64_t i = 0; i < n && ok; i++) {
    ok = write_stamp(f, stamps[i]);
    for (int k = 0; k < 36 && ok; k++) ok = fprintf(f, k == 35 ? "%g\n" : "%g ", cov[i * 36 + k]) > 0;
  }
  ok = fclose(f) == 0 && ok;
  return ok ? CFEAR_OK : CFEAR_ERR_IO;
}
