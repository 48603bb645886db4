// closure.hip -- cfear_closure_candidates_batch: the two loop-candidate generators of the reference that need no
// descriptors, for a batch of complete pose graphs (gfx950, wave64, fp64).
//
// Restates, per origin node and from fresh state (empty pair_attempted_ / origin_attempted_, itr_current = begin),
//   GTVicinityClosure::SearchAndAddConstraint (tbv_slam/src/tbv_slam/loopclosure.cpp:394-467) with
//     PoseGraph::TraveledDistance / EuclidianDistance (posegraph.cpp:151-172), and
//   MiniClosure::SearchAndAddConstraint (loopclosure.cpp:469-552),
// and loopclosure::VerifyByOdometry (:776-806) for every pair they emit.
//
// The reference's GTVicinity search is O(N^3): every pair re-walks the constraints between its two nodes.  Here the walk
// from an origin is ONE serial sum that the origin's lane carries along its sweep over the later nodes:
//   trav(i, j) = ((0.0 + step[i]) + step[i + 1]) + ... + step[j - 1]
// which is what TraveledDistance returns for the pair and what MiniClosure's `trav_distance +=` holds at j, bit for bit
// (0.0 + d == d).  It is NOT a difference of prefix sums.
//
// closure_sweep_kernel: one lane per origin, one 64-lane workgroup per kClosureOrigins consecutive origins of one graph
// (a host-built block table maps workgroup -> graph, first origin, as pgo_batch.hip maps its chunks).  The later nodes are
// staged tile by tile into LDS as (x, y, z, step[j - 1]); in an iteration all lanes read the same LDS address (a
// broadcast).  Tiles that lie wholly at or before the workgroup's first origin are never staged.  Only the add chain is
// serial: the body is branch-free and unrolled, so the sqrt and the divide of several j are in flight at once.  Steps are
// validated non-negative, so trav never decreases and a lane is finished once trav > max_d_travel; the workgroup stops
// when all its lanes are.
// closure_odom_kernel: one lane per emitted pair, the arithmetic of cfear_verify_by_odometry (verify.hip) in its order.
#include <cfloat>
#include <cmath>

#include "common.hpp"
#include "pose2d.hpp"

namespace {

constexpr int kClosureOrigins = CFEAR_CLOSURE_ORIGINS;
constexpr int kClosureTile = CFEAR_CLOSURE_TILE;
constexpr int kClosureUnroll = 8;
static_assert(kClosureOrigins == CFEAR_WAVE, "one wavefront per workgroup: the all-lanes-finished test is one ballot");
static_assert(kClosureTile % kClosureUnroll == 0 && kClosureTile % kClosureOrigins == 0, "tiles are whole unrolled groups");

struct ClosureBlock {        // one workgroup's share
  int64_t node0;             // the graph's first node in the flat arrays
  int32_t n;                 // nodes of the graph
  int32_t origin0;           // first origin of the workgroup, within the graph
};
static_assert(sizeof(ClosureBlock) == 16, "block table record");

struct ClosureArgs {
  const double* pos;         // [n_nodes][3]
  const double* steps;       // [n_nodes]
  const double* rel;         // [n_nodes][3] or nullptr
  const ClosureBlock* blocks;
  cfear_closure_candidate* out;
  double min_d_travel, max_d_travel, max_d_close, two_sigma2;
  int32_t mode, verify_via_odometry;
};

__global__ __launch_bounds__(kClosureOrigins) void closure_sweep_kernel(const ClosureArgs a) {
  __shared__ double4 tile[kClosureTile];
  const ClosureBlock b = a.blocks[blockIdx.x];
  const int lane = threadIdx.x;
  const int i = b.origin0 + lane;
  const bool active = i < b.n;
  const double* pos = a.pos + 3 * b.node0;
  const double* steps = a.steps + b.node0;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (active) { px = pos[3 * (size_t)i]; py = pos[3 * (size_t)i + 1]; pz = pos[3 * (size_t)i + 2]; }
  const bool mini = a.mode == 1;
  double trav = 0.0, best = DBL_MAX, best_eucl = 0.0, best_trav = 0.0;
  int to = -1, exhausted = 0;
  bool done = !active;
  // the first node any lane needs is origin0 + 1
  for (int t0 = (b.origin0 + 1) / kClosureTile * kClosureTile; t0 < b.n; t0 += kClosureTile) {
    const int cnt = min(kClosureTile, b.n - t0);
    for (int k = lane; k < kClosureTile; k += kClosureOrigins) {
      const int j = t0 + k;
      // the padding of the last tile is never a candidate (j >= n is masked below); zeros keep its arithmetic finite
      double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
      if (k < cnt) v = make_double4(pos[3 * (size_t)j], pos[3 * (size_t)j + 1], pos[3 * (size_t)j + 2], j > 0 ? steps[j - 1] : 0.0);
      tile[k] = v;
    }
    __syncthreads();
    for (int k0 = max(0, b.origin0 + 1 - t0) / kClosureUnroll * kClosureUnroll; k0 < cnt; k0 += kClosureUnroll) {
#pragma unroll
      for (int u = 0; u < kClosureUnroll; u++) {
        const int j = t0 + k0 + u;
        const double4 q = tile[k0 + u];
        const bool live = !done && j > i && j < b.n;
        trav = live ? trav + q.w : trav;
        // MiniClosure asks `trav < min` first (:496-501): below min_d_travel an origin is never given up, whatever max says
        const bool past = live && trav > a.max_d_travel && !(mini && trav < a.min_d_travel);
        done = done || past;
        exhausted = past && mini ? 1 : exhausted;
        const double dx = px - q.x, dy = py - q.y, dz = pz - q.z;
        const double eucl = sqrt((dx * dx + dy * dy) + dz * dz);
        const double rel = eucl / trav;
        // GTVicinity: eucl <= close, min <= trav, trav <= max.  MiniClosure: !(trav < min), !(trav > max), eucl <= close.
        // With thresholds and trav that are not NaN the two read the same; `rel < best` keeps inf and NaN from winning.
        const bool win = live && !past && eucl <= a.max_d_close && a.min_d_travel <= trav && rel < best;
        best = win ? rel : best;
        best_eucl = win ? eucl : best_eucl;
        best_trav = win ? trav : best_trav;
        to = win ? j : to;
      }
      if (__ballot(!done) == 0) break;
    }
    if (__ballot(!done) == 0) break;
    __syncthreads();
  }
  if (active) {
    cfear_closure_candidate c;
    c.to = to;
    c.exhausted = exhausted;
    c.eucl = best_eucl;
    c.trav = best_trav;
    c.rel = to >= 0 ? best : 0.0;
    c.odom_bounds = 0.0;
    a.out[b.node0 + i] = c;
  }
}

// loopclosure::VerifyByOdometry(from = the later node, to = the origin): RelativeMotion(k, k + 1), k = origin .. to - 1
__global__ __launch_bounds__(kClosureOrigins) void closure_odom_kernel(const ClosureArgs a) {
  const ClosureBlock b = a.blocks[blockIdx.x];
  const int i = b.origin0 + (int)threadIdx.x;
  if (i >= b.n) return;
  cfear_closure_candidate* c = a.out + b.node0 + i;
  const int to = c->to;
  if (to < 0) return;
  if (!a.verify_via_odometry) { c->odom_bounds = 1.0; return; }
  c->odom_bounds = odom_chain_similarity(a.rel + 3 * b.node0, i, to, a.two_sigma2);
}

}  // namespace

extern "C" void cfear_closure_params_default(cfear_closure_params* p, int32_t mode) {
  if (!p) return;
  p->mode = mode;
  p->verify_via_odometry = 1;                  // loopclosure.h:122
  if (mode == CFEAR_CLOSURE_MINI) {            // MiniClosure::Parameters, loopclosure.h:95-97
    p->min_d_travel = 25.0; p->max_d_travel = 500.0; p->max_d_close = 15.0;
  } else {                                     // GTVicinityClosure::Parameters, loopclosure.h:84-86
    p->min_d_travel = 40.0; p->max_d_travel = 4200.0; p->max_d_close = 15.0;
  }
  p->odom_sigma_error = 0.03;                  // loopclosure.h:123
}

extern "C" int cfear_closure_candidates_batch(cfear_ctx* ctx, const double* positions, const double* steps, const double* rel_xyt,
                                              const int64_t* node_offsets, int64_t n_nodes, int32_t n_graphs,
                                              const cfear_closure_params* par, cfear_closure_candidate* out, int32_t* failed_graph) {
  if (failed_graph) *failed_graph = -1;
  // ---- everything is checked before anything is launched or written; the checks need no device ---------------------------
  if (n_graphs < 0 || n_nodes < 0 || !par || !node_offsets)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null or negative argument (node_offsets holds n_graphs + 1 entries)");
  if (n_nodes > 0 && (!positions || !steps || !out)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (cfear_is_device_ptr(positions) || cfear_is_device_ptr(steps) || cfear_is_device_ptr(rel_xyt) || cfear_is_device_ptr(out) ||
      cfear_is_device_ptr(node_offsets))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "all arrays must be host memory");
  if (par->mode != CFEAR_CLOSURE_GTVICINITY && par->mode != CFEAR_CLOSURE_MINI)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "unknown mode %d (0 GTVicinityClosure, 1 MiniClosure)", par->mode);
  if (std::isnan(par->min_d_travel) || std::isnan(par->max_d_travel) || std::isnan(par->max_d_close) ||
      (par->verify_via_odometry && rel_xyt && std::isnan(par->odom_sigma_error)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "a threshold is NaN");
  const OffsetsReport table = check_offsets(node_offsets, n_graphs, n_nodes);
  if (table.start_not_0 || table.end_not_total) {
    // the start and the end before the ranges; the graph whose range the table mis-states: the first if it does not start
    // at 0, else the last
    const int gi = n_graphs > 0 ? (table.start_not_0 ? 0 : n_graphs - 1) : -1;
    if (failed_graph) *failed_graph = gi;
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: node_offsets must run from 0 to n_nodes over n_graphs + 1 entries", gi);
  }
  int64_t n_blocks = 0;
  for (int gi = 0; gi < n_graphs; gi++) {
    const int64_t n = node_offsets[gi + 1] - node_offsets[gi];
    if (gi == table.bad_range() || n > INT32_MAX - kClosureTile) {
      if (failed_graph) *failed_graph = gi;
      return cfear_set_error(ctx, n > 0 ? CFEAR_ERR_CAPACITY : CFEAR_ERR_INVALID_ARGUMENT,
                             "graph %d: offsets descend or leave the arrays, or more than %d nodes", gi, INT32_MAX - kClosureTile);
    }
    n_blocks += (n + kClosureOrigins - 1) / kClosureOrigins;
  }
  for (int gi = 0; gi < n_graphs; gi++) {
    const int64_t n0 = node_offsets[gi], n = node_offsets[gi + 1] - n0;
    const char* what = nullptr;
    int64_t at = 0;
    for (int64_t k = 0; k < n && !what; k++) {
      const double* p = positions + 3 * (n0 + k);
      if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) { what = "a position that is not finite"; at = k; }
      else if (k + 1 < n && !(steps[n0 + k] >= 0.0 && std::isfinite(steps[n0 + k]))) { what = "a step that is negative or not finite"; at = k; }
    }
    if (what) {
      if (failed_graph) *failed_graph = gi;
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: %s at node %lld", gi, what, (long long)at);
    }
  }
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n_nodes == 0) return CFEAR_OK;
  if (n_blocks > INT32_MAX) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 x %d nodes in one call", kClosureOrigins);
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsClosure);
  ClosureArgs a{};
  char* d_tab;
  st.in(a.pos, positions, (size_t)n_nodes * 24);
  st.in(a.steps, steps, (size_t)n_nodes * 8);
  st.in(a.rel, rel_xyt, (size_t)n_nodes * 24);
  st.out(a.out, out, (size_t)n_nodes * sizeof(cfear_closure_candidate));
  const size_t tab_bytes = (size_t)n_blocks * sizeof(ClosureBlock);
  st.piece(d_tab, tab_bytes);
  CFEAR_CHECK(st.carve());
  ClosureBlock* hb = (ClosureBlock*)st.record(tab_bytes);
  int64_t nb = 0;
  for (int gi = 0; gi < n_graphs; gi++) {
    const int64_t n0 = node_offsets[gi], n = node_offsets[gi + 1] - n0;
    for (int64_t o = 0; o < n; o += kClosureOrigins) hb[nb++] = ClosureBlock{n0, (int32_t)n, (int32_t)o};
  }
  CFEAR_CHECK(st.upload(d_tab, hb, tab_bytes));
  a.blocks = (const ClosureBlock*)d_tab;
  a.mode = par->mode;
  a.verify_via_odometry = par->verify_via_odometry;
  a.min_d_travel = par->min_d_travel; a.max_d_travel = par->max_d_travel; a.max_d_close = par->max_d_close;
  a.two_sigma2 = 2.0 * par->odom_sigma_error * par->odom_sigma_error;
  {
    ProfScope ps(ctx, "closure_sweep");
    hipLaunchKernelGGL(closure_sweep_kernel, dim3((unsigned)n_blocks), dim3(kClosureOrigins), 0, ctx->stream, a);
  }
  if (rel_xyt) {
    ProfScope ps(ctx, "closure_odom");
    hipLaunchKernelGGL(closure_odom_kernel, dim3((unsigned)n_blocks), dim3(kClosureOrigins), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  CFEAR_CHECK(st.finish());
  return CFEAR_OK;
}
