// graphfinish.hip -- what every run of the reference's SLAM executables ends in (tbv_slam/src/tbv_slam_offline.cpp:248-266),
// for a batch of pose graphs: PoseGraph::Align, SaveGraphString and OutputGraph, and the two maps PoseGraphVis::ProcessFrame
// builds (tbv_slam/src/tbv_slam/posegraph.cpp, cited below as :line).  DESIGN.md section 4.17.  The batch layout is
// cfear_pgo_solve_batch's: flat per-node arrays and node_offsets [n_graphs + 1].
//
// cfear_graph_align_batch (:235-263).  Everything is fp64 without contraction (-ffp-contract=off):
//   graph_align_sums     workgroup per graph   the centroids of Tgt.p and T.p over the nodes with ground truth and
//                                              H^T = sum (b - cB)(a - cA)^T of best_fit_transform (cfear_radarodometry/src/
//                                              cfear_radarodometry/eval_trajectory.cpp:343-395): align_sums (pose_rows.hpp),
//                                              the body eval_align_sums runs
//   host                                       the evaluator's 3 x 3 SVD (cfear_align_from_sums, evaluate.hip) and the general
//                                              inverse of [R | t] (affine_inverse, pose_rows.hpp)
//   graph_align_apply    thread per node       PoseEigToCeres(Tgtalign * GetPose()) (types.cpp:25-38), eigen_quat.hpp
//   graph_align_ate      workgroup per graph   sum |Tgt.p - p_new| / max(N, 1) over the nodes with ground truth (a mean)
// A graph's sums depend on the graph alone, so its result does not depend on what else the batch holds.
//
// cfear_graph_map_batch (:539-584).  The point ranges follow from the offsets, so the host computes them, writes the summaries
// and builds two tables: a record per selected node with a non-empty cloud (source, destinations, count) and an entry per
// output tile of kMapTile points (its node record, its first point).  graph_map_kernel is one grid over the tiles: threads 0
// and 1 form the node's two 3 x 4 matrices from the quaternions (toRotationMatrix) into LDS, every thread moves one point --
// one 16-byte load, pcl::transformPointCloud<PointXYZI, double>'s float(((m0 x + m1 y) + m2 z) + m3) per row and map, one or
// two 16-byte stores.  A source point is read once for both maps; the kernel moves 32 or 48 bytes per point.
//
// cfear_graph_string_write / cfear_graph_output_write: the two host writers (:177-187, :201-234), no context.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <vector>

#include "pose_rows.hpp"

namespace {
constexpr int kGfThreads = kAlignThreads;
constexpr int kMapTile = CFEAR_GRAPH_MAP_TILE;
static_assert(kMapTile == kGfThreads, "one thread moves one point of a tile");
static_assert(sizeof(cfear_pose3d) == 56, "cfear_pose3d is 7 doubles (include/cfear_hip.h)");
static_assert(sizeof(cfear_graph_align_summary) == 112, "cfear_graph_align_summary is 112 bytes (include/cfear_hip.h)");
static_assert(sizeof(cfear_graph_map_summary) == 32 && sizeof(cfear_graph_map_params) == 8, "include/cfear_hip.h");

struct GfGraph { int64_t first; int32_t n, pad; };         // a graph's nodes in the flat arrays
struct GfPost {                                            // what the host adds between the two halves of the align call
  double align[12];                                        // Tgtalign
  int32_t apply, pad;                                      // 0: the graph's poses stay as they are (CFEAR_ERR_SOLVER)
};
struct GfAlignArgs {
  const GfGraph* graphs;
  const GfPost* post;
  const int2* blocks;          // graph_align_apply: (graph, first node of the graph) of every workgroup
  cfear_pose3d* poses;
  const cfear_pose3d* gt;
  const uint8_t* has_gt;
  double* sums;                // [n_graphs][16]: cA (3), cB (3), sum (b - cB)(a - cA)^T row-major (9), the nodes with ground truth
  double* ate;                 // [n_graphs]
};

struct GfMapNode {             // a selected node with at least one point
  int64_t src;                 // first point in xyzi
  int64_t dst;                 // first point in map
  int64_t dst_gt;              // first point in map_gt, -1: none (no ground truth, or no ground-truth map wanted)
  int32_t n, node;             // points; the node in the flat arrays
};
struct GfMapArgs {
  const GfMapNode* nodes;
  const int2* tiles;           // (node record, first point of the tile within the node)
  const cfear_pose3d* poses;
  const cfear_pose3d* gt;
  const float* xyzi;
  float* map;
  float* map_gt;
};

__device__ __forceinline__ cfear_pose3d pose3d_load(const cfear_pose3d* at) {
  cfear_pose3d r;
  const double* d = (const double*)at;
#pragma unroll
  for (int k = 0; k < 3; k++) r.p[k] = gload<double>(d + k);
#pragma unroll
  for (int k = 0; k < 4; k++) r.q[k] = gload<double>(d + 3 + k);
  return r;
}

// best_fit_transform(A = Tgt.p, B = T.p), eval_trajectory.cpp:343-368, in the layout cfear_align_from_sums reads: x = A, y = B
struct GfAlignSrc {
  static constexpr bool kSkips = true;
  const cfear_pose3d *T, *G;
  const uint8_t* has;
  int n;
  __device__ bool counts(int i) const { return has[i] != 0; }
  __device__ double x(int i, int k) const { return gload<double>((const double*)(G + i) + k); }
  __device__ double y(int i, int k) const { return gload<double>((const double*)(T + i) + k); }
  __device__ double mean_div(double n_gt) const { return fmax(n_gt, 1.0); }   // std::max(row, 1), :361
  __device__ double cov(double sum) const { return sum; }                     // H = AA^T BB is not divided by the rows (:368)
};
__global__ __launch_bounds__(kGfThreads) void graph_align_sums_kernel(GfAlignArgs a) {
  __shared__ double red[4];
  const GfGraph g = a.graphs[blockIdx.x];
  align_sums(GfAlignSrc{a.poses + g.first, a.gt + g.first, a.has_gt + g.first, g.n}, a.sums + (size_t)blockIdx.x * 16, red);
}

// itr->second.T = PoseEigToCeres(Tgtalign * itr->second.GetPose()), :252
__global__ __launch_bounds__(kGfThreads) void graph_align_apply_kernel(GfAlignArgs a) {
  const int2 blk = a.blocks[blockIdx.x];
  const GfGraph g = a.graphs[blk.x];
  const int i = blk.y + threadIdx.x;
  if (i >= g.n) return;
  const GfPost& post = a.post[blk.x];
  if (!post.apply) return;
  Pose A, B;
  double q[4];
#pragma unroll
  for (int k = 0; k < 12; k++) A.m[k] = post.align[k];
  cfear_pose3d* at = a.poses + g.first + i;
  pose3d_to_rows(pose3d_load(at), B.m);
  const Pose R = pose_mul(A, B);
  quat_from_rows(R.m, q);
  // Quaternion::normalize(): coeffs() /= norm(), the squared norm a 2-wide packet reduction, (xx + zz) + (yy + ww)
  const double norm = __dsqrt_rn((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]));
  double* d = (double*)at;
  gstore<double>(d + 0, R.m[3]); gstore<double>(d + 1, R.m[7]); gstore<double>(d + 2, R.m[11]);
#pragma unroll
  for (int k = 0; k < 4; k++) gstore<double>(d + 3 + k, q[k] / norm);
}

// d += (Tgt.p - GetPose().translation()).norm(); d / std::max(N, 1), :254-262
__global__ __launch_bounds__(kGfThreads) void graph_align_ate_kernel(GfAlignArgs a) {
  __shared__ double red[4];
  const GfGraph g = a.graphs[blockIdx.x];
  const cfear_pose3d* T = a.poses + g.first;
  const cfear_pose3d* G = a.gt + g.first;
  const uint8_t* has = a.has_gt + g.first;
  double s = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < g.n; i += kGfThreads) {
    if (!has[i]) continue;
    cnt += 1.0;
    const double* pg = (const double*)(G + i);
    const double* pt = (const double*)(T + i);
    s += norm3(gload<double>(pg) - gload<double>(pt), gload<double>(pg + 1) - gload<double>(pt + 1), gload<double>(pg + 2) - gload<double>(pt + 2));
  }
  const double n_gt = block_sum(cnt, red);
  const double ate = block_sum(s, red) / fmax(n_gt, 1.0);
  if (threadIdx.x == 0) a.ate[blockIdx.x] = ate;
}

// pcl::transformPointCloud<PointXYZI, double> (PCL 1.10 common/impl/transforms.hpp): float(((m0 x + m1 y) + m2 z) + m3)
__device__ __forceinline__ g_f32x4 tf_point(const double* m, const g_f32x4 p) {
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  g_f32x4 o;
  o.x = (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
  o.y = (float)(((m[4] * x + m[5] * y) + m[6] * z) + m[7]);
  o.z = (float)(((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
  o.w = p.w;
  return o;
}

__global__ __launch_bounds__(kGfThreads) void graph_map_kernel(GfMapArgs a) {
  __shared__ double M[2][12];
  const int2 tile = a.tiles[blockIdx.x];
  const GfMapNode rec = a.nodes[tile.x];
  const bool with_gt = rec.dst_gt >= 0;
  if (threadIdx.x == 0) pose3d_to_rows(pose3d_load(a.poses + rec.node), M[0]);
  if (threadIdx.x == 1 && with_gt) pose3d_to_rows(pose3d_load(a.gt + rec.node), M[1]);
  __syncthreads();
  const int i = tile.y + (int)threadIdx.x;
  if (i >= rec.n) return;
  const g_f32x4 p = gload<g_f32x4>(a.xyzi + (rec.src + i) * 4);
  gstore<g_f32x4>(a.map + (rec.dst + i) * 4, tf_point(M[0], p));
  if (with_gt) gstore<g_f32x4>(a.map_gt + (rec.dst_gt + i) * 4, tf_point(M[1], p));
}

// MatToString (types.cpp:64-73) of PoseCeresToEig(p).matrix()
bool write_pose_row(FILE* f, const cfear_pose3d& p, const char* end) {
  double m[12];
  pose3d_to_rows(p, m);
  return kitti_row_write(f, m, end);
}
}  // namespace

extern "C" int cfear_graph_align_batch(cfear_ctx* ctx, cfear_pose3d* poses, const cfear_pose3d* gt, const uint8_t* has_gt,
                                       const int64_t* node_offsets, int64_t n_nodes, int32_t n_graphs,
                                       cfear_graph_align_summary* summaries) {
  if (n_graphs < 0 || n_nodes < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "negative count");
  if (!node_offsets || (n_graphs > 0 && !summaries) || (n_nodes > 0 && (!poses || !gt || !has_gt)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (cfear_is_device_ptr(node_offsets) || cfear_is_device_ptr(summaries))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node_offsets and summaries must be host memory");
  if (!check_offsets(node_offsets, n_graphs, n_nodes).fine())
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node_offsets must run from 0 to n_nodes without descending");
  const int kind = n_nodes ? memory_kind({poses, gt, has_gt}) : 0;
  if (kind < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "poses, gt and has_gt must be all host or all device memory");
  if (kind == 1 && (((uintptr_t)poses | (uintptr_t)gt) & 7))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "device poses must be 8-byte aligned");
  std::vector<GfGraph> graphs((size_t)n_graphs);
  std::vector<int2> blocks;
  bool grid_ok = true;
  for (int g = 0; g < n_graphs; g++) {
    const int64_t n = node_offsets[g + 1] - node_offsets[g];
    if (n > INT32_MAX - kGfThreads) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "graph %d holds more than 2^31 nodes", g);
    graphs[g] = GfGraph{node_offsets[g], (int32_t)n, 0};
    grid_ok = flat_grid_add(blocks, g, n, kGfThreads) && grid_ok;
  }
  if (!grid_ok) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 x 256 nodes in one call");
  if (!ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null context");
  if (n_graphs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsGraphFinish);
  GfAlignArgs a{};
  st.in(a.poses, poses, (size_t)n_nodes * sizeof(cfear_pose3d), true);
  st.in(a.gt, gt, (size_t)n_nodes * sizeof(cfear_pose3d));
  st.in(a.has_gt, has_gt, (size_t)n_nodes);
  StagedTables tab(st, (size_t)n_graphs * sizeof(GfGraph), blocks.size() * sizeof(int2), (size_t)n_graphs * sizeof(GfPost));
  st.piece(a.sums, (size_t)n_graphs * 16 * 8);
  st.piece(a.ate, (size_t)n_graphs * 8);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(tab.upload(graphs.data(), blocks.data()));
  a.graphs = tab.records<GfGraph>();
  a.blocks = tab.blocks<int2>();
  a.post = tab.second<GfPost>();
  {
    ProfScope ps(ctx, "graph_align_sums");
    hipLaunchKernelGGL(graph_align_sums_kernel, dim3(n_graphs), dim3(kGfThreads), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  std::vector<double> h_sums((size_t)n_graphs * 16), h_ate((size_t)n_graphs);
  st.fetch(h_sums.data(), a.sums, h_sums.size() * 8);
  CFEAR_CHECK(st.wait());
  // host half: best_fit_transform's SVD (:376-393) and the inverse of :249
  GfPost* post = tab.host_second<GfPost>();
  std::vector<int32_t> status((size_t)n_graphs, CFEAR_OK);
  for (int g = 0; g < n_graphs; g++) {
    const double* s = h_sums.data() + (size_t)g * 16;
    double fit[12];
    bool zero = true;
    for (int k = 0; k < 9; k++) zero = zero && s[6 + k] == 0.0;
    // JacobiSVD of a zero H returns identities: R = I, t = cB - cA, which is what the routine leaves when it finds no rotation
    const bool ok = cfear_align_from_sums(s, fit) || zero;
    bool finite = true;
    if (ok) {
      affine_inverse(fit, post[g].align);
      for (int k = 0; k < 12; k++) finite = finite && std::isfinite(post[g].align[k]);
    }
    post[g].apply = ok && finite;
    post[g].pad = 0;
    if (!post[g].apply) {
      memcpy(post[g].align, kIdentityRows, sizeof(kIdentityRows));
      status[g] = CFEAR_ERR_SOLVER;
    }
  }
  CFEAR_CHECK(tab.upload_second());
  if (!blocks.empty()) {
    ProfScope ps(ctx, "graph_align_apply");
    hipLaunchKernelGGL(graph_align_apply_kernel, dim3((unsigned)blocks.size()), dim3(kGfThreads), 0, ctx->stream, a);
  }
  {
    ProfScope ps(ctx, "graph_align_ate");
    hipLaunchKernelGGL(graph_align_ate_kernel, dim3(n_graphs), dim3(kGfThreads), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  st.fetch(h_ate.data(), a.ate, h_ate.size() * 8);
  CFEAR_CHECK(st.finish());
  for (int g = 0; g < n_graphs; g++) {
    memcpy(summaries[g].align, post[g].align, sizeof(post[g].align));
    summaries[g].ate = h_ate[g];
    summaries[g].n_gt = (int32_t)h_sums[(size_t)g * 16 + 15];
    summaries[g].status = status[g];
  }
  return CFEAR_OK;
}

extern "C" int cfear_graph_map_batch(cfear_ctx* ctx, const cfear_pose3d* poses, const cfear_pose3d* gt, const uint8_t* has_gt,
                                     const int64_t* node_offsets, int64_t n_nodes, int32_t n_graphs, const float* xyzi,
                                     const int64_t* cloud_offsets, int64_t n_points, const cfear_graph_map_params* par, float* map,
                                     int64_t map_cap, float* map_gt, int64_t map_gt_cap, cfear_graph_map_summary* summaries) {
  if (!par || par->skip_frames < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "skip_frames must be at least 1");
  if (n_graphs < 0 || n_nodes < 0 || n_points < 0 || map_cap < 0 || map_gt_cap < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "negative count");
  const bool want_gt = par->want_gt_map != 0;
  if (!node_offsets || !cloud_offsets || (n_graphs > 0 && !summaries) || (n_nodes > 0 && (!poses || (want_gt && (!gt || !has_gt)))) ||
      (n_points > 0 && !xyzi) || (map_cap > 0 && !map) || (want_gt && map_gt_cap > 0 && !map_gt))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (cfear_is_device_ptr(node_offsets) || cfear_is_device_ptr(cloud_offsets) || cfear_is_device_ptr(summaries))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node_offsets, cloud_offsets and summaries must be host memory");
  if (!check_offsets(node_offsets, n_graphs, n_nodes).fine())
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node_offsets must run from 0 to n_nodes without descending");
  if (!check_offsets(cloud_offsets, n_nodes, n_points).fine())
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cloud_offsets must run from 0 to n_points without descending");
  const int in_kind = memory_kind({n_nodes ? poses : nullptr, n_nodes && want_gt ? gt : nullptr, n_nodes && want_gt ? has_gt : nullptr,
                                   n_points ? xyzi : nullptr});
  const int out_kind = memory_kind({map_cap ? map : nullptr, want_gt && map_gt_cap ? map_gt : nullptr});
  if (in_kind < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "poses, gt, has_gt and xyzi must be all host or all device memory");
  if (out_kind < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "map and map_gt must both be host or both be device memory");
  if ((in_kind == 1 && ((((uintptr_t)poses | (uintptr_t)gt) & 7) || ((uintptr_t)xyzi & 15))) ||
      (out_kind == 1 && (((uintptr_t)map | (uintptr_t)(want_gt ? map_gt : nullptr)) & 15)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "device poses must be 8-byte aligned, device clouds and maps 16-byte aligned");
  if (n_nodes > INT32_MAX) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 nodes in one call");
  if (!ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null context");
  if (n_graphs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  // the flags decide the ground-truth ranges: device flags are read back first
  std::vector<uint8_t> h_has;
  if (want_gt && n_nodes > 0 && in_kind == 1) {
    h_has.resize((size_t)n_nodes);
    HostStage pre(ctx, kWsGraphFinish);
    pre.fetch(h_has.data(), has_gt, (size_t)n_nodes);
    CFEAR_CHECK(pre.wait());
    has_gt = h_has.data();
  }
  // ---- the ranges, the node records and the tile table: host arithmetic on the offsets -----------------------------------
  std::vector<GfMapNode> nodes;
  std::vector<int2> tiles;
  int64_t total = 0, total_gt = 0;
  bool too_many = false;
  for (int g = 0; g < n_graphs; g++) {
    cfear_graph_map_summary& s = summaries[g];
    s.map_offset = total;
    s.map_gt_offset = total_gt;
    for (int64_t k = node_offsets[g]; k < node_offsets[g + 1]; k += par->skip_frames) {   // ordinal % skip_frames == 0, :573
      const int64_t n = cloud_offsets[k + 1] - cloud_offsets[k];
      if (n > INT32_MAX - kMapTile) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "node %lld holds more than 2^31 points", (long long)k);
      const bool with_gt = want_gt && has_gt[k];
      if (n > 0 && !too_many) {
        too_many = !flat_grid_add(tiles, (int32_t)nodes.size(), n, kMapTile);
        nodes.push_back(GfMapNode{cloud_offsets[k], total, with_gt ? total_gt : -1, (int32_t)n, (int32_t)k});
      }
      total += n;
      if (with_gt) total_gt += n;
    }
    s.map_points = total - s.map_offset;
    s.map_gt_points = total_gt - s.map_gt_offset;
  }
  if (total > map_cap || (want_gt && total_gt > map_gt_cap))
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "the maps hold %lld and %lld points, the buffers %lld and %lld (the summaries are complete)",
                           (long long)total, (long long)(want_gt ? total_gt : 0), (long long)map_cap, (long long)(want_gt ? map_gt_cap : 0));
  if (too_many) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "more than 2^31 tiles in one call");
  if (total == 0) return CFEAR_OK;
  HostStage st(ctx, kWsGraphFinish);
  GfMapArgs a{};
  st.in(a.poses, poses, (size_t)n_nodes * sizeof(cfear_pose3d));
  if (want_gt) st.in(a.gt, gt, (size_t)n_nodes * sizeof(cfear_pose3d));
  st.in(a.xyzi, xyzi, (size_t)n_points * 16);
  st.out(a.map, map, (size_t)total * 16);
  if (want_gt && total_gt > 0) st.out(a.map_gt, map_gt, (size_t)total_gt * 16);
  // megabytes at a realistic size: staged in pinned memory
  StagedTables tab(st, nodes.size() * sizeof(GfMapNode), tiles.size() * sizeof(int2), 0, true);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(tab.upload(nodes.data(), tiles.data()));
  a.nodes = tab.records<GfMapNode>();
  a.tiles = tab.blocks<int2>();
  {
    ProfScope ps(ctx, "graph_map");
    hipLaunchKernelGGL(graph_map_kernel, dim3((unsigned)tiles.size()), dim3(kGfThreads), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}

// ---- host writers, no context -----------------------------------------------------------------------------------------
// PoseGraph::SaveGraphString, :177-187: RadarScan::ToString (types.cpp:93-102) ends its line itself and the loop adds an endl
extern "C" int cfear_graph_string_write(const char* path, const cfear_pose3d* poses, const uint64_t* stamps, int64_t n) {
  if (!path || n < 0 || (n > 0 && (!poses || !stamps))) return CFEAR_ERR_INVALID_ARGUMENT;
  FILE* f = fopen(path, "w");
  if (!f) return CFEAR_ERR_IO;
  bool ok = true;
  for (int64_t i = 0; i < n && ok; i++) ok = write_pose_row(f, poses[i], " ") && fprintf(f, "%" PRIu64 "\n\n", stamps[i]) > 0;
  ok = fclose(f) == 0 && ok;
  return ok ? CFEAR_OK : CFEAR_ERR_IO;
}

// PoseGraph::OutputGraph, :201-234
extern "C" int cfear_graph_output_write(const char* est_path, const char* gt_path, const cfear_pose3d* poses, const cfear_pose3d* gt,
                                        const uint8_t* has_gt, int64_t n) {
  if (!est_path || !gt_path || n < 0 || (n > 0 && !poses)) return CFEAR_ERR_INVALID_ARGUMENT;
  bool gt_found = false;
  for (int64_t i = 0; i < n && has_gt && !gt_found; i++) gt_found = has_gt[i] != 0;
  if (gt_found && !gt) return CFEAR_ERR_INVALID_ARGUMENT;
  FILE* fe = fopen(est_path, "w");
  if (!fe) return CFEAR_ERR_IO;
  FILE* fg = fopen(gt_path, "w");
  if (!fg) { fclose(fe); return CFEAR_ERR_IO; }
  bool ok = true;
  for (int64_t i = 0; i < n && ok; i++) {
    if (gt_found && !has_gt[i]) continue;
    ok = write_pose_row(fe, poses[i], "\n");
    if (gt_found && ok) ok = write_pose_row(fg, gt[i], "\n");
  }
  ok = fclose(fe) == 0 && ok;
  ok = fclose(fg) == 0 && ok;
  return ok ? CFEAR_OK : CFEAR_ERR_IO;
}
