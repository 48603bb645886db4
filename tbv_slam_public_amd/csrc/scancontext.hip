// scancontext.hip -- radar Scan Context descriptors and their column-shift distance on gfx950.
//
// Replaces (place_recognition_radar/src/place_recognition_radar/):
//   RSCManager::MakeRadarCloudContext (+ the 4 lateral augmentations)   RadarScancontext.cpp:59-131, 156-180
//   makeRingkeyFromScancontext / makeSectorkeyFromScancontext           Scancontext.cpp:239-268
//   distanceBtnScanContext = fastAlignUsingVkey + distDirectSC + circshift   Scancontext.cpp:80-189
// i.e. the arithmetic of the step BEFORE the registration path (loop-candidate generation).
// The database, the odometry-coupled key search and the candidate ranking (RadarScancontext.cpp:181-345)
// are host policy and live in the caller (tbv_slam_public_amd/api.py RSCManager mirrors them).
//
// sc_descriptor_kernel: one workgroup per (cloud, augmentation); the ring x sector accumulator lives in LDS
//   (fp64 sum + hit count, or order-preserving integer max); ceil-indexed polar binning with the reference's
//   float arithmetic; the "division before the NO_POINT check" quirk is kept (empty bins hold -1000 / divider
//   unless the divider is 1).  Intensities of radar clouds are integer valued, so the LDS fp64 atomics sum
//   exactly and the result does not depend on the order of arrival.
// sc_distance_kernel: one workgroup per (query, candidate) pair; both descriptors in LDS (2 x 38 KiB at
//   40 x 120); one thread per column / per shift, every inner sum sequential in the reference's order, so
//   distances and argmin shifts are bit-identical with the CPU restatement.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kScMaxCells = 5120;        // ring x sector capacity of the LDS accumulators (reference: 40 x 120)
constexpr int kScDistThreads = 1024;     // one distance workgroup per CU (two descriptors = 77 KB of LDS): wide blocks
constexpr int kScMaxAug = 8;

struct ScCloud { const float4* xyzi; int32_t n; int32_t pad; };
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct ScDescArgs {
  const ScCloud* clouds;
  int num_ring, num_sector, desc_function, n_aug;
  double max_radius, desc_divider, no_point;
  double shift_y[kScMaxAug];
  double* desc;          // [n_clouds][n_aug][R * S]
  double* ringkey;       // [n_clouds][n_aug][R]
  double* sectorkey;     // [n_clouds][n_aug][S]
};

// Scancontext.cpp:60-76; the reference calls the float overload of atan: the correctly rounded float
// arctangent is taken from the fp64 routine
__device__ __forceinline__ float sc_xy2theta(float x, float y) {
  auto atan_f = [](float v) { return (float)atan((double)v); };
  if ((x >= 0) & (y >= 0)) return (float)((180 / M_PI) * atan_f(y / x));
  if ((x < 0) & (y >= 0)) return (float)(180 - ((180 / M_PI) * atan_f(y / (-x))));
  if ((x < 0) & (y < 0)) return (float)(180 + ((180 / M_PI) * atan_f(y / x)));
  if ((x >= 0) & (y < 0)) return (float)(360 - ((180 / M_PI) * atan_f((-y) / x)));
  return 0;
}

// makeRingkeyFromScancontext / makeSectorkeyFromScancontext (Scancontext.cpp:239-268) of one descriptor d [R][S], by the
// whole workgroup; sk may be null
__device__ __forceinline__ void sc_keys(const double* d, int R, int S, double* rk, double* sk) {
  for (int r = threadIdx.x; r < R; r += blockDim.x) {  // row means, sequential like Eigen's row.mean() restatement
    double s = 0;
    for (int c = 0; c < S; c++) s += d[r * S + c];
    rk[r] = s / S;
  }
  if (!sk) return;
  for (int c = threadIdx.x; c < S; c += blockDim.x) {
    double s = 0;
    for (int r = 0; r < R; r++) s += d[r * S + c];
    sk[c] = s / R;
  }
}

// The LDS accumulator of one descriptor, shared by sc_descriptor_kernel and sc_local_map_kernel: acc [cells] fp64 sums,
// hit [cells] hit counts (sum) or the order-preserving int image of the float maximum (max).
struct ScBin {
  int num_ring, num_sector, desc_function;
  double max_radius, desc_divider, no_point;
};

__device__ __forceinline__ void sc_acc_clear(double* acc, int* hit, const ScBin& b) {
  const int cells = b.num_ring * b.num_sector;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) { acc[i] = 0.0; hit[i] = b.desc_function == 0 ? 0 : (int)0x80000000; }
}

// one point: the lateral augmentation, then the ceil-indexed polar binning (MakeRadarCloudContext)
__device__ __forceinline__ void sc_acc_point(double* acc, int* hit, const float4 p, double shift_y, const ScBin& b) {
  const int R = b.num_ring, S = b.num_sector;
  float px = p.x, py = p.y;
  if (shift_y != 0.0) {                              // pcl::transformPointCloud with an identity rotation (:163-170)
    px = (float)(((1.0 * (double)p.x + 0.0 * (double)p.y) + 0.0 * (double)p.z) + 0.0);
    py = (float)(((0.0 * (double)p.x + 1.0 * (double)p.y) + 0.0 * (double)p.z) + shift_y);
  }
  const float azim_range = sqrtf(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)));
  const float azim_angle = sc_xy2theta(px, py);
  if ((double)azim_range > b.max_radius) return;
  const double rr = ceil(((double)azim_range / b.max_radius) * R), ss = ceil(((double)azim_angle / 360.0) * S);
  const int ring_idx = max(min(R, rr == rr ? (int)rr : 1), 1);
  const int sctor_idx = max(min(S, ss == ss ? (int)ss : 1), 1);
  const int cell = (ring_idx - 1) * S + (sctor_idx - 1);
  if (b.desc_function == 0) {
    atomicAdd(&acc[cell], (double)p.w);
    atomicAdd(&hit[cell], 1);
  } else {                                           // max: order-preserving int image of the float intensity
    int u = __float_as_int(p.w);
    u = u >= 0 ? u : (u ^ 0x7fffffff);
    atomicMax(&hit[cell], u);
  }
}

// the finished descriptor, into acc (for the keys) and out
__device__ __forceinline__ void sc_acc_finish(double* acc, const int* hit, const ScBin& b, double* out) {
  const int cells = b.num_ring * b.num_sector;
  const int NO_POINT = -1000;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    double d;
    if (b.desc_function == 0) d = hit[i] > 0 ? acc[i] : (double)NO_POINT;
    else {
      const int u = hit[i];
      d = u == (int)0x80000000 ? (double)NO_POINT : (double)__int_as_float(u >= 0 ? u : (u ^ 0x7fffffff));
    }
    d = d / b.desc_divider;                          // "Divison before no_point check" (:113)
    if (d == NO_POINT) d = b.no_point;
    acc[i] = d;
    out[i] = d;
  }
}

__global__ __launch_bounds__(256) void sc_descriptor_kernel(const ScDescArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const ScBin b{a.num_ring, a.num_sector, a.desc_function, a.max_radius, a.desc_divider, a.no_point};
  const int R = a.num_ring, S = a.num_sector, cells = R * S;
  double* acc = (double*)smem;                       // [cells] sum
  int* hit = (int*)(acc + cells);                    // [cells] count (sum) / float-ordered max (max)
  const ScCloud cl = a.clouds[blockIdx.x];
  const double shift_y = a.shift_y[blockIdx.y];
  sc_acc_clear(acc, hit, b);
  __syncthreads();
  for (int k = threadIdx.x; k < cl.n; k += blockDim.x) sc_acc_point(acc, hit, cl.xyzi[k], shift_y, b);
  __syncthreads();
  sc_acc_finish(acc, hit, b, a.desc + ((size_t)blockIdx.x * a.n_aug + blockIdx.y) * cells);
  __syncthreads();
  sc_keys(acc, R, S, a.ringkey + ((size_t)blockIdx.x * a.n_aug + blockIdx.y) * R,
          a.sectorkey + ((size_t)blockIdx.x * a.n_aug + blockIdx.y) * S);
}

// ---- whole-graph Scan Context ------------------------------------------------------------------
// sc_local_map_kernel: one workgroup per (centre node, augmentation).  ScansToLocalMap (loopclosure.cpp:553-569) + the
// descriptor: every point of every member node goes to the world frame and back into the centre's frame with
// pcl::transformPointCloud's arithmetic (double products, summed left to right, rounded to float; z and the intensity are
// carried), then into the same LDS accumulator as sc_descriptor_kernel.
struct ScMapNode {
  const float4* xyzi;
  int32_t n, pad;
  double T[8], Tinv[8];              // rows 0 and 1 of node -> world and world -> node
};

struct ScMapArgs {
  const ScMapNode* nodes;
  const int32_t* center;             // [n_centers] node index
  const int2* members;               // [n_centers] first / last member node index
  ScBin bin;
  int n_aug;
  double shift_y[kScMaxAug];
  double* desc;                      // [n_centers][n_aug][R * S]
  double* db;                        // optional: augmentation 0 also to db [n_centers][R * S]
  double* ringkey;                   // [n_centers][n_aug][R]
  double* sectorkey;                 // optional [n_centers][n_aug][S]
};

__device__ __forceinline__ float sc_affine_row(const double* m, float x, float y, float z) {
  return (float)(((m[0] * (double)x + m[1] * (double)y) + m[2] * (double)z) + m[3]);
}

__global__ __launch_bounds__(256) void sc_local_map_kernel(const ScMapArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int R = a.bin.num_ring, S = a.bin.num_sector, cells = R * S;
  double* acc = (double*)smem;
  int* hit = (int*)(acc + cells);
  const int c = blockIdx.x, k = blockIdx.y;
  const double* Ti = a.nodes[a.center[c]].Tinv;
  const double shift_y = a.shift_y[k];
  const int2 mem = a.members[c];
  sc_acc_clear(acc, hit, a.bin);
  __syncthreads();
  for (int j = mem.x; j <= mem.y; j++) {
    const ScMapNode& m = a.nodes[j];
    for (int i = threadIdx.x; i < m.n; i += blockDim.x) {
      const float4 p = m.xyzi[i];
      const float wx = sc_affine_row(m.T, p.x, p.y, p.z), wy = sc_affine_row(m.T + 4, p.x, p.y, p.z);
      const float4 q = make_float4(sc_affine_row(Ti, wx, wy, p.z), sc_affine_row(Ti + 4, wx, wy, p.z), p.z, p.w);
      sc_acc_point(acc, hit, q, shift_y, a.bin);
    }
  }
  __syncthreads();
  const size_t o = (size_t)c * a.n_aug + k;
  sc_acc_finish(acc, hit, a.bin, a.desc + o * cells);
  if (k == 0 && a.db)
    for (int i = threadIdx.x; i < cells; i += blockDim.x) a.db[(size_t)c * cells + i] = acc[i];
  __syncthreads();
  sc_keys(acc, R, S, a.ringkey + o * R, a.sectorkey ? a.sectorkey + o * S : nullptr);
}

// Odometry terms of ExcludeAndUpdateLikelihood (RadarScancontext.cpp:201-222) for the query nodes q0 .. q0 + nq - 1.
// sc_travel_kernel: one thread per query node i sums the segment lengths seg[m] = |p_{m+1} - p_m| from m = i - 1 downwards,
// in the reference's order; trav [s][nq] is the sum down to node i - 1 - s.
__global__ __launch_bounds__(256) void sc_travel_kernel(const double* seg, int q0, int nq, double* trav) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const int i = q0 + t;
  double s = 0.0;
  for (int m = i - 1; m >= 0; m--) {
    s += seg[m];
    trav[(size_t)(i - 1 - m) * nq + t] = s;
  }
}

// sc_odom_sim_kernel: odom_similarity[idx] = 1 - exp(-rel^2 / (2 sigma^2)), rel = max(|p_i - p_idx| - 5, 0) / trav, for every
// query node i and idx < i: sim [nq][ld]
__global__ __launch_bounds__(256) void sc_odom_sim_kernel(const double2* pos, const double* trav, int q0, int nq, int ld,
                                                          double sigma, double* sim) {
  const size_t n_items = (size_t)nq * (q0 + nq);
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < n_items; it += (size_t)gridDim.x * blockDim.x) {
    const int t = (int)(it % nq), s = (int)(it / nq);
    const int i = q0 + t, idx = i - 1 - s;
    if (idx < 0) continue;
    const double2 pi = pos[i], pj = pos[idx];
    const double est = hypot(pi.x - pj.x, pi.y - pj.y);
    const double e5 = est - 5.0;
    const double error = e5 < 0.0 ? 0.0 : e5;        // std::max(est - 5.0, 0.0)
    const double rel = error / trav[(size_t)s * nq + t];
    const double prob = exp(-rel * rel / (2 * sigma * sigma));
    sim[(size_t)t * ld + idx] = 1.0 - prob;
  }
}

// sc_keysearch_kernel: one workgroup per (query node, augmentation).  The ring-key search of detectLoopClosureID
// (RadarScancontext.cpp:225-284) over the eligible prefix [0, n_search): OdometryNNSearch's L2norm (float accumulator, double
// error terms, a 41st element 10 x odometry similarity) or VanillaKDNNSearch's L2_Adaptor (groups of four), and the
// k_sel smallest by (distance, index) -- the order std::stable_sort leaves.  Every thread keeps its own sorted k_sel best in
// LDS (it visits ascending indices, so equal distances stay in index order), then k_sel rounds of a workgroup minimum over the
// list heads pick the result.  Vanilla mode pads a short result with node 0 (the zero-initialised index vector).
constexpr int kScSearchThreads = 256;
constexpr int kScMaxTreeK = 64;

struct ScSearchArgs {
  const double* ringkey;             // [n_db][n_aug][R]: the database is augmentation 0
  const double* sim;                 // odometry mode: [nq][ld]
  const int32_t* n_search;           // [nq][n_aug] eligible prefix (odometry: max(i - 1 - exclude, 0); vanilla: the tree's size)
  const int32_t* pair_off;           // [nq][n_aug] first pair (of the whole call); -1: no search
  int pair_base;                     // first pair of the chunk
  int q0, ld, R, n_aug, k_sel, odometry;
  int32_t* pairs;                    // [.][2] (query (node - q0) * n_aug + k, database node)
  double* pair_sim;                  // odometry similarity of the pair's database node
};

__device__ __forceinline__ bool sc_key_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// One search by the whole workgroup, shared by sc_keysearch_kernel and sc_batch_keysearch_kernel.  dbkeys: the ring keys the
// query may see, [.][n_aug][R] from its database's node 0; qkey: the query's own key; srow: its odometry similarities by
// database index (odometry mode).  The n_out pairs go to `off`: (qi, db_base + database index).
__device__ __forceinline__ void sc_keysearch_body(const double* dbkeys, const double* qkey, const double* srow, int L, int K, int R,
                                                  int n_aug, int odometry, int off, int qi, int db_base, int32_t* pairs,
                                                  double* pair_sim) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* ld = (float*)smem;                          // [K][threads] distances of every thread's list
  int* li = (int*)(ld + (size_t)K * kScSearchThreads);   // [K][threads] indices
  float* qk = (float*)(li + (size_t)K * kScSearchThreads);   // [R + 1] query key
  float* rd = qk + R + 1;                            // [waves] per-wave minimum
  int* ri = (int*)(rd + kScSearchThreads / 64);
  for (int r = threadIdx.x; r < R; r += blockDim.x) qk[r] = (float)qkey[r];   // eig2stdvec
  __syncthreads();
  int cnt = 0;
  for (int idx = threadIdx.x; idx < L; idx += blockDim.x) {
    const double* kk = dbkeys + (size_t)idx * n_aug * R;
    float d = 0.f;
    if (odometry) {                                  // L2norm (:250-257)
      for (int r = 0; r < R; r++) {
        const double err = (double)(qk[r] - (float)kk[r]);
        d = (float)((double)d + err * err);
      }
      const double err = (double)(0.0f - (float)(10 * srow[idx]));
      d = (float)((double)d + err * err);
    } else {                                         // L2_Adaptor::evalMetric
      int r = 0;
      for (; r + 3 < R; r += 4) {
        const float e0 = qk[r] - (float)kk[r], e1 = qk[r + 1] - (float)kk[r + 1], e2 = qk[r + 2] - (float)kk[r + 2],
                    e3 = qk[r + 3] - (float)kk[r + 3];
        d += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
      }
      for (; r < R; r++) { const float e = qk[r] - (float)kk[r]; d += e * e; }
    }
    if (cnt == K && !(d < ld[(K - 1) * kScSearchThreads + threadIdx.x])) continue;
    int pos = cnt < K ? cnt : K - 1;                 // insert after every entry <= d (they have smaller indices)
    while (pos > 0 && d < ld[(pos - 1) * kScSearchThreads + threadIdx.x]) {
      ld[pos * kScSearchThreads + threadIdx.x] = ld[(pos - 1) * kScSearchThreads + threadIdx.x];
      li[pos * kScSearchThreads + threadIdx.x] = li[(pos - 1) * kScSearchThreads + threadIdx.x];
      pos--;
    }
    ld[pos * kScSearchThreads + threadIdx.x] = d;
    li[pos * kScSearchThreads + threadIdx.x] = idx;
    cnt = min(cnt + 1, K);
  }
  const int n_out = odometry ? min(L, K) : K;
  int head = 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = 0; c < n_out; c++) {
    float bd = 0.f;
    int bi = INT_MAX;
    if (head < cnt) { bd = ld[head * kScSearchThreads + threadIdx.x]; bi = li[head * kScSearchThreads + threadIdx.x]; }
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_xor(bd, o);
      const int oi = __shfl_xor(bi, o);
      if (oi != INT_MAX && (bi == INT_MAX || sc_key_less(od, oi, bd, bi))) { bd = od; bi = oi; }
    }
    if (lane == 0) { rd[wave] = bd; ri[wave] = bi; }
    __syncthreads();
    bd = rd[0]; bi = ri[0];
    for (int w = 1; w < kScSearchThreads / 64; w++)
      if (ri[w] != INT_MAX && (bi == INT_MAX || sc_key_less(rd[w], ri[w], bd, bi))) { bd = rd[w]; bi = ri[w]; }
    __syncthreads();
    if (head < cnt && li[head * kScSearchThreads + threadIdx.x] == bi) head++;
    if (threadIdx.x == 0) {
      const int db_idx = bi == INT_MAX ? 0 : bi;      // vanilla: a tree with fewer points leaves node 0 in place
      pairs[2 * (off + c)] = qi;
      pairs[2 * (off + c) + 1] = db_base + db_idx;
      pair_sim[off + c] = odometry ? srow[db_idx] : 0.0;
    }
  }
}

__global__ __launch_bounds__(kScSearchThreads) void sc_keysearch_kernel(const ScSearchArgs a) {
  const int t = blockIdx.x, k = blockIdx.y;
  if (a.pair_off[t * a.n_aug + k] < 0) return;
  sc_keysearch_body(a.ringkey, a.ringkey + ((size_t)(a.q0 + t) * a.n_aug + k) * a.R, a.odometry ? a.sim + (size_t)t * a.ld : nullptr,
                    a.n_search[t * a.n_aug + k], a.k_sel, a.R, a.n_aug, a.odometry, a.pair_off[t * a.n_aug + k] - a.pair_base,
                    t * a.n_aug + k, 0, a.pairs, a.pair_sim);
}

// ---- a batch of graphs (cfear_sc_detect_batch) ----------------------------------------------------
// The detected nodes of every graph, one behind the other, are the queries d = 0 .. D - 1; a chunk [q0, q0 + nq) of them may
// start and end inside a graph.  Every query carries its graph: first (the query index of the graph's node 0; positions,
// segments and ring keys are indexed by query), db_base (the descriptor index of the graph's node 0 in the database) and
// row_off, the start of its row of trav / sim: query d with i = d - first[d] earlier nodes owns i entries, so the rows of a
// chunk are packed one behind the other (a prefix sum of i) instead of a [nq][largest graph] rectangle.
struct ScBatchTab {
  const int32_t* first;              // [D]
  const int32_t* db_base;            // [D]
  const int32_t* center;             // [D] the query's node in the caller's node list
  const long long* row_off;          // [D + 1]
  const double2* pos;                // [D] Todom
  const double* seg;                 // [D] |p_{d+1} - p_d| (unused at a graph's last node)
  const int32_t* n_search;           // [D][n_aug]
  const int32_t* pair_off;           // [D][n_aug] first pair (of the whole call); -1: no search
  const int32_t* node_pairs;         // [D + 1] first pair of every query
};

// sc_travel_kernel's sums, back to the graph's first node: trav[row + s] is the sum down to node i - 1 - s
__global__ __launch_bounds__(256) void sc_batch_travel_kernel(const ScBatchTab tb, int q0, int nq, double* trav) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nq) return;
  const int d = q0 + t, g0 = tb.first[d], i = d - g0;
  double* row = trav + (tb.row_off[d] - tb.row_off[q0]);
  double s = 0.0;
  for (int m = i - 1; m >= 0; m--) {
    s += tb.seg[g0 + m];
    row[i - 1 - m] = s;
  }
}

// sc_odom_sim_kernel's terms against the graph's own earlier nodes: one workgroup per query, sim[row + idx]
__global__ __launch_bounds__(256) void sc_batch_odom_sim_kernel(const ScBatchTab tb, const double* trav, int q0, double sigma,
                                                                double* sim) {
  const int d = q0 + blockIdx.x, g0 = tb.first[d], i = d - g0;
  const long long ro = tb.row_off[d] - tb.row_off[q0];
  const double2 pi = tb.pos[d];
  for (int idx = threadIdx.x; idx < i; idx += blockDim.x) {
    const double2 pj = tb.pos[g0 + idx];
    const double est = hypot(pi.x - pj.x, pi.y - pj.y);
    const double e5 = est - 5.0;
    const double error = e5 < 0.0 ? 0.0 : e5;        // std::max(est - 5.0, 0.0)
    const double rel = error / trav[ro + (i - 1 - idx)];
    const double prob = exp(-rel * rel / (2 * sigma * sigma));
    sim[ro + idx] = 1.0 - prob;
  }
}

struct ScBatchSearchArgs {
  ScBatchTab tb;
  const double* ringkey;             // [D][n_aug][R]
  const double* sim;                 // odometry mode: the chunk's packed rows
  int pair_base, q0, R, n_aug, k_sel, odometry;
  int query_is_node;                 // raw mode: the query descriptor is the database entry of the node
  int32_t* pairs;
  double* pair_sim;
};

// one workgroup per (query, augmentation): sc_keysearch_kernel over the graph's own eligible prefix
__global__ __launch_bounds__(kScSearchThreads) void sc_batch_keysearch_kernel(const ScBatchSearchArgs a) {
  const int t = blockIdx.x, k = blockIdx.y, d = a.q0 + t;
  const int po = a.tb.pair_off[d * a.n_aug + k];
  if (po < 0) return;
  const int g0 = a.tb.first[d];
  sc_keysearch_body(a.ringkey + (size_t)g0 * a.n_aug * a.R, a.ringkey + ((size_t)d * a.n_aug + k) * a.R,
                    a.odometry ? a.sim + (a.tb.row_off[d] - a.tb.row_off[a.q0]) : nullptr, a.tb.n_search[d * a.n_aug + k], a.k_sel, a.R,
                    a.n_aug, a.odometry, po - a.pair_base, a.query_is_node ? a.tb.db_base[d] + (d - g0) : t * a.n_aug + k,
                    a.tb.db_base[d], a.pairs, a.pair_sim);
}

// ring keys of the raw descriptors of the queries (no sector keys: the distance kernel forms its own)
__global__ __launch_bounds__(256) void sc_batch_raw_keys_kernel(const double* db, const ScBatchTab tb, int R, int S, double* ringkey) {
  const int d = blockIdx.x;
  sc_keys(db + (size_t)(tb.db_base[d] + (d - tb.first[d])) * R * S, R, S, ringkey + (size_t)d * R, nullptr);
}

// sc_rank_kernel: detectLoopClosureID's ranking (:300-322), one wavefront per query.  The query's pairs are contiguous, in
// visiting order (augmentation, then search rank), at most kScMaxAug * kScMaxTreeK = 64 lanes x 8.  n_sel = min(n_candidates,
// pairs) rounds each take the smallest remaining (min_dist, visiting position): what a stable sort of the growing list
// followed by dropping the last entry leaves, as among equal min_dist the earlier-visited pair stays in front.  The lane that
// owns the winner writes its 64-byte record; records past n_sel keep the zeros the caller's rows were cleared to.
constexpr int kScRankPerLane = kScMaxAug * kScMaxTreeK / 64;

struct ScRankArgs {
  ScBatchTab tb;
  const int32_t* pairs;
  const double* dist;
  const int32_t* shift;
  const double* pair_sim;
  int pair_base, q0, nq, n_aug, n_candidates, odometry;
  double unit;                       // 360 / num_sector
  double shift_y[kScMaxAug];
  cfear_sc_candidate* out;           // [D][n_candidates]
  int32_t* n_out;                    // [D]
};

__device__ __forceinline__ bool sc_rank_less(double da, int pa, double db, int pb) { return da < db || (!(db < da) && pa < pb); }

__global__ __launch_bounds__(256) void sc_rank_kernel(const ScRankArgs a) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.nq) return;                             // the whole wavefront
  const int d = a.q0 + t;
  const int p0 = a.tb.node_pairs[d] - a.pair_base, P = a.tb.node_pairs[d + 1] - a.tb.node_pairs[d];
  const int n_sel = min(a.n_candidates, P);
  double md[kScRankPerLane];
#pragma unroll
  for (int j = 0; j < kScRankPerLane; j++) {
    const int pos = lane + 64 * j;
    md[j] = 0.0;
    if (pos < P) md[j] = a.odometry ? a.dist[p0 + pos] + a.pair_sim[p0 + pos] : a.dist[p0 + pos];
  }
  uint32_t taken = 0;
  for (int c = 0; c < n_sel; c++) {
    double bd = 0.0;
    int bp = INT_MAX;
#pragma unroll
    for (int j = 0; j < kScRankPerLane; j++) {
      const int pos = lane + 64 * j;
      if (pos < P && !((taken >> j) & 1u) && (bp == INT_MAX || sc_rank_less(md[j], pos, bd, bp))) { bd = md[j]; bp = pos; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(bd, o);
      const int op = __shfl_xor(bp, o);
      if (op != INT_MAX && (bp == INT_MAX || sc_rank_less(od, op, bd, bp))) { bd = od; bp = op; }
    }
    bp = __shfl(bp, 0);                              // one answer for the wavefront, whatever a NaN did to the order
    if (bp == INT_MAX) break;
    if ((bp & 63) != lane) continue;
    taken |= 1u << (bp >> 6);
    const int p = p0 + bp;
    double shift_y = 0.0;                            // of the augmentation whose pairs hold p: the last that starts at or before it
#pragma unroll
    for (int kk = 0; kk < kScMaxAug; kk++) {
      const int po = kk < a.n_aug ? a.tb.pair_off[d * a.n_aug + kk] : -1;
      if (po >= 0 && po - a.pair_base <= p) shift_y = a.shift_y[kk];
    }
    const int shift = a.shift[p];
    const double dist = a.dist[p], osim = a.odometry ? a.pair_sim[p] : 0.0;
    cfear_sc_candidate r;
    r.min_dist_sc = dist;
    r.min_dist_odom = osim;
    r.min_dist = a.odometry ? dist + osim : dist;
    const float ang = (float)(shift * a.unit);
    r.yaw_diff_rad = (float)(ang * M_PI / 180.0);
    r.nn_idx = a.pairs[2 * p + 1] - a.tb.db_base[d];
    r.argmin_shift = shift;
    r.pad = 0;
    r.Taug[0] = 0.0; r.Taug[1] = shift_y; r.Taug[2] = 0.0;
    a.out[(size_t)d * a.n_candidates + c] = r;
  }
  if (lane == 0) a.n_out[d] = n_sel;
}

struct ScDistArgs {
  const double* desc_q;      // [nq][R * S]
  const double* desc_c;      // [nc][R * S]
  const int32_t* pairs;      // [n_pairs][2] (query index, candidate index)
  int num_ring, num_sector;
  double search_ratio;
  double* dist;              // [n_pairs]
  int32_t* shift;            // [n_pairs]
  uint32_t sim_off;          // LDS offset of the [chunk][S] similarity matrix
  int chunk;                 // shifts evaluated together (<= 256, as many as the LDS holds)
};

__global__ __launch_bounds__(1024) void sc_distance_kernel(const ScDistArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int R = a.num_ring, S = a.num_sector, cells = R * S;
  double* sc1 = (double*)smem;
  double* sc2 = sc1 + cells;
  double* n1 = sc2 + cells;            // [S] column norms of sc1
  double* n2 = n1 + S;
  double* v1 = n2 + S;                 // [S] sector keys
  double* v2 = v1 + S;
  double* tmp = v2 + S;                // [S] per-shift / per-column results
  int* ctl = (int*)(tmp + S);          // [2 + m] argmin, count, search space (sc_distance_layout)
  const int qi = a.pairs[2 * blockIdx.x], ci = a.pairs[2 * blockIdx.x + 1];
  const double* gq = a.desc_q + (size_t)qi * cells;
  const double* gc = a.desc_c + (size_t)ci * cells;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) { sc1[i] = gq[i]; sc2[i] = gc[i]; }
  __syncthreads();
  for (int c = threadIdx.x; c < S; c += blockDim.x) {
    double s1 = 0, s2 = 0, q1 = 0, q2 = 0;
    for (int r = 0; r < R; r++) {
      const double x = sc1[r * S + c], y = sc2[r * S + c];
      s1 += x; s2 += y; q1 += x * x; q2 += y * y;
    }
    v1[c] = s1 / R; v2[c] = s2 / R; n1[c] = sqrt(q1); n2[c] = sqrt(q2);
  }
  __syncthreads();
  // fastAlignUsingVkey (Scancontext.cpp:134-154): |vkey1 - circshift(vkey2, sh)| for every shift
  for (int sh = threadIdx.x; sh < S; sh += blockDim.x) {
    double sq = 0;
    for (int c = 0; c < S; c++) {
      const double d = v1[(c + sh) % S] - v2[c];
      sq += d * d;
    }
    tmp[sh] = sqrt(sq);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int arg = 0;
    double mn = 10000000;
    for (int sh = 0; sh < S; sh++)
      if (tmp[sh] < mn) { arg = sh; mn = tmp[sh]; }
    // search space around it, ascending (:166-174)
    const int rad = (int)round(0.5 * a.search_ratio * S);
    int* space = ctl + 2;
    int m = 0;
    space[m++] = arg;
    for (int ii = 1; ii < rad + 1; ii++) { space[m++] = (arg + ii + S) % S; space[m++] = (arg - ii + S) % S; }
    for (int i = 1; i < m; i++) {                    // insertion sort (m <= 2 rad + 1)
      const int v = space[i];
      int j = i - 1;
      while (j >= 0 && space[j] > v) { space[j + 1] = space[j]; j--; }
      space[j + 1] = v;
    }
    ctl[0] = m;
  }
  __syncthreads();
  const int m = ctl[0];
  const int* space = ctl + 2;
  // distDirectSC(sc1, circshift(sc2, sh)) (:110-131) for every shift of the search space at once: the (shift, column)
  // cosine similarities are independent, so all threads work on them; the per-shift sum over the columns keeps the
  // reference's sequential order (one thread per shift), as does the dot product over the rings.
  double* sim = (double*)(smem + a.sim_off);         // [chunk][S]; -2 marks "not counted" (similarities lie in [-1, 1])
  double best = 10000000;
  int best_shift = 0;
  for (int k0 = 0; k0 < m; k0 += a.chunk) {          // TBV: 13 shifts, one chunk
    const int mk = min(a.chunk, m - k0);
    for (int item = threadIdx.x; item < mk * S; item += blockDim.x) {
      const int k = item / S, c = item - k * S;
      const int c2 = ((c - space[k0 + k]) % S + S) % S;
      double dot = 0;
      for (int r = 0; r < R; r++) dot += sc1[r * S + c] * sc2[r * S + c2];
      const bool skip = (n1[c] == 0) | (n2[c2] == 0);
      sim[item] = skip ? -2.0 : dot / (n1[c] * n2[c2]);
    }
    __syncthreads();
    if ((int)threadIdx.x < mk) {
      const double* row = sim + (size_t)threadIdx.x * S;
      int eff = 0;
      double sum = 0;
      for (int c = 0; c < S; c++)
        if (row[c] != -2.0) { sum = sum + row[c]; eff = eff + 1; }
      eff = max(eff, 1);
      tmp[threadIdx.x] = 1.0 - sum / eff;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int k = 0; k < mk; k++)
        if (tmp[k] < best) { best_shift = space[k0 + k]; best = tmp[k]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { a.dist[blockIdx.x] = best; a.shift[blockIdx.x] = best_shift; }
}

// ---- raw-sweep Scan Context: RSCManager::MakeRadarContext (RadarScancontext.cpp:41-57) ------------------------------
// cv::threshold(THRESH_TOZERO) of the 8-bit sweep + cv::resize(INTER_AREA) to num_ring x num_sector, as OpenCV 4.2 computes
// them (DESIGN.md section "raw-sweep Scan Context"; restated from OpenCV's imgproc sources, NOT pinned against OpenCV here):
//  * threshold (thresh.cpp, 8U): t = cvFloor(radar_threshold); v is kept where v > t, else 0 (t < 0 keeps all, t >= 255
//    clears all).  The reference thresholds the caller's image in place; this reads it only.
//  * the logical image L [H][W] is the reader's (PNGReaderInterface::Get transposes when rows < cols): rings run along H,
//    sectors along W.  transpose = 1: the stored sweep is azimuth-major, L[y][x] = stored[x][y]; transpose = 0: L = stored.
//  * scale = 1 / ((double)dsize / ssize) per axis.  Both integer (|scale - cvRound(scale)| < DBL_EPSILON): resizeAreaFast_
//    <uchar, int>, integer box sum, cvRound((float)sum * (1.f / area)); 2 x 2 is refused (OpenCV's SIMD body rounds it
//    (s + 2) >> 2, its scalar tail half to even).  Otherwise, both >= 1: computeResizeAreaTab + resizeArea_<uchar, float>:
//    per source row sy (y-table order) buf[dx] = sum of (float)L[sy][sx] * alpha over the x-table entries of dx in order,
//    then sum[dx] = beta * buf[dx] (first row of the output row) or sum[dx] += beta * buf[dx]; every product and sum a
//    separate float operation (no FMA); result saturate_cast<uchar> = cvRound, half to even.  Scales below 1 are refused.
//  * desc = (double)u8; desc_divider / no_point do not apply; keys as sc_keys.  normalize = true and interpolations other
//    than INTER_AREA are refused: TBV cannot reach them, and cv::normalize's convertTo runs in OpenCV's AVX2 FMA dispatch,
//    which a restatement cannot follow exactly.
// sc_raw_descriptor_kernel: one workgroup per (sweep, block of NS sectors).  Stage 1 forms buf[dx][y] for the block's sectors
// and every y into LDS: the source rows x the block touches are walked in ascending x, each row adding into the (at most two)
// sectors it belongs to, so every sector sees its x-table entries in table order, and a row two sectors share is read once.
// transpose = 1: a lane owns 16 consecutive y (one 16-byte load per row, up to kScRawRows rows in flight); transpose = 0: a
// lane owns one y and reads the row's bytes.  Stage 2: one lane per (sector, ring) sums the ring's y-table entries from LDS in
// ascending order.
constexpr int kScRawRows = 8;            // source rows loaded together per lane (transpose = 1)
constexpr int kScRawMaxH = 16384;        // ring-axis source length: NS = 1 needs H * 4 bytes of LDS
constexpr int kScRawLdsBudget = 32 * 1024;

struct ScRawArgs {
  const uint8_t* img;
  int rows, cols, stride, thr;           // stored layout; thr = cvFloor(radar_threshold) clamped to [-1, 255]
  long long batch_stride;
  int H, W, R, S, nblk, Hp, fast;        // logical image H x W -> R x S; nblk sector blocks per sweep; LDS pitch (floats)
  float inv_area;                        // fast path: 1.f / (iscale_x * iscale_y)
  const int4* rowtab;                    // [W] per source x: (dx, alpha bits, dx', alpha' bits), dx' = -1 if none
  const int2* xspan;                     // [S] first / last source x of sector dx
  const int* yoff;                       // [R + 1] y-table entries of ring dy: [yoff[dy], yoff[dy + 1])
  const int2* yent;                      // (sy, beta bits)
  double* desc;                          // [batch][R * S]
};

__device__ __forceinline__ float sc_raw_val(uint32_t byte, int thr) { return (int)byte > thr ? (float)byte : 0.0f; }

// one source row's contribution: acc[k] += v * alpha for each sector dx0 + k of the block the row belongs to (table entry
// t, see ScRawArgs::rowtab); no FMA: the order and rounding of resizeArea_
template <int NS, int N>
__device__ __forceinline__ void sc_raw_row(float (&acc)[NS][N], const float (&v)[N], const int4 t, int dx0) {
#pragma unroll
  for (int k = 0; k < NS; k++) {
    const int dx = dx0 + k;
    if (t.x == dx || t.z == dx) {
      const float alpha = __int_as_float(t.x == dx ? t.y : t.w);
#pragma unroll
      for (int j = 0; j < N; j++) acc[k][j] = __fadd_rn(acc[k][j], __fmul_rn(v[j], alpha));
    }
  }
}

// 16 bytes of a row from `pos` into w, zeros past n.  The piece is read whole (one 16-byte load) where the row starts on a
// 4-byte boundary and the piece ends inside the image (room = bytes from the row start to the image's end); the bytes past n
// are then cleared in registers.  Otherwise only bytes < n are read, one by one.
__device__ __forceinline__ void sc_raw_piece(const uint8_t* rowp, int pos, int n, long long room, uint32_t (&w)[4]) {
  if ((((uintptr_t)rowp) & 3) == 0 && (long long)pos + 16 <= room) {
    const u32x4_a4 v = __builtin_nontemporal_load((const u32x4_a4*)(rowp + pos));
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    if (pos + 16 > n) {
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const int rem = n - (pos + 4 * d);
        w[d] &= rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
      }
    }
  } else {
#pragma unroll
    for (int d = 0; d < 4; d++) {
      uint32_t word = 0;
#pragma unroll
      for (int by = 0; by < 4; by++) {
        const int p = pos + 4 * d + by;
        if (p < n) word |= (uint32_t)rowp[p] << (8 * by);
      }
      w[d] = word;
    }
  }
}

template <int NS, int TRANSPOSE>
__global__ __launch_bounds__(256) void sc_raw_descriptor_kernel(const ScRawArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* buf = (float*)smem;                                   // [NS][Hp]
  const int blk = blockIdx.x % a.nblk, b = blockIdx.x / a.nblk;
  const int dx0 = blk * NS, ns = min(NS, a.S - dx0);
  const int xr0 = a.xspan[dx0].x, xr1 = a.xspan[dx0 + ns - 1].y;
  const uint8_t* img = a.img + (long long)b * a.batch_stride;
  const long long img_end = (long long)(a.rows - 1) * a.stride + a.cols;
  if (TRANSPOSE) {
    // stored rows are x (azimuths), contiguous along y
    const int npieces = (a.H + 15) / 16;
    for (int p = threadIdx.x; p < npieces; p += blockDim.x) {
      float acc[NS][16];
#pragma unroll
      for (int k = 0; k < NS; k++)
#pragma unroll
        for (int j = 0; j < 16; j++) acc[k][j] = 0.0f;
      for (int x0 = xr0; x0 <= xr1; x0 += kScRawRows) {
        uint32_t w[kScRawRows][4];
#pragma unroll
        for (int r = 0; r < kScRawRows; r++) {
          const int x = x0 + r;
          if (x <= xr1) {
            const long long off = (long long)x * a.stride;
            sc_raw_piece(img + off, p * 16, a.H, img_end - off, w[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < kScRawRows; r++) {
          const int x = x0 + r;
          if (x <= xr1) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = sc_raw_val((w[r][j >> 2] >> (8 * (j & 3))) & 0xffu, a.thr);
            sc_raw_row<NS, 16>(acc, v, a.rowtab[x], dx0);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < NS; k++)
#pragma unroll
        for (int q = 0; q < 4; q++)
          *(float4*)(buf + k * a.Hp + p * 16 + 4 * q) = make_float4(acc[k][4 * q], acc[k][4 * q + 1], acc[k][4 * q + 2], acc[k][4 * q + 3]);
    }
  } else {
    // stored rows are y, contiguous along x
    for (int y = threadIdx.x; y < a.H; y += blockDim.x) {
      float acc[NS][1];
#pragma unroll
      for (int k = 0; k < NS; k++) acc[k][0] = 0.0f;
      const uint8_t* rowp = img + (long long)y * a.stride;
      for (int x = xr0; x <= xr1; x++) {
        const float v[1] = {sc_raw_val(rowp[x], a.thr)};
        sc_raw_row<NS, 1>(acc, v, a.rowtab[x], dx0);
      }
#pragma unroll
      for (int k = 0; k < NS; k++) buf[k * a.Hp + y] = acc[k][0];
    }
  }
  __syncthreads();
  double* out = a.desc + (size_t)b * a.R * a.S;
  for (int t = threadIdx.x; t < ns * a.R; t += blockDim.x) {
    const int k = t / a.R, dy = t - k * a.R;
    const float* bk = buf + k * a.Hp;
    const int e0 = a.yoff[dy], e1 = a.yoff[dy + 1];
    float v;
    if (a.fast) {                                              // resizeAreaFast_: integer box sum (buf holds integers)
      int s = 0;
      for (int e = e0; e < e1; e++) s += (int)bk[a.yent[e].x];
      v = __fmul_rn((float)s, a.inv_area);
    } else {
      const int2 f = a.yent[e0];
      v = __fmul_rn(__int_as_float(f.y), bk[f.x]);
      for (int e = e0 + 1; e < e1; e++) {
        const int2 g = a.yent[e];
        v = __fadd_rn(v, __fmul_rn(__int_as_float(g.y), bk[g.x]));
      }
    }
    const int u = min(max(__float2int_rn(v), 0), 255);        // saturate_cast<uchar>(float): cvRound, half to even
    out[(size_t)dy * a.S + dx0 + k] = (double)u;
  }
}

__global__ __launch_bounds__(256) void sc_raw_keys_kernel(const double* desc, int R, int S, double* ringkey, double* sectorkey) {
  const size_t b = blockIdx.x;
  sc_keys(desc + b * R * S, R, S, ringkey + b * R, sectorkey + b * S);
}

// LDS of sc_distance_kernel: both descriptors, five [S] vectors, ctl = (argmin, count, search space), then the [chunk][S]
// similarity matrix.  The search space holds m = 2 round(0.5 search_ratio S) + 1 shifts (duplicates included, as the
// reference keeps them); a negative radius leaves the vkey argmin alone.
constexpr size_t kScDistLds = (size_t)160 * 1024;
constexpr double kScMaxSpace = 1 << 20;  // search-space entries checked before the int conversion (the LDS refuses far fewer)

struct ScDistLayout { size_t base; int m_max; };

// the layout for (R, S, ratio); ratio must be finite
ScDistLayout sc_distance_layout(int R, int S, double ratio) {
  const double rad = std::round(0.5 * ratio * S);
  const int m_max = rad < 0 ? 1 : (rad > kScMaxSpace ? (int)kScMaxSpace : 2 * (int)rad + 1);
  const size_t base = (((size_t)2 * R * S + 5 * (size_t)S) * 8 + (size_t)(2 + m_max) * 4 + 15) & ~(size_t)15;
  return {base, m_max};
}

int check_sc_params(cfear_ctx* ctx, const cfear_sc_params* p) {
  if (!p) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null parameters");
  if (p->num_ring < 1 || p->num_sector < 1 || (long long)p->num_ring * p->num_sector > kScMaxCells)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "num_ring x num_sector must be in [1, %d]", kScMaxCells);
  if (!(p->max_radius > 0) || p->desc_divider == 0.0 || p->desc_function < 0 || p->desc_function > 1 || !std::isfinite(p->search_ratio))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad scan-context parameters");
  // the distance kernel keeps both descriptors, the search space and one shift's similarities in LDS
  const ScDistLayout l = sc_distance_layout(p->num_ring, p->num_sector, p->search_ratio);
  if (l.base + (size_t)p->num_sector * 8 > kScDistLds)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "scan-context distance of %d x %d with search_ratio %g needs more than %d KiB of LDS",
                           p->num_ring, p->num_sector, p->search_ratio, (int)(kScDistLds / 1024));
  return CFEAR_OK;
}

// sc_distance_kernel over n_pairs device pairs: a carries the device buffers, the rest is filled in here; par passed
// check_sc_params
int sc_distance_launch(cfear_ctx* ctx, ScDistArgs a, int n_pairs, const cfear_sc_params* par) {
  if (n_pairs == 0) return CFEAR_OK;
  const int R = par->num_ring, S = par->num_sector;
  a.num_ring = R; a.num_sector = S; a.search_ratio = par->search_ratio;
  const ScDistLayout l = sc_distance_layout(R, S, par->search_ratio);
  const size_t room = (kScDistLds - l.base) / ((size_t)S * 8);
  // tmp[] holds one distance per shift of a chunk (<= S); one thread sums each shift (<= block size)
  a.chunk = (int)std::max<size_t>(1, std::min<size_t>({room, (size_t)l.m_max, (size_t)256, (size_t)S}));
  a.sim_off = (uint32_t)l.base;
  const size_t lds = l.base + (size_t)a.chunk * S * 8;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)sc_distance_kernel, kScDistLds));
  {
    ProfScope ps(ctx, "sc_distance");
    hipLaunchKernelGGL(sc_distance_kernel, dim3(n_pairs), dim3(kScDistThreads), lds, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

// the query's lateral shifts: the node itself, then RadarScancontext.cpp:164's augmentations
std::vector<double> sc_aug_shifts(bool augment) {
  if (!augment) return {0.0};
  return {0.0, -2.0, 2.0, -4.0, 4.0};
}

}  // namespace

extern "C" void cfear_sc_params_default(cfear_sc_params* p) {
  if (!p) return;
  p->num_ring = 40; p->num_sector = 120;           // RadarScancontext.h:37-38
  p->max_radius = 80.0;                            // :39
  p->search_ratio = 0.1;                           // :40
  p->desc_function = 0;                            // "sum" (:52)
  p->pad = 0;
  p->desc_divider = 1000.0;                        // tbv_slam_offline.cpp:88 (the struct default is 1)
  p->no_point = 0.0;                               // :51
}

extern "C" int cfear_sc_descriptors(cfear_ctx* ctx, const cfear_sc_cloud* clouds, int32_t n_clouds,
                                    const cfear_sc_params* par, const double* shifts_y, int32_t n_aug, double* desc,
                                    double* ringkey, double* sectorkey) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!clouds || !desc || n_clouds < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_sc_params(ctx, par));
  if (n_aug < 1 || n_aug > kScMaxAug || (n_aug > 1 && !shifts_y))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_aug must be in [1, %d]", kScMaxAug);
  if (n_clouds == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int R = par->num_ring, S = par->num_sector, cells = R * S;
  HostStage st(ctx, kWsCoral);
  for (int i = 0; i < n_clouds; i++) {
    if (clouds[i].n < 0 || (clouds[i].n > 0 && !clouds[i].xyzi)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cloud %d: null", i);
    st.cloud_in(clouds[i].xyzi, clouds[i].n);
  }
  const size_t nd = (size_t)n_clouds * n_aug;
  ScDescArgs a;
  st.piece(a.clouds, (size_t)n_clouds * sizeof(ScCloud));
  st.out(a.desc, desc, nd * cells * sizeof(double));         // a descriptor database kept in HBM is written in place
  st.piece(a.ringkey, nd * (R + S) * sizeof(double));
  CFEAR_CHECK(st.carve());
  ScCloud* h = (ScCloud*)st.record((size_t)n_clouds * sizeof(ScCloud));
  for (int i = 0; i < n_clouds; i++) {
    h[i].n = clouds[i].n; h[i].pad = 0;
    h[i].xyzi = st.cloud(clouds[i].xyzi);
  }
  CFEAR_CHECK(st.upload((void*)a.clouds, h, (size_t)n_clouds * sizeof(ScCloud)));
  a.num_ring = R; a.num_sector = S; a.desc_function = par->desc_function; a.n_aug = n_aug;
  a.max_radius = par->max_radius; a.desc_divider = par->desc_divider; a.no_point = par->no_point;
  for (int k = 0; k < kScMaxAug; k++) a.shift_y[k] = (k < n_aug && shifts_y) ? shifts_y[k] : 0.0;
  a.sectorkey = a.ringkey + nd * R;
  {
    ProfScope ps(ctx, "sc_descriptor");
    hipLaunchKernelGGL(sc_descriptor_kernel, dim3(n_clouds, n_aug), dim3(256), (size_t)cells * 12, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  if (ringkey) st.back(ringkey, a.ringkey, nd * R * sizeof(double));
  if (sectorkey) st.back(sectorkey, a.sectorkey, nd * S * sizeof(double));
  return st.finish();
}

extern "C" int cfear_sc_distance_batch(cfear_ctx* ctx, const double* desc_q, int32_t n_q, const double* desc_c,
                                       int32_t n_c, const int32_t* pairs, int32_t n_pairs, const cfear_sc_params* par,
                                       double* dist, int32_t* shift) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!desc_q || !desc_c || !pairs || !dist || !shift || n_pairs < 0 || n_q < 0 || n_c < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_sc_params(ctx, par));
  if (n_pairs == 0) return CFEAR_OK;
  for (int i = 0; i < n_pairs; i++)
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_q || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= n_c)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "pair %d out of range", i);
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int R = par->num_ring, S = par->num_sector, cells = R * S;
  const size_t qb = (size_t)n_q * cells * 8, cb = (size_t)n_c * cells * 8, pb = (size_t)n_pairs * 8;
  HostStage st(ctx, kWsClouds);
  ScDistArgs a;
  st.in(a.desc_q, desc_q, qb);
  st.in(a.desc_c, desc_c, cb);
  st.in(a.pairs, pairs, pb);
  st.out(a.dist, dist, (size_t)n_pairs * 8);
  st.out(a.shift, shift, (size_t)n_pairs * 4);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(sc_distance_launch(ctx, a, n_pairs, par));
  return st.finish();
}

extern "C" void cfear_sc_raw_params_default(cfear_sc_raw_params* p) {
  if (!p) return;
  p->radar_threshold = 0.0;                        // RadarScancontext.h:36
  p->transpose = 1;                                // an azimuth-major sweep, read as PNGReaderInterface::Get returns it
  p->normalize = 0;                                // :45
  p->interpolation = CFEAR_SC_INTER_AREA;          // "area" (:46)
  p->pad = 0;
}

namespace {
// computeResizeAreaTab (OpenCV imgproc/src/resize.cpp) for one axis: entries (output index, source index, weight) in order
void sc_area_tab(int ssize, int dsize, std::vector<int>& di, std::vector<int>& si, std::vector<float>& alpha) {
  const double scale = 1. / ((double)dsize / ssize);
  for (int d = 0; d < dsize; d++) {
    const double fs1 = d * scale, fs2 = fs1 + scale, cell = std::min(scale, ssize - fs1);
    int s1 = (int)std::ceil(fs1), s2 = (int)std::floor(fs2);
    s2 = std::min(s2, ssize - 1);
    s1 = std::min(s1, s2);
    if (s1 - fs1 > 1e-3) { di.push_back(d); si.push_back(s1 - 1); alpha.push_back((float)((s1 - fs1) / cell)); }
    for (int s = s1; s < s2; s++) { di.push_back(d); si.push_back(s); alpha.push_back((float)(1.0 / cell)); }
    if (fs2 - s2 > 1e-3) { di.push_back(d); si.push_back(s2); alpha.push_back((float)(std::min(std::min(fs2 - s2, 1.), cell) / cell)); }
  }
}

int float_bits(float f) { int i; memcpy(&i, &f, 4); return i; }

template <int NS>
void sc_raw_launch(const ScRawArgs& a, int transpose, int batch, size_t lds, hipStream_t s) {
  if (transpose) hipLaunchKernelGGL((sc_raw_descriptor_kernel<NS, 1>), dim3(a.nblk * batch), dim3(256), lds, s, a);
  else hipLaunchKernelGGL((sc_raw_descriptor_kernel<NS, 0>), dim3(a.nblk * batch), dim3(256), lds, s, a);
}
}  // namespace

extern "C" int cfear_sc_raw_descriptors(cfear_ctx* ctx, const uint8_t* imgs, const cfear_polar_desc* desc,
                                        const cfear_sc_params* par, const cfear_sc_raw_params* raw, double* out,
                                        double* ringkey, double* sectorkey) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!imgs || !desc || !par || !raw || !out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (raw->normalize)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: normalize = true is not supported");
  if (raw->interpolation != CFEAR_SC_INTER_AREA)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: only INTER_AREA interpolation is supported");
  if (raw->transpose != 0 && raw->transpose != 1)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: transpose must be 0 or 1");
  if (!(raw->radar_threshold >= -2147483648.0 && raw->radar_threshold < 2147483648.0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: radar_threshold must be finite and fit an int");
  const int R = par->num_ring, S = par->num_sector;
  if (R < 1 || S < 1 || (long long)R * S > kScMaxCells)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "num_ring x num_sector must be in [1, %d]", kScMaxCells);
  const cfear_polar_desc& d = *desc;
  if (d.rows <= 0 || d.cols <= 0 || d.stride < d.cols || d.batch < 0 || (d.batch > 1 && d.batch_stride < (int64_t)d.rows * d.stride))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad polar descriptor");
  const int H = raw->transpose ? d.cols : d.rows, W = raw->transpose ? d.rows : d.cols;
  if (H > kScRawMaxH) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "raw scan context: %d source rings > %d", H, kScRawMaxH);
  const double scale_x = 1. / ((double)S / W), scale_y = 1. / ((double)R / H);
  if (scale_x < 1 || scale_y < 1)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: a %d x %d image cannot be area-downscaled to %d x %d",
                           H, W, R, S);
  const int isx = (int)std::nearbyint(scale_x), isy = (int)std::nearbyint(scale_y);
  const bool fast = std::abs(scale_x - isx) < DBL_EPSILON && std::abs(scale_y - isy) < DBL_EPSILON;
  if (fast && isx == 2 && isy == 2)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: INTER_AREA at exactly 2 x 2 is not supported");
  if (d.batch == 0) return CFEAR_OK;
  // tables: per source x its (at most two) sectors, per sector its source span, per ring its y entries
  std::vector<int> xd, xs, yd, ys;
  std::vector<float> xa, ya;
  if (fast) {
    for (int x = 0; x < W; x++) { xd.push_back(x / isx); xs.push_back(x); xa.push_back(1.0f); }
    for (int y = 0; y < H; y++) { yd.push_back(y / isy); ys.push_back(y); ya.push_back(1.0f); }
  } else {
    sc_area_tab(W, S, xd, xs, xa);
    sc_area_tab(H, R, yd, ys, ya);
  }
  const size_t ny = ys.size();
  const size_t o_span = (size_t)W * 16, o_yoff = o_span + (size_t)S * 8, o_yent = (o_yoff + (size_t)(R + 1) * 4 + 7) & ~(size_t)7;
  const size_t tab_bytes = o_yent + ny * 8;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsCoral);
  const uint8_t* d_img;
  const cfear_polar_desc dd = st.images(d_img, imgs, d);
  ScRawArgs a;
  char* d_tab;
  st.piece(d_tab, tab_bytes);
  st.out(a.desc, out, (size_t)d.batch * R * S * sizeof(double));
  double* d_keys = nullptr;
  if (ringkey || sectorkey) st.piece(d_keys, (size_t)d.batch * (R + S) * sizeof(double));
  char* h = (char*)st.record(tab_bytes);
  int4* rowtab = (int4*)h;
  int2* span = (int2*)(h + o_span);
  int* yoff = (int*)(h + o_yoff);
  int2* yent = (int2*)(h + o_yent);
  for (int x = 0; x < W; x++) rowtab[x] = make_int4(-1, 0, -1, 0);
  for (int s = 0; s < S; s++) span[s] = make_int2(INT32_MAX, -1);
  for (size_t e = 0; e < xs.size(); e++) {
    int4& t = rowtab[xs[e]];
    if (t.x < 0) { t.x = xd[e]; t.y = float_bits(xa[e]); }
    else if (t.z < 0) { t.z = xd[e]; t.w = float_bits(xa[e]); }
    else return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: source column %d in more than two sectors", xs[e]);
    span[xd[e]].x = std::min(span[xd[e]].x, xs[e]);
    span[xd[e]].y = std::max(span[xd[e]].y, xs[e]);
  }
  for (int s = 0; s < S; s++)
    if (span[s].y < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: sector %d is empty", s);
  for (int r = 0; r <= R; r++) yoff[r] = 0;
  for (size_t e = 0; e < ny; e++) { yoff[yd[e] + 1]++; yent[e] = make_int2(ys[e], float_bits(ya[e])); }
  for (int r = 0; r < R; r++) {
    if (yoff[r + 1] == 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "raw scan context: ring %d is empty", r);
    yoff[r + 1] += yoff[r];
  }
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(st.upload(d_tab, h, tab_bytes));
  a.img = d_img;
  a.rows = dd.rows; a.cols = dd.cols; a.stride = dd.stride;
  a.batch_stride = dd.batch > 1 ? dd.batch_stride : 0;
  a.thr = (int)std::max(-1.0, std::min(255.0, std::floor(raw->radar_threshold)));
  a.H = H; a.W = W; a.R = R; a.S = S; a.fast = fast ? 1 : 0;
  a.inv_area = 1.f / (float)(fast ? isx * isy : 1);
  a.rowtab = (const int4*)d_tab; a.xspan = (const int2*)(d_tab + o_span);
  a.yoff = (const int*)(d_tab + o_yoff); a.yent = (const int2*)(d_tab + o_yent);
  a.Hp = (H + 15) / 16 * 16;
  const int ns = (size_t)4 * a.Hp * 4 <= (size_t)kScRawLdsBudget && S >= 4 ? 4 : ((size_t)2 * a.Hp * 4 <= (size_t)kScRawLdsBudget && S >= 2 ? 2 : 1);
  a.nblk = (S + ns - 1) / ns;
  const size_t lds = (size_t)ns * a.Hp * 4;
  if ((long long)a.nblk * d.batch > INT32_MAX) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "raw scan context: batch too large");
  {
    ProfScope ps(ctx, "sc_raw_descriptor");
    if (ns == 4) sc_raw_launch<4>(a, raw->transpose, d.batch, lds, ctx->stream);
    else if (ns == 2) sc_raw_launch<2>(a, raw->transpose, d.batch, lds, ctx->stream);
    else sc_raw_launch<1>(a, raw->transpose, d.batch, lds, ctx->stream);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  if (d_keys) {
    {
      ProfScope ps(ctx, "sc_raw_keys");
      hipLaunchKernelGGL(sc_raw_keys_kernel, dim3(d.batch), dim3(256), 0, ctx->stream, a.desc, R, S, d_keys, d_keys + (size_t)d.batch * R);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    if (ringkey) st.back(ringkey, d_keys, (size_t)d.batch * R * sizeof(double));
    if (sectorkey) st.back(sectorkey, d_keys + (size_t)d.batch * R, (size_t)d.batch * S * sizeof(double));
  }
  return st.finish();
}

// ---- RSCManager: descriptor database + retrieval policy (host) around the two kernels ----------------------
// Restates RSCManager::makeAndSaveScancontextAndKeysRadarCloud (RadarScancontext.cpp:156-180), the recent-node
// exclusion and odometry likelihood (:181-222), OdometryNNSearch / the ring-key KNN (:225-284) and
// detectLoopClosureID (:286-345).  The descriptors never leave HBM: the database is one device array, the query and
// its lateral augmentations another; only ring keys (40 floats per descriptor) and distances cross PCIe.
struct cfear_sc_manager {
  cfear_ctx* ctx = nullptr;
  cfear_sc_manager_params par{};
  int cells = 0;
  DevBuf<double> d_db;           // [cap][cells]
  int cap = 0, n = 0;
  DevBuf<double> d_cur;          // [n_aug][cells] current node and its augmentations
  int n_aug = 1;
  int cur_aug = 1;               // entries of current_and_augments_: n_aug after add, 1 after add_raw (RadarScancontext.cpp:133-146)
  std::vector<std::vector<float>> ringkeys;          // polarcontext_invkeys_mat_
  std::vector<std::vector<float>> cur_keys;          // ring keys of current_and_augments_
  std::vector<double> shifts;                        // lateral shift of every augmentation (Taug = (0, shift, 0))
  std::vector<double> poses;                         // odom_poses_ (x, y, theta)
  std::vector<double> odom_similarity;
  int num_exclude_recent = 0;
  // VanillaKDNNSearch's tree bookkeeping (RadarScancontext.cpp:227-238; Scancontext.h:116-117): rebuilt on every 50th CALL
  // from the keys older than the recent-node exclusion at that moment
  int tree_making_period_counter = 0;
  int tree_n = 0;                                    // polarcontext_invkeys_to_search_ = ringkeys[0 .. tree_n)
};

extern "C" void cfear_sc_manager_params_default(cfear_sc_manager_params* p) {
  if (!p) return;
  cfear_sc_params_default(&p->sc);
  p->num_candidates_from_tree = 10;   // NUM_CANDIDATES_FROM_TREE (Scancontext.h:117)
  p->n_candidates = 3;                // par.N_CANDIDATES (tbv_slam launch default)
  p->odom_sigma_error = 0.05;         // RSCManager::Parameters::odom_sigma_error
  p->odometry_coupled_closure = 1;
  p->augment_sc = 1;
  p->pad = 0;
  p->distance_exclude_recent = 10.0;  // DISTANCE_EXCLUDE_RECENT (Scancontext.h:108)
}

extern "C" int cfear_sc_manager_create(cfear_ctx* ctx, const cfear_sc_manager_params* par, cfear_sc_manager** out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!par || !out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  const int rc = check_sc_params(ctx, &par->sc);
  if (rc != CFEAR_OK) return rc;
  if (par->num_candidates_from_tree < 1 || par->n_candidates < 1 || !(par->odom_sigma_error > 0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad scan-context manager parameters");
  std::unique_ptr<cfear_sc_manager> m(new cfear_sc_manager());
  m->ctx = ctx; m->par = *par;
  m->cells = par->sc.num_ring * par->sc.num_sector;
  m->shifts = sc_aug_shifts(par->augment_sc != 0);
  m->n_aug = (int)m->shifts.size();
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (!(m->d_cur = dev_alloc<double>((size_t)m->n_aug * m->cells * sizeof(double))))
    return cfear_set_error(ctx, CFEAR_ERR_HIP, "hipMalloc failed");
  *out = m.release();
  return CFEAR_OK;
}

extern "C" int cfear_sc_manager_destroy(cfear_sc_manager* m) {
  if (!m) return CFEAR_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  delete m;
  return CFEAR_OK;
}

extern "C" int cfear_sc_manager_size(const cfear_sc_manager* m) { return m ? m->n : CFEAR_ERR_INVALID_ARGUMENT; }

namespace {
// Host policy shared by the streaming manager and cfear_sc_detect_sequence.
// ExcludeAndUpdateLikelihood's recent-node count (RadarScancontext.cpp:181-200) for node `cur`; seg(i) = |p_i - p_{i+1}|
template <class Seg>
int sc_num_exclude_recent(int cur, double distance_exclude_recent, Seg seg) {
  if (cur + 1 <= 2) return 2;
  double distance = 0.0;
  int n_ex = 0;
  for (int i = cur; i >= 0 && distance < distance_exclude_recent; i--) {
    distance = distance + (i == cur ? std::hypot(0.0, 0.0) : seg(i));
    n_ex++;
  }
  return n_ex;
}

// VanillaKDNNSearch's tree bookkeeping for one call (:227-238): rebuilt on every 50th call from the n - exclude oldest keys
inline void sc_tree_step(int& counter, int& tree_n, int n, int num_exclude_recent) {
  if (counter % 50 == 0) tree_n = std::max(n - num_exclude_recent, 0);
  counter++;
}

// detectLoopClosureID's ranking (:300-322) of one (augmentation, candidate) pair: std::sort of the growing list, then the
// worst is erased.  The list is sorted already, so the stable sort puts the new entry after every entry of equal min_dist.
void sc_rank_push(std::vector<cfear_sc_candidate>& similar, const cfear_sc_manager_params& par, double dist, int shift,
                  double odom_sim, int idx, double shift_y) {
  const double unit = 360.0 / (double)par.sc.num_sector;
  cfear_sc_candidate c{};
  c.min_dist_sc = dist;
  c.min_dist_odom = par.odometry_coupled_closure ? odom_sim : 0.0;
  c.min_dist = par.odometry_coupled_closure ? dist + c.min_dist_odom : dist;
  const float ang = (float)(shift * unit);
  c.yaw_diff_rad = (float)(ang * M_PI / 180.0);
  c.nn_idx = idx;
  c.argmin_shift = shift;
  c.Taug[0] = 0.0; c.Taug[1] = shift_y; c.Taug[2] = 0.0;
  similar.push_back(c);
  std::stable_sort(similar.begin(), similar.end(),
                   [](const cfear_sc_candidate& a, const cfear_sc_candidate& b) { return a.min_dist < b.min_dist; });
  if ((int)similar.size() > par.n_candidates) similar.pop_back();
}

// makeAndSaveScancontextAndKeys (RadarScancontext.cpp:133-146) + ExcludeAndUpdateLikelihood (:181-222) for the descriptors
// just written to d_cur: d_cur[0] joins the database, the n_cur entries of d_cur (ring keys rk) become current_and_augments_
int sc_manager_commit(cfear_sc_manager* m, const std::vector<double>& rk, int n_cur, const double Todom[3]) {
  cfear_ctx* ctx = m->ctx;
  const int R = m->par.sc.num_ring;
  if (m->n == m->cap) {                                      // grow the database (device to device)
    const int ncap = std::max(256, m->cap * 2);
    DevBuf<double> nd = dev_alloc<double>((size_t)ncap * m->cells * sizeof(double));
    if (!nd) return cfear_set_error(ctx, CFEAR_ERR_HIP, "descriptor database: hipMalloc failed");
    if (m->n > 0)
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(nd.get(), m->d_db.get(), (size_t)m->n * m->cells * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    m->d_db = std::move(nd);                                  // only now: a failed copy above frees nd and keeps the database
    m->cap = ncap;
  }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(m->d_db.get() + (size_t)m->n * m->cells, m->d_cur.get(), (size_t)m->cells * sizeof(double),
                                      hipMemcpyDeviceToDevice, ctx->stream));
  m->n++;
  m->cur_aug = n_cur;
  m->cur_keys.assign(n_cur, std::vector<float>(R));
  for (int k = 0; k < n_cur; k++)
    for (int r = 0; r < R; r++) m->cur_keys[k][r] = (float)rk[(size_t)k * R + r];      // eig2stdvec: double -> float
  m->ringkeys.push_back(m->cur_keys[0]);
  // ExcludeAndUpdateLikelihood (:181-222)
  m->poses.insert(m->poses.end(), Todom, Todom + 3);
  const int np = (int)m->poses.size() / 3;
  auto px = [&](int i) { return m->poses[3 * (size_t)i]; };
  auto py = [&](int i) { return m->poses[3 * (size_t)i + 1]; };
  m->num_exclude_recent = sc_num_exclude_recent(np - 1, m->par.distance_exclude_recent,
                                                [&](int i) { return std::hypot(px(i) - px(i + 1), py(i) - py(i + 1)); });
  const int cur = np - 1;
  m->odom_similarity.assign(cur, 0.0);
  double tpx = Todom[0], tpy = Todom[1], trav = 0.0;
  for (int i = cur - 1; i >= 0; i--) {
    trav += std::hypot(tpx - px(i), tpy - py(i));
    tpx = px(i); tpy = py(i);
    const double est = std::hypot(Todom[0] - px(i), Todom[1] - py(i));
    const double error = std::max(est - 5.0, 0.0);
    const double rel = error / trav;
    const double prob = std::exp(-rel * rel / (2 * m->par.odom_sigma_error * m->par.odom_sigma_error));
    m->odom_similarity[i] = 1.0 - prob;
  }
  return CFEAR_OK;
}
}  // namespace

extern "C" int cfear_sc_manager_add(cfear_sc_manager* m, const float* xyzi, int32_t n_points, const double Todom[3]) {
  if (!m || !Todom || n_points < 0 || (n_points > 0 && !xyzi)) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = m->ctx;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int R = m->par.sc.num_ring;
  cfear_sc_cloud cloud{xyzi, n_points, 0};
  std::vector<double> rk((size_t)m->n_aug * R);
  int rc = cfear_sc_descriptors(ctx, &cloud, 1, &m->par.sc, m->shifts.data(), m->n_aug, m->d_cur.get(), rk.data(), nullptr);
  if (rc != CFEAR_OK) return rc;
  return sc_manager_commit(m, rk, m->n_aug, Todom);
}

// makeAndSaveScancontextAndKeysRadarRaw (RadarScancontext.cpp:148-154): the node's raw sweep, no lateral augmentations
extern "C" int cfear_sc_manager_add_raw(cfear_sc_manager* m, const uint8_t* img, const cfear_polar_desc* desc,
                                        const cfear_sc_raw_params* raw, const double Todom[3]) {
  if (!m || !Todom || !img || !desc || !raw) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = m->ctx;
  if (desc->batch != 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "add_raw takes one sweep (batch = 1)");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<double> rk((size_t)m->par.sc.num_ring);
  const int rc = cfear_sc_raw_descriptors(ctx, img, desc, &m->par.sc, raw, m->d_cur.get(), rk.data(), nullptr);
  if (rc != CFEAR_OK) return rc;
  return sc_manager_commit(m, rk, 1, Todom);
}

extern "C" int cfear_sc_manager_detect(cfear_sc_manager* m, cfear_sc_candidate* out, int32_t cap, int32_t* n_out) {
  if (!m || !n_out || cap < 0 || (cap > 0 && !out)) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = m->ctx;
  *n_out = 0;
  if (m->n < m->num_exclude_recent + 1) return CFEAR_OK;                      // :288-291
  const int R = m->par.sc.num_ring;
  const int cur = m->n - 1;
  std::vector<int32_t> pairs;                                                 // (augmentation, candidate) in visiting order
  for (int k = 0; k < m->cur_aug; k++) {
    const std::vector<float>& key = m->cur_keys[k];
    std::vector<std::pair<float, int>> cands;
    if (m->par.odometry_coupled_closure) {                                    // OdometryNNSearch (:259-284)
      for (int idx = 0; idx < std::max(cur - 1 - m->num_exclude_recent, 0); idx++) {
        float l2 = 0.f;                                                       // L2norm (:250-257): float sum, double terms
        for (int r = 0; r <= R; r++) {
          const float a = r < R ? key[r] : 0.0f;
          const float b = r < R ? m->ringkeys[idx][r] : (float)(10 * m->odom_similarity[idx]);
          const double err = (double)(a - b);
          l2 = (float)((double)l2 + err * err);
        }
        cands.emplace_back(l2, idx);
      }
    } else {                                                                  // VanillaKDNNSearch (:225-248)
      // The reference asks a nanoflann kd-tree (exact search, eps = 0) that it rebuilds on every TREE_MAKING_PERIOD_-th
      // call only, and copies the whole zero-initialised index vector: a tree with fewer points than requested proposes
      // node 0 for the missing places.  A linear scan with the tree's metric arithmetic (L2_Adaptor::evalMetric: four
      // squared differences are added among themselves, then to the running sum) finds the same neighbours; equal
      // distances come back in index order here, in tree-visiting order there (tests/test_ref_nanoflann.py).
      sc_tree_step(m->tree_making_period_counter, m->tree_n, m->n, m->num_exclude_recent);
      for (int idx = 0; idx < m->tree_n; idx++) {
        const float* kk = m->ringkeys[idx].data();
        float d = 0.f;
        int r = 0;
        for (; r + 3 < R; r += 4) {
          const float e0 = key[r] - kk[r], e1 = key[r + 1] - kk[r + 1], e2 = key[r + 2] - kk[r + 2], e3 = key[r + 3] - kk[r + 3];
          d += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
        }
        for (; r < R; r++) { const float e = key[r] - kk[r]; d += e * e; }
        cands.emplace_back(d, idx);
      }
      std::stable_sort(cands.begin(), cands.end());
      for (int c = 0; c < m->par.num_candidates_from_tree; c++) {
        pairs.push_back(k);
        pairs.push_back(c < (int)cands.size() ? cands[c].second : 0);
      }
      continue;
    }
    std::stable_sort(cands.begin(), cands.end());
    for (int c = 0; c < (int)cands.size() && c < m->par.num_candidates_from_tree; c++) {
      pairs.push_back(k);
      pairs.push_back(cands[c].second);
    }
  }
  const int np = (int)pairs.size() / 2;
  if (np == 0) return CFEAR_OK;
  std::vector<double> dist(np);
  std::vector<int32_t> shift(np);
  const int rc = cfear_sc_distance_batch(ctx, m->d_cur.get(), m->cur_aug, m->d_db.get(), m->n, pairs.data(), np, &m->par.sc, dist.data(),
                                         shift.data());
  if (rc != CFEAR_OK) return rc;
  std::vector<cfear_sc_candidate> similar;
  for (int i = 0; i < np; i++) {                                              // :300-322
    const int k = pairs[2 * i], idx = pairs[2 * i + 1];
    sc_rank_push(similar, m->par, dist[i], shift[i], m->par.odometry_coupled_closure ? m->odom_similarity[idx] : 0.0, idx,
                 m->shifts[k]);
  }
  *n_out = (int32_t)similar.size();
  if ((int)similar.size() > cap) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "%d candidates > cap %d", (int)similar.size(), cap);
  for (size_t i = 0; i < similar.size(); i++) out[i] = similar[i];
  return CFEAR_OK;
}

// ---- whole-graph Scan Context: cfear_sc_local_map_descriptors / cfear_sc_detect_sequence ---------
namespace {
constexpr size_t kScSeqBudget = (size_t)512 << 20;   // device bytes of one query chunk of cfear_sc_detect_sequence
static_assert(sizeof(cfear_sc_node) == 152, "cfear_sc_node is 152 bytes (include/cfear_hip.h)");

int check_sc_nodes(cfear_ctx* ctx, const cfear_sc_node* nodes, int32_t n_nodes, int32_t n_aggregate) {
  if (n_nodes < 0 || (n_nodes > 0 && !nodes)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null nodes");
  if (n_aggregate < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_aggregate must be >= 0");
  for (int i = 0; i < n_nodes; i++) {
    const cfear_sc_cloud& c = nodes[i].cloud;
    if (c.n < 0 || (c.n > 0 && !c.xyzi)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node %d: null cloud", i);
    if (i > 0 && nodes[i].id <= nodes[i - 1].id)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "node %d: ids must increase strictly", i);
  }
  return CFEAR_OK;
}

// NodeExists over [id - n_aggregate, id + n_aggregate] (loopclosure.cpp:553-569): the ids increase, so the members of a
// centre are one range of nodes
int2 sc_members(const cfear_sc_node* nodes, int32_t n_nodes, int32_t center, int32_t n_aggregate) {
  const int64_t lo_id = (int64_t)nodes[center].id - n_aggregate, hi_id = (int64_t)nodes[center].id + n_aggregate;
  int lo = center, hi = center;
  {
    int a = 0, b = center;                           // first node with id >= lo_id
    while (a < b) { const int m = (a + b) / 2; if ((int64_t)nodes[m].id < lo_id) a = m + 1; else b = m; }
    lo = a;
  }
  {
    int a = center, b = n_nodes;                     // first node with id > hi_id
    while (a < b) { const int m = (a + b) / 2; if ((int64_t)nodes[m].id <= hi_id) a = m + 1; else b = m; }
    hi = a - 1;
  }
  return make_int2(lo, hi);
}

// the node table the local-map kernel reads (after carve(): st.cloud resolves staged clouds)
void sc_fill_nodes(const HostStage& st, const cfear_sc_node* nodes, int32_t n_nodes, ScMapNode* h) {
  for (int i = 0; i < n_nodes; i++) {
    h[i].xyzi = st.cloud(nodes[i].cloud.xyzi);
    h[i].n = nodes[i].cloud.n;
    h[i].pad = 0;
    for (int j = 0; j < 8; j++) { h[i].T[j] = nodes[i].T[j]; h[i].Tinv[j] = nodes[i].Tinv[j]; }
  }
}

int sc_local_map_launch(cfear_ctx* ctx, const ScMapArgs& a, int n_centers) {
  const size_t cells = (size_t)a.bin.num_ring * a.bin.num_sector;
  {
    ProfScope ps(ctx, "sc_local_map");
    hipLaunchKernelGGL(sc_local_map_kernel, dim3(n_centers, a.n_aug), dim3(256), cells * 12, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

ScBin sc_bin(const cfear_sc_params* p) {
  return ScBin{p->num_ring, p->num_sector, p->desc_function, p->max_radius, p->desc_divider, p->no_point};
}
}  // namespace

extern "C" int cfear_sc_local_map_descriptors(cfear_ctx* ctx, const cfear_sc_node* nodes, int32_t n_nodes,
                                              const int32_t* centers, int32_t n_centers, int32_t n_aggregate,
                                              const cfear_sc_params* par, const double* shifts_y, int32_t n_aug, double* desc,
                                              double* ringkey, double* sectorkey) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (n_centers < 0 || (n_centers > 0 && (!centers || !desc)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_sc_params(ctx, par));
  if (n_aug < 1 || n_aug > kScMaxAug || (n_aug > 1 && !shifts_y))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_aug must be in [1, %d]", kScMaxAug);
  CFEAR_CHECK(check_sc_nodes(ctx, nodes, n_nodes, n_aggregate));
  for (int c = 0; c < n_centers; c++)
    if (centers[c] < 0 || centers[c] >= n_nodes)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "centre %d: node %d out of range", c, (int)centers[c]);
  if (n_centers == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int R = par->num_ring, S = par->num_sector, cells = R * S;
  const size_t nd = (size_t)n_centers * n_aug;
  const size_t o_center = (size_t)n_nodes * sizeof(ScMapNode), o_mem = o_center + (((size_t)n_centers * 4 + 7) & ~(size_t)7);
  const size_t tab_bytes = o_mem + (size_t)n_centers * sizeof(int2);
  HostStage st(ctx, kWsScSequence);
  for (int i = 0; i < n_nodes; i++) st.cloud_in(nodes[i].cloud.xyzi, nodes[i].cloud.n);
  ScMapArgs a{};
  char* d_tab;
  st.piece(d_tab, tab_bytes);
  st.out(a.desc, desc, nd * cells * sizeof(double));
  st.out(a.ringkey, ringkey, nd * R * sizeof(double));
  if (sectorkey) st.out(a.sectorkey, sectorkey, nd * S * sizeof(double));
  CFEAR_CHECK(st.carve());
  char* h = (char*)st.record(tab_bytes);
  sc_fill_nodes(st, nodes, n_nodes, (ScMapNode*)h);
  memcpy(h + o_center, centers, (size_t)n_centers * 4);
  int2* mem = (int2*)(h + o_mem);
  for (int c = 0; c < n_centers; c++) mem[c] = sc_members(nodes, n_nodes, centers[c], n_aggregate);
  CFEAR_CHECK(st.upload(d_tab, h, tab_bytes));
  a.nodes = (const ScMapNode*)d_tab;
  a.center = (const int32_t*)(d_tab + o_center);
  a.members = (const int2*)(d_tab + o_mem);
  a.bin = sc_bin(par);
  a.n_aug = n_aug;
  for (int k = 0; k < kScMaxAug; k++) a.shift_y[k] = (k < n_aug && shifts_y) ? shifts_y[k] : 0.0;
  CFEAR_CHECK(sc_local_map_launch(ctx, a, n_centers));
  return st.finish();
}

extern "C" int cfear_sc_detect_sequence(cfear_ctx* ctx, const cfear_sc_manager_params* par, const cfear_sc_node* nodes,
                                        int32_t n_nodes, int32_t n_aggregate, int32_t n_detect, cfear_sc_candidate* out,
                                        int32_t* n_out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!par) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null parameters");
  CFEAR_CHECK(check_sc_params(ctx, &par->sc));
  if (par->num_candidates_from_tree < 1 || par->n_candidates < 1 || !(par->odom_sigma_error > 0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad scan-context manager parameters");
  if (par->num_candidates_from_tree > kScMaxTreeK)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "num_candidates_from_tree %d > %d", par->num_candidates_from_tree, kScMaxTreeK);
  CFEAR_CHECK(check_sc_nodes(ctx, nodes, n_nodes, n_aggregate));
  if (n_detect < 0 || n_detect > n_nodes)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_detect %d must be in [0, n_nodes = %d]", (int)n_detect, (int)n_nodes);
  if (n_detect > 0 && (!out || !n_out)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null output");
  if (n_detect > 0 && (cfear_is_device_ptr(out) || cfear_is_device_ptr(n_out)))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "out / n_out must be host memory");
  if (n_detect == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int R = par->sc.num_ring, S = par->sc.num_sector, cells = R * S, K = par->num_candidates_from_tree;
  const int N = n_detect;
  const bool odo = par->odometry_coupled_closure != 0;
  const std::vector<double> shifts = sc_aug_shifts(par->augment_sc != 0);
  const int A = (int)shifts.size();
  // host policy, O(N): segment lengths, recent-node exclusion, the vanilla tree schedule, every (node, augmentation)'s
  // eligible prefix and its place in the pair list
  std::vector<double> seg(N > 1 ? N - 1 : 1);
  auto px = [&](int i) { return nodes[i].T[3]; };
  auto py = [&](int i) { return nodes[i].T[7]; };
  for (int i = 0; i + 1 < N; i++) seg[i] = std::hypot(px(i) - px(i + 1), py(i) - py(i + 1));   // = |p_{i+1} - p_i|: hypot is even
  std::vector<int32_t> n_search((size_t)N * A, 0), pair_off((size_t)N * A, -1);
  std::vector<int> node_pairs(N + 1, 0);             // first pair of each node
  {
    int counter = 0, tree_n = 0;
    int total = 0;
    for (int i = 0; i < N; i++) {
      node_pairs[i] = total;
      const int nex = sc_num_exclude_recent(i, par->distance_exclude_recent, [&](int j) { return seg[j]; });
      if (i + 1 < nex + 1) continue;                 // detectLoopClosureID's gate (:288-291)
      for (int k = 0; k < A; k++) {
        int L, cnt;
        if (odo) { L = std::max(i - 1 - nex, 0); cnt = std::min(L, K); }
        else { sc_tree_step(counter, tree_n, i + 1, nex); L = tree_n; cnt = K; }
        n_search[(size_t)i * A + k] = L;
        if (cnt > 0) { pair_off[(size_t)i * A + k] = total; total += cnt; }
      }
    }
    node_pairs[N] = total;
  }
  const int n_pairs = node_pairs[N];
  // query chunks: the descriptors of the chunk's nodes and augmentations, the odometry terms and the pair list
  const size_t per_node = (size_t)A * cells * 8 + (odo ? (size_t)2 * N * 8 : 0) + (size_t)A * K * (8 + 8 + 4 + 8);
  int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)N, kScSeqBudget / per_node));
  if (ctx->opt[CFEAR_OPT_SC_QUERY_CHUNK] > 0) chunk = (int)std::min<int64_t>(chunk, ctx->opt[CFEAR_OPT_SC_QUERY_CHUNK]);
  int max_chunk_pairs = 1;
  for (int q0 = 0; q0 < N; q0 += chunk) max_chunk_pairs = std::max(max_chunk_pairs, node_pairs[std::min(N, q0 + chunk)] - node_pairs[q0]);
  std::vector<int32_t> h_pairs((size_t)std::max(n_pairs, 1) * 2), h_shift(std::max(n_pairs, 1));
  std::vector<double> h_dist(std::max(n_pairs, 1)), h_psim(std::max(n_pairs, 1));
  // device: tables (uploaded once), database + ring keys of every node, one chunk's working set
  const size_t o_center = (size_t)n_nodes * sizeof(ScMapNode);
  const size_t o_mem = o_center + (((size_t)N * 4 + 15) & ~(size_t)15);
  const size_t o_pos = o_mem + (size_t)N * 8;
  const size_t o_seg = o_pos + (size_t)N * 16;
  const size_t o_ns = o_seg + (size_t)seg.size() * 8;
  const size_t o_po = o_ns + (size_t)N * A * 4;
  const size_t tab_bytes = o_po + (size_t)N * A * 4;
  HostStage st(ctx, kWsScSequence);
  for (int i = 0; i < n_nodes; i++) st.cloud_in(nodes[i].cloud.xyzi, nodes[i].cloud.n);
  char* d_tab;
  double *d_db, *d_rk, *d_q, *d_trav = nullptr, *d_sim = nullptr, *d_dist, *d_psim;
  int32_t *d_pairs, *d_shift;
  st.piece(d_tab, tab_bytes);
  st.piece(d_db, (size_t)N * cells * 8);
  st.piece(d_rk, (size_t)N * A * R * 8);
  st.piece(d_q, (size_t)chunk * A * cells * 8);
  if (odo) { st.piece(d_trav, (size_t)N * chunk * 8); st.piece(d_sim, (size_t)chunk * N * 8); }
  st.piece(d_pairs, (size_t)max_chunk_pairs * 8);
  st.piece(d_dist, (size_t)max_chunk_pairs * 8);
  st.piece(d_shift, (size_t)max_chunk_pairs * 4);
  st.piece(d_psim, (size_t)max_chunk_pairs * 8);
  CFEAR_CHECK(st.carve());
  char* h = (char*)st.record(tab_bytes);
  sc_fill_nodes(st, nodes, n_nodes, (ScMapNode*)h);
  int32_t* hc = (int32_t*)(h + o_center);
  int2* hm = (int2*)(h + o_mem);
  double2* hp = (double2*)(h + o_pos);
  for (int i = 0; i < N; i++) { hc[i] = i; hm[i] = sc_members(nodes, n_nodes, i, n_aggregate); hp[i] = make_double2(px(i), py(i)); }
  memcpy(h + o_seg, seg.data(), seg.size() * 8);
  memcpy(h + o_ns, n_search.data(), (size_t)N * A * 4);
  memcpy(h + o_po, pair_off.data(), (size_t)N * A * 4);
  CFEAR_CHECK(st.upload(d_tab, h, tab_bytes));
  ScMapArgs ma{};
  ma.nodes = (const ScMapNode*)d_tab;
  ma.bin = sc_bin(&par->sc);
  ma.n_aug = A;
  for (int k = 0; k < kScMaxAug; k++) ma.shift_y[k] = k < A ? shifts[k] : 0.0;
  const size_t search_lds = (size_t)K * kScSearchThreads * 8 + (size_t)(R + 1) * 4 + (kScSearchThreads / 64) * 8;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)sc_keysearch_kernel, search_lds));
  for (int q0 = 0; q0 < N; q0 += chunk) {
    const int nq = std::min(chunk, N - q0);
    const int p0 = node_pairs[q0], np = node_pairs[q0 + nq] - p0;
    ma.center = (const int32_t*)(d_tab + o_center) + q0;
    ma.members = (const int2*)(d_tab + o_mem) + q0;
    ma.desc = d_q;
    ma.db = d_db + (size_t)q0 * cells;
    ma.ringkey = d_rk + (size_t)q0 * A * R;
    ma.sectorkey = nullptr;
    CFEAR_CHECK(sc_local_map_launch(ctx, ma, nq));
    if (np == 0) continue;
    if (odo) {
      {
        ProfScope ps(ctx, "sc_odom_terms");
        hipLaunchKernelGGL(sc_travel_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, (const double*)(d_tab + o_seg), q0,
                           nq, d_trav);
        const size_t items = (size_t)nq * (q0 + nq);
        const int blocks = (int)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, (size_t)ctx->n_cu * 16));
        hipLaunchKernelGGL(sc_odom_sim_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const double2*)(d_tab + o_pos), d_trav, q0,
                           nq, N, par->odom_sigma_error, d_sim);
      }
      CFEAR_HIP_CHECK(ctx, hipGetLastError());
    }
    ScSearchArgs sa{};
    sa.ringkey = d_rk;
    sa.sim = d_sim;
    sa.n_search = (const int32_t*)(d_tab + o_ns) + (size_t)q0 * A;
    sa.pair_off = (const int32_t*)(d_tab + o_po) + (size_t)q0 * A;
    sa.pair_base = p0;
    sa.q0 = q0; sa.ld = N; sa.R = R; sa.n_aug = A; sa.k_sel = K; sa.odometry = odo ? 1 : 0;
    sa.pairs = d_pairs;
    sa.pair_sim = d_psim;
    {
      ProfScope ps(ctx, "sc_keysearch");
      hipLaunchKernelGGL(sc_keysearch_kernel, dim3(nq, A), dim3(kScSearchThreads), search_lds, ctx->stream, sa);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    ScDistArgs da{};
    da.desc_q = d_q; da.desc_c = d_db; da.pairs = d_pairs; da.dist = d_dist; da.shift = d_shift;
    CFEAR_CHECK(sc_distance_launch(ctx, da, np, &par->sc));
    // the chunk's buffers are reused by the next chunk: its copies are ordered before that on the stream
    st.fetch(h_pairs.data() + (size_t)2 * p0, d_pairs, (size_t)np * 8);
    st.fetch(h_dist.data() + p0, d_dist, (size_t)np * 8);
    st.fetch(h_shift.data() + p0, d_shift, (size_t)np * 4);
    st.fetch(h_psim.data() + p0, d_psim, (size_t)np * 8);
  }
  CFEAR_CHECK(st.finish());
  // the ranking of every node's pairs, in the streaming loop's visiting order (augmentation, then search rank)
  std::vector<cfear_sc_candidate> similar;
  for (int i = 0; i < N; i++) {
    similar.clear();
    for (int p = node_pairs[i]; p < node_pairs[i + 1]; p++) {
      const int k = h_pairs[2 * (size_t)p] % A;                                // query = (node - q0) * A + k
      sc_rank_push(similar, *par, h_dist[p], h_shift[p], h_psim[p], h_pairs[2 * (size_t)p + 1], shifts[k]);
    }
    n_out[i] = (int32_t)similar.size();
    for (size_t j = 0; j < similar.size(); j++) out[(size_t)i * par->n_candidates + j] = similar[j];
  }
  return CFEAR_OK;
}

// ---- cfear_sc_detect_batch: the same for a batch of graphs, in either descriptor mode, ranked on the device -----------------
namespace {
static_assert(sizeof(cfear_sc_batch) == 96, "cfear_sc_batch is 96 bytes (include/cfear_hip.h)");

// everything the call refuses, decided on the host; ctx may be null.  D: the detected nodes of the whole batch
int check_sc_batch(cfear_ctx* ctx, const cfear_sc_manager_params* par, const cfear_sc_batch* b, const cfear_sc_candidate* out,
                   const int32_t* n_out, int64_t* D) {
  if (!par || !b) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_sc_params(ctx, &par->sc));
  if (par->num_candidates_from_tree < 1 || par->n_candidates < 1 || !(par->odom_sigma_error > 0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad scan-context manager parameters");
  if (par->num_candidates_from_tree > kScMaxTreeK)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "num_candidates_from_tree %d > %d", par->num_candidates_from_tree, kScMaxTreeK);
  if (b->mode != CFEAR_SC_NODES_CLOUD && b->mode != CFEAR_SC_NODES_RAW)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "unknown node mode %d", (int)b->mode);
  const int G = b->n_graphs;
  if (G < 0 || (G > 0 && !b->node_off)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null node_off");
  *D = 0;
  if (G == 0) return CFEAR_OK;
  if (b->node_off[0] != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph 0: node_off[0] must be 0");
  for (int g = 0; g < G; g++) {
    if (b->node_off[g + 1] < b->node_off[g]) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: node_off decreases", g);
    const int n = b->node_off[g + 1] - b->node_off[g], nd = b->n_detect ? b->n_detect[g] : n;
    if (nd < 0 || nd > n)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d: n_detect %d must be in [0, nodes = %d]", g, nd, n);
    *D += nd;
  }
  const int64_t N = b->node_off[G];
  if (N > 0 && !b->T) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null T");
  if (b->ids)
    for (int g = 0; g < G; g++)
      for (int i = b->node_off[g] + 1; i < b->node_off[g + 1]; i++)
        if (b->ids[i] <= b->ids[i - 1])
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: ids must increase strictly", g, i - b->node_off[g]);
  if (b->mode == CFEAR_SC_NODES_CLOUD) {
    if (b->n_aggregate < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_aggregate must be >= 0");
    if (N > 0 && (!b->Tinv || !b->point_off)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null Tinv or point_off");
    if (N > 0 && b->point_off[0] < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph 0, node 0: point_off is negative");
    for (int g = 0; g < G; g++)
      for (int i = b->node_off[g]; i < b->node_off[g + 1]; i++) {
        const int64_t n = b->point_off[i + 1] - b->point_off[i];
        if (n < 0 || n > INT32_MAX)
          return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: point_off decreases (or the cloud is past 2^31 points)",
                                 g, i - b->node_off[g]);
        if (n > 0 && !b->xyzi) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "graph %d, node %d: null cloud", g, i - b->node_off[g]);
      }
  } else {
    if (N > 0 && (!b->imgs || !b->desc || !b->raw)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null sweeps");
    if (N > 0 && b->desc->batch != N)
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "%d sweeps for %lld nodes", (int)b->desc->batch, (long long)N);
  }
  if (*D > INT32_MAX / (kScMaxAug * kScMaxTreeK)) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "%lld detected nodes", (long long)*D);
  if (*D > 0) {
    if (!out || !n_out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null output");
    if (memory_kind({out, n_out}) < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "out and n_out must share host or device memory");
  }
  return CFEAR_OK;
}

// first / last member of the local map of node c of the graph [nb, ne): the ids within n_aggregate of c's
int2 sc_batch_members(const int32_t* ids, int nb, int ne, int c, int n_aggregate) {
  if (!ids) return make_int2((int)std::max<int64_t>(nb, (int64_t)c - n_aggregate), (int)std::min<int64_t>(ne - 1, (int64_t)c + n_aggregate));
  const int64_t lo_id = (int64_t)ids[c] - n_aggregate, hi_id = (int64_t)ids[c] + n_aggregate;
  const int lo = (int)(std::lower_bound(ids + nb, ids + c, lo_id, [](int32_t v, int64_t w) { return (int64_t)v < w; }) - ids);
  const int hi = (int)(std::upper_bound(ids + c, ids + ne, hi_id, [](int64_t w, int32_t v) { return w < (int64_t)v; }) - ids) - 1;
  return make_int2(lo, hi);
}
}  // namespace

extern "C" int cfear_sc_detect_batch(cfear_ctx* ctx, const cfear_sc_manager_params* par, const cfear_sc_batch* batch,
                                     cfear_sc_candidate* out, int32_t* n_out) {
  int64_t D64 = 0;
  const auto t_start = std::chrono::steady_clock::now();
  CFEAR_CHECK(check_sc_batch(ctx, par, batch, out, n_out, &D64));
  if (!ctx) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null context");
  if (D64 == 0) return CFEAR_OK;
  const cfear_sc_batch& b = *batch;
  const bool raw = b.mode == CFEAR_SC_NODES_RAW, odo = par->odometry_coupled_closure != 0;
  const int G = b.n_graphs, N = b.node_off[G], D = (int)D64;
  const int R = par->sc.num_ring, S = par->sc.num_sector, cells = R * S, K = par->num_candidates_from_tree;
  const std::vector<double> shifts = sc_aug_shifts(!raw && par->augment_sc != 0);
  const int A = (int)shifts.size();
  // one table for the whole batch (uploaded once): the node records of the local maps, then the per-query arrays
  size_t tab_bytes = 0;
  auto take = [&](size_t bytes) { const size_t o = tab_bytes; tab_bytes = (tab_bytes + bytes + 15) & ~(size_t)15; return o; };
  const size_t o_nodes = take(raw ? 0 : (size_t)N * sizeof(ScMapNode)), o_first = take((size_t)D * 4), o_dbb = take((size_t)D * 4),
               o_center = take((size_t)D * 4), o_mem = take((size_t)D * 8), o_row = take((size_t)(D + 1) * 8),
               o_pos = take((size_t)D * 16), o_seg = take((size_t)D * 8), o_ns = take((size_t)D * A * 4),
               o_po = take((size_t)D * A * 4), o_np = take((size_t)(D + 1) * 4);
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsScSequence);
  char* h = (char*)st.record(tab_bytes);
  int32_t *h_first = (int32_t*)(h + o_first), *h_dbb = (int32_t*)(h + o_dbb), *h_center = (int32_t*)(h + o_center);
  int2* h_mem = (int2*)(h + o_mem);
  long long* h_row = (long long*)(h + o_row);
  double2* h_pos = (double2*)(h + o_pos);
  double* h_seg = (double*)(h + o_seg);
  int32_t *h_ns = (int32_t*)(h + o_ns), *h_po = (int32_t*)(h + o_po), *h_np = (int32_t*)(h + o_np);
  // host policy, O(nodes), per graph: segment lengths, recent-node exclusion, the vanilla tree schedule (a counter and a
  // tree per graph), every (query, augmentation)'s eligible prefix and its place in the pair list
  // CFEAR_OPT_HOST_TIMELINE = 1: where the host spends the call, one line on stderr
  double t_ms[5] = {0, 0, 0, 0, 0};
  auto t_last = t_start;
  auto lap = [&](int i) {
    const auto now = std::chrono::steady_clock::now();
    t_ms[i] += std::chrono::duration<double, std::milli>(now - t_last).count();
    t_last = now;
  };
  int total = 0, max_len = 0;
  {
    int d0 = 0;
    h_row[0] = 0;
    for (int g = 0; g < G; g++) {
      const int nb = b.node_off[g], ne = b.node_off[g + 1], nd = b.n_detect ? b.n_detect[g] : ne - nb;
      auto px = [&](int i) { return b.T[(size_t)(nb + i) * 8 + 3]; };
      auto py = [&](int i) { return b.T[(size_t)(nb + i) * 8 + 7]; };
      for (int i = 0; i + 1 < nd; i++) h_seg[d0 + i] = std::hypot(px(i) - px(i + 1), py(i) - py(i + 1));
      int counter = 0, tree_n = 0;
      for (int i = 0; i < nd; i++) {
        const int d = d0 + i;
        h_first[d] = d0;
        h_dbb[d] = raw ? nb : d0;
        h_center[d] = nb + i;
        if (!raw) h_mem[d] = sc_batch_members(b.ids, nb, ne, nb + i, b.n_aggregate);
        h_pos[d] = make_double2(px(i), py(i));
        h_row[d + 1] = h_row[d] + (odo ? i : 0);
        h_np[d] = total;
        for (int k = 0; k < A; k++) { h_ns[(size_t)d * A + k] = 0; h_po[(size_t)d * A + k] = -1; }
        const int nex = sc_num_exclude_recent(i, par->distance_exclude_recent, [&](int j) { return h_seg[d0 + j]; });
        if (i + 1 < nex + 1) continue;               // detectLoopClosureID's gate (:288-291)
        for (int k = 0; k < A; k++) {
          int L, cnt;
          if (odo) { L = std::max(i - 1 - nex, 0); cnt = std::min(L, K); }
          else { sc_tree_step(counter, tree_n, i + 1, nex); L = tree_n; cnt = K; }
          h_ns[(size_t)d * A + k] = L;
          if (cnt > 0) { h_po[(size_t)d * A + k] = total; total += cnt; }
        }
      }
      max_len = std::max(max_len, nd);
      d0 += nd;
    }
    h_np[D] = total;
  }
  lap(0);
  // query chunks of the concatenated list: the chunk's query descriptors, its packed odometry rows and its pair list
  const size_t per_query = (raw ? 0 : (size_t)A * cells * 8) + (odo ? (size_t)2 * max_len * 8 : 0) + (size_t)A * K * (8 + 8 + 4 + 8);
  int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)D, kScSeqBudget / per_query));
  if (ctx->opt[CFEAR_OPT_SC_QUERY_CHUNK] > 0) chunk = (int)std::min<int64_t>(chunk, ctx->opt[CFEAR_OPT_SC_QUERY_CHUNK]);
  int max_chunk_pairs = 1;
  long long max_rows = 1;
  for (int q0 = 0; q0 < D; q0 += chunk) {
    const int q1 = std::min(D, q0 + chunk);
    max_chunk_pairs = std::max(max_chunk_pairs, h_np[q1] - h_np[q0]);
    max_rows = std::max(max_rows, h_row[q1] - h_row[q0]);
  }
  const size_t n_db = raw ? (size_t)N : (size_t)D;   // raw mode describes every sweep in one launch, cloud mode the detected nodes
  const size_t nc = (size_t)par->n_candidates;
  char* d_tab;
  const float* d_xyzi = nullptr;
  double *d_db, *d_rk, *d_q = nullptr, *d_trav = nullptr, *d_sim = nullptr, *d_dist, *d_psim;
  int32_t *d_pairs, *d_shift, *d_nout;
  cfear_sc_candidate* d_out;
  if (!raw) st.in(d_xyzi, b.xyzi, (size_t)b.point_off[N] * 16);
  st.piece(d_tab, tab_bytes);
  st.piece(d_db, n_db * cells * 8);
  st.piece(d_rk, (size_t)D * A * R * 8);
  if (!raw) st.piece(d_q, (size_t)chunk * A * cells * 8);
  if (odo) { st.piece(d_trav, (size_t)max_rows * 8); st.piece(d_sim, (size_t)max_rows * 8); }
  st.piece(d_pairs, (size_t)max_chunk_pairs * 8);
  st.piece(d_dist, (size_t)max_chunk_pairs * 8);
  st.piece(d_shift, (size_t)max_chunk_pairs * 4);
  st.piece(d_psim, (size_t)max_chunk_pairs * 8);
  st.out(d_out, out, (size_t)D * nc * sizeof(cfear_sc_candidate));   // device rows are written in place
  st.out(d_nout, n_out, (size_t)D * 4);
  CFEAR_CHECK(st.carve());
  lap(1);
  // raw mode: every sweep's descriptor, straight into the database; what cfear_sc_raw_descriptors refuses is refused here,
  // before the first launch of this call
  if (raw) CFEAR_CHECK(cfear_sc_raw_descriptors(ctx, b.imgs, b.desc, &par->sc, b.raw, d_db, nullptr, nullptr));
  if (!raw) {
    ScMapNode* hn = (ScMapNode*)(h + o_nodes);
    for (int i = 0; i < N; i++) {
      hn[i].xyzi = (const float4*)d_xyzi + b.point_off[i];
      hn[i].n = (int32_t)(b.point_off[i + 1] - b.point_off[i]);
      hn[i].pad = 0;
      memcpy(hn[i].T, b.T + (size_t)i * 8, 64);
      memcpy(hn[i].Tinv, b.Tinv + (size_t)i * 8, 64);
    }
  }
  CFEAR_CHECK(st.upload(d_tab, h, tab_bytes));
  lap(2);
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(d_out, 0, (size_t)D * nc * sizeof(cfear_sc_candidate), ctx->stream));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(d_nout, 0, (size_t)D * 4, ctx->stream));
  ScBatchTab tb{};
  tb.first = (const int32_t*)(d_tab + o_first); tb.db_base = (const int32_t*)(d_tab + o_dbb);
  tb.center = (const int32_t*)(d_tab + o_center); tb.row_off = (const long long*)(d_tab + o_row);
  tb.pos = (const double2*)(d_tab + o_pos); tb.seg = (const double*)(d_tab + o_seg);
  tb.n_search = (const int32_t*)(d_tab + o_ns); tb.pair_off = (const int32_t*)(d_tab + o_po);
  tb.node_pairs = (const int32_t*)(d_tab + o_np);
  ScMapArgs ma{};
  ma.nodes = (const ScMapNode*)(d_tab + o_nodes);
  ma.bin = sc_bin(&par->sc);
  ma.n_aug = A;
  for (int k = 0; k < kScMaxAug; k++) ma.shift_y[k] = k < A ? shifts[k] : 0.0;
  if (raw) {
    {
      ProfScope ps(ctx, "sc_raw_keys");
      hipLaunchKernelGGL(sc_batch_raw_keys_kernel, dim3(D), dim3(256), 0, ctx->stream, d_db, tb, R, S, d_rk);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  const size_t search_lds = (size_t)K * kScSearchThreads * 8 + (size_t)(R + 1) * 4 + (kScSearchThreads / 64) * 8;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)sc_batch_keysearch_kernel, search_lds));
  for (int q0 = 0; q0 < D; q0 += chunk) {
    const int nq = std::min(chunk, D - q0);
    const int p0 = h_np[q0], np = h_np[q0 + nq] - p0;
    if (!raw) {
      ma.center = tb.center + q0;
      ma.members = (const int2*)(d_tab + o_mem) + q0;
      ma.desc = d_q;
      ma.db = d_db + (size_t)q0 * cells;
      ma.ringkey = d_rk + (size_t)q0 * A * R;
      ma.sectorkey = nullptr;
      CFEAR_CHECK(sc_local_map_launch(ctx, ma, nq));
    }
    if (np == 0) continue;
    if (odo) {
      {
        ProfScope ps(ctx, "sc_odom_terms");
        hipLaunchKernelGGL(sc_batch_travel_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, tb, q0, nq, d_trav);
        hipLaunchKernelGGL(sc_batch_odom_sim_kernel, dim3(nq), dim3(256), 0, ctx->stream, tb, (const double*)d_trav, q0,
                           par->odom_sigma_error, d_sim);
      }
      CFEAR_HIP_CHECK(ctx, hipGetLastError());
    }
    ScBatchSearchArgs sa{};
    sa.tb = tb;
    sa.ringkey = d_rk;
    sa.sim = d_sim;
    sa.pair_base = p0;
    sa.q0 = q0; sa.R = R; sa.n_aug = A; sa.k_sel = K; sa.odometry = odo ? 1 : 0; sa.query_is_node = raw ? 1 : 0;
    sa.pairs = d_pairs;
    sa.pair_sim = d_psim;
    {
      ProfScope ps(ctx, "sc_keysearch");
      hipLaunchKernelGGL(sc_batch_keysearch_kernel, dim3(nq, A), dim3(kScSearchThreads), search_lds, ctx->stream, sa);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    ScDistArgs da{};
    da.desc_q = raw ? d_db : d_q; da.desc_c = d_db; da.pairs = d_pairs; da.dist = d_dist; da.shift = d_shift;
    CFEAR_CHECK(sc_distance_launch(ctx, da, np, &par->sc));
    ScRankArgs ra{};
    ra.tb = tb;
    ra.pairs = d_pairs; ra.dist = d_dist; ra.shift = d_shift; ra.pair_sim = d_psim;
    ra.pair_base = p0; ra.q0 = q0; ra.nq = nq; ra.n_aug = A; ra.n_candidates = par->n_candidates; ra.odometry = odo ? 1 : 0;
    ra.unit = 360.0 / (double)S;
    for (int k = 0; k < kScMaxAug; k++) ra.shift_y[k] = k < A ? shifts[k] : 0.0;
    ra.out = d_out; ra.n_out = d_nout;
    {
      ProfScope ps(ctx, "sc_rank");
      hipLaunchKernelGGL(sc_rank_kernel, dim3((nq + 3) / 4), dim3(256), 0, ctx->stream, ra);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  lap(3);
  const int rc = st.finish();
  lap(4);
  if (ctx->opt[CFEAR_OPT_HOST_TIMELINE])
    fprintf(stderr, "cfear_sc_detect_batch host timeline: %d graphs, %d detected nodes, %d pairs, %d-query chunks: checks + policy tables %.3f ms, "
            "workspace + staged inputs %.3f ms, node table + upload %.3f ms, launches %.3f ms, drain + read-back %.3f ms\n",
            G, D, total, chunk, t_ms[0], t_ms[1], t_ms[2], t_ms[3], t_ms[4]);
  return rc;
}
