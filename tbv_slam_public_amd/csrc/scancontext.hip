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
#include <cmath>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kScMaxCells = 5120;        // ring x sector capacity of the LDS accumulators (reference: 40 x 120)
constexpr int kScDistThreads = 1024;     // one distance workgroup per CU (two descriptors = 77 KB of LDS): wide blocks
constexpr int kScMaxAug = 8;

struct ScCloud { const float4* xyzi; int32_t n; int32_t pad; };

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

__global__ __launch_bounds__(256) void sc_descriptor_kernel(const ScDescArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int R = a.num_ring, S = a.num_sector, cells = R * S;
  double* acc = (double*)smem;                       // [cells] sum
  int* hit = (int*)(acc + cells);                    // [cells] count (sum) / float-ordered max (max)
  const ScCloud cl = a.clouds[blockIdx.x];
  const double shift_y = a.shift_y[blockIdx.y];
  for (int i = threadIdx.x; i < cells; i += blockDim.x) { acc[i] = 0.0; hit[i] = a.desc_function == 0 ? 0 : (int)0x80000000; }
  __syncthreads();
  for (int k = threadIdx.x; k < cl.n; k += blockDim.x) {
    const float4 p = cl.xyzi[k];
    float px = p.x, py = p.y;
    if (shift_y != 0.0) {                            // pcl::transformPointCloud with an identity rotation (:163-170)
      px = (float)(((1.0 * (double)p.x + 0.0 * (double)p.y) + 0.0 * (double)p.z) + 0.0);
      py = (float)(((0.0 * (double)p.x + 1.0 * (double)p.y) + 0.0 * (double)p.z) + shift_y);
    }
    const float azim_range = sqrtf(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)));
    const float azim_angle = sc_xy2theta(px, py);
    if ((double)azim_range > a.max_radius) continue;
    const double rr = ceil(((double)azim_range / a.max_radius) * R), ss = ceil(((double)azim_angle / 360.0) * S);
    const int ring_idx = max(min(R, rr == rr ? (int)rr : 1), 1);
    const int sctor_idx = max(min(S, ss == ss ? (int)ss : 1), 1);
    const int cell = (ring_idx - 1) * S + (sctor_idx - 1);
    if (a.desc_function == 0) {
      atomicAdd(&acc[cell], (double)p.w);
      atomicAdd(&hit[cell], 1);
    } else {                                         // max: order-preserving int image of the float intensity
      int u = __float_as_int(p.w);
      u = u >= 0 ? u : (u ^ 0x7fffffff);
      atomicMax(&hit[cell], u);
    }
  }
  __syncthreads();
  const int NO_POINT = -1000;
  double* out = a.desc + ((size_t)blockIdx.x * a.n_aug + blockIdx.y) * cells;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    double d;
    if (a.desc_function == 0) d = hit[i] > 0 ? acc[i] : (double)NO_POINT;
    else {
      const int u = hit[i];
      d = u == (int)0x80000000 ? (double)NO_POINT : (double)__int_as_float(u >= 0 ? u : (u ^ 0x7fffffff));
    }
    d = d / a.desc_divider;                          // "Divison before no_point check" (:113)
    if (d == NO_POINT) d = a.no_point;
    acc[i] = d;
    out[i] = d;
  }
  __syncthreads();
  double* rk = a.ringkey + ((size_t)blockIdx.x * a.n_aug + blockIdx.y) * R;
  double* sk = a.sectorkey + ((size_t)blockIdx.x * a.n_aug + blockIdx.y) * S;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {  // row means, sequential like Eigen's row.mean() restatement
    double s = 0;
    for (int c = 0; c < S; c++) s += acc[r * S + c];
    rk[r] = s / S;
  }
  for (int c = threadIdx.x; c < S; c += blockDim.x) {
    double s = 0;
    for (int r = 0; r < R; r++) s += acc[r * S + c];
    sk[c] = s / R;
  }
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
  int* ctl = (int*)(tmp + S);          // [2 + 2 * S] argmin, count, search space
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

int check_sc_params(cfear_ctx* ctx, const cfear_sc_params* p) {
  if (!p) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null parameters");
  if (p->num_ring < 1 || p->num_sector < 1 || (long long)p->num_ring * p->num_sector > kScMaxCells)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "num_ring x num_sector must be in [1, %d]", kScMaxCells);
  if (!(p->max_radius > 0) || p->desc_divider == 0.0 || p->desc_function < 0 || p->desc_function > 1)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad scan-context parameters");
  return CFEAR_OK;
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
  a.num_ring = R; a.num_sector = S; a.search_ratio = par->search_ratio;
  const size_t base = (((size_t)2 * cells + 5 * S) * 8 + (size_t)(2 + 2 * S + 2) * 4 + 16 + 15) & ~(size_t)15;
  const int m_max = 2 * (int)std::round(0.5 * par->search_ratio * S) + 1;
  const size_t room = base < (size_t)156 * 1024 ? ((size_t)156 * 1024 - base) / ((size_t)S * 8) : 0;
  // tmp[] holds one distance per shift of a chunk (<= S); one thread sums each shift (<= block size)
  a.chunk = (int)std::max<size_t>(1, std::min<size_t>({room, (size_t)m_max, (size_t)256, (size_t)S}));
  a.sim_off = (uint32_t)base;
  const size_t lds = base + (size_t)a.chunk * S * 8;
  { const int rc_lds = cfear_allow_lds(ctx, (const void*)sc_distance_kernel, 160 * 1024); if (rc_lds != CFEAR_OK) return rc_lds; }
  {
    ProfScope ps(ctx, "sc_distance");
    hipLaunchKernelGGL(sc_distance_kernel, dim3(n_pairs), dim3(kScDistThreads), lds, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
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
  double* d_db = nullptr;        // [cap][cells]
  int cap = 0, n = 0;
  double* d_cur = nullptr;       // [n_aug][cells] current node and its augmentations
  int n_aug = 1;
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
  cfear_sc_manager* m = new cfear_sc_manager();
  m->ctx = ctx; m->par = *par;
  m->cells = par->sc.num_ring * par->sc.num_sector;
  m->shifts = {0.0};
  if (par->augment_sc) { m->shifts.push_back(-2.0); m->shifts.push_back(2.0); m->shifts.push_back(-4.0); m->shifts.push_back(4.0); }   // :164
  m->n_aug = (int)m->shifts.size();
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (hipMalloc((void**)&m->d_cur, (size_t)m->n_aug * m->cells * sizeof(double)) != hipSuccess) {
    delete m;
    return cfear_set_error(ctx, CFEAR_ERR_HIP, "hipMalloc failed");
  }
  *out = m;
  return CFEAR_OK;
}

extern "C" int cfear_sc_manager_destroy(cfear_sc_manager* m) {
  if (!m) return CFEAR_OK;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->d_db) (void)hipFree(m->d_db);
  if (m->d_cur) (void)hipFree(m->d_cur);
  delete m;
  return CFEAR_OK;
}

extern "C" int cfear_sc_manager_size(const cfear_sc_manager* m) { return m ? m->n : CFEAR_ERR_INVALID_ARGUMENT; }

extern "C" int cfear_sc_manager_add(cfear_sc_manager* m, const float* xyzi, int32_t n_points, const double Todom[3]) {
  if (!m || !Todom || n_points < 0 || (n_points > 0 && !xyzi)) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = m->ctx;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int R = m->par.sc.num_ring;
  cfear_sc_cloud cloud{xyzi, n_points, 0};
  std::vector<double> rk((size_t)m->n_aug * R);
  int rc = cfear_sc_descriptors(ctx, &cloud, 1, &m->par.sc, m->shifts.data(), m->n_aug, m->d_cur, rk.data(), nullptr);
  if (rc != CFEAR_OK) return rc;
  if (m->n == m->cap) {                                      // grow the database (device to device)
    const int ncap = std::max(256, m->cap * 2);
    double* nd = nullptr;
    if (hipMalloc((void**)&nd, (size_t)ncap * m->cells * sizeof(double)) != hipSuccess)
      return cfear_set_error(ctx, CFEAR_ERR_HIP, "descriptor database: hipMalloc failed");
    if (m->n > 0)
      CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(nd, m->d_db, (size_t)m->n * m->cells * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    CFEAR_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (m->d_db) (void)hipFree(m->d_db);
    m->d_db = nd;
    m->cap = ncap;
  }
  CFEAR_HIP_CHECK(ctx, hipMemcpyAsync(m->d_db + (size_t)m->n * m->cells, m->d_cur, (size_t)m->cells * sizeof(double),
                                      hipMemcpyDeviceToDevice, ctx->stream));
  m->n++;
  m->cur_keys.assign(m->n_aug, std::vector<float>(R));
  for (int k = 0; k < m->n_aug; k++)
    for (int r = 0; r < R; r++) m->cur_keys[k][r] = (float)rk[(size_t)k * R + r];      // eig2stdvec: double -> float
  m->ringkeys.push_back(m->cur_keys[0]);
  // ExcludeAndUpdateLikelihood (:181-222)
  m->poses.insert(m->poses.end(), Todom, Todom + 3);
  const int np = (int)m->poses.size() / 3;
  auto px = [&](int i) { return m->poses[3 * (size_t)i]; };
  auto py = [&](int i) { return m->poses[3 * (size_t)i + 1]; };
  if (np <= 2) {
    m->num_exclude_recent = 2;
  } else {
    double distance = 0.0;
    int n_ex = 0, prev = np - 1;
    for (int i = np - 1; i >= 0 && distance < m->par.distance_exclude_recent; i--) {
      distance = distance + std::hypot(px(i) - px(prev), py(i) - py(prev));
      prev = i;
      n_ex++;
    }
    m->num_exclude_recent = n_ex;
  }
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

extern "C" int cfear_sc_manager_detect(cfear_sc_manager* m, cfear_sc_candidate* out, int32_t cap, int32_t* n_out) {
  if (!m || !n_out || cap < 0 || (cap > 0 && !out)) return CFEAR_ERR_INVALID_ARGUMENT;
  cfear_ctx* ctx = m->ctx;
  *n_out = 0;
  if (m->n < m->num_exclude_recent + 1) return CFEAR_OK;                      // :288-291
  const int R = m->par.sc.num_ring;
  const int cur = m->n - 1;
  std::vector<int32_t> pairs;                                                 // (augmentation, candidate) in visiting order
  for (int k = 0; k < m->n_aug; k++) {
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
      if (m->tree_making_period_counter % 50 == 0) m->tree_n = std::max(m->n - m->num_exclude_recent, 0);
      m->tree_making_period_counter++;
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
  const int rc = cfear_sc_distance_batch(ctx, m->d_cur, m->n_aug, m->d_db, m->n, pairs.data(), np, &m->par.sc, dist.data(),
                                         shift.data());
  if (rc != CFEAR_OK) return rc;
  const double unit = 360.0 / (double)m->par.sc.num_sector;
  std::vector<cfear_sc_candidate> similar;
  for (int i = 0; i < np; i++) {                                              // :300-322
    const int k = pairs[2 * i], idx = pairs[2 * i + 1];
    cfear_sc_candidate c{};
    c.min_dist_sc = dist[i];
    c.min_dist_odom = m->par.odometry_coupled_closure ? m->odom_similarity[idx] : 0.0;
    c.min_dist = m->par.odometry_coupled_closure ? dist[i] + c.min_dist_odom : dist[i];
    const float ang = (float)(shift[i] * unit);
    c.yaw_diff_rad = (float)(ang * M_PI / 180.0);
    c.nn_idx = idx;
    c.argmin_shift = shift[i];
    c.Taug[0] = 0.0; c.Taug[1] = m->shifts[k]; c.Taug[2] = 0.0;
    similar.push_back(c);
    std::stable_sort(similar.begin(), similar.end(),
                     [](const cfear_sc_candidate& a, const cfear_sc_candidate& b) { return a.min_dist < b.min_dist; });
    if ((int)similar.size() > m->par.n_candidates) similar.pop_back();
  }
  *n_out = (int32_t)similar.size();
  if ((int)similar.size() > cap) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "%d candidates > cap %d", (int)similar.size(), cap);
  for (size_t i = 0; i < similar.size(); i++) out[i] = similar[i];
  return CFEAR_OK;
}
