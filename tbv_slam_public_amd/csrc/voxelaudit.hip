// voxelaudit.hip -- which scans hang on the in-voxel summation order of pcl::VoxelGrid: a diagnostic,
// not a stage.
//
// PCL sorts (voxel, point) pairs with an unstable std::sort and sums every voxel's points sequentially in float
// (pointnormal.cpp:277-280); the surface kernels pin input order.  Per scan the audit encloses the float centroid of EVERY
// order of every voxel, classifies each (voxel, point) pair against the radius test with that enclosure, and keeps a
// witness: the centroid summed last to first.
//   voxel_leaders_kernel  one workgroup per scan: bounding box, the first point of every voxel key (its leader), compacted
//   voxel_audit_kernel    one workgroup per scan, a thread per voxel: sums forward and backward, enclosure, pair classes
// Brute force over LDS tiles of the cloud, and none of surface.hip or gridsort.hpp: an audit that reused the sort it audits
// would inherit its order.  Everything a record holds is an integer sum or a maximum, so it does not depend on the batch.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kVaThreads = 256;
constexpr int kVaTile = CFEAR_VOXEL_AUDIT_TILE;           // points per LDS tile (16 KB)
constexpr int kVaMaxPoints = CFEAR_VOXEL_AUDIT_MAX_POINTS;
constexpr float kVaMaxIndex = 8388608.f;                  // 2^23: voxel indices up to here are exact in float
static_assert(kVaTile % kVaThreads == 0, "a tile is staged by whole workgroups");

// One scan as the host describes it (point offsets into xyzi, into the leader scratch, into the voxel table) ...
struct VaIn {
  int64_t off, scr, voff;
  int32_t n, status;                                      // status: what the host already knows (empty, over capacity)
};
// ... and as voxel_leaders_kernel found it
struct VaScan {
  int32_t status, n_vox, min_bx, min_by, div_bx, pad;
};
struct VaGrid {
  float inv_leaf;
  int min_bx, min_by, div_bx;
};
struct __align__(16) VaPoint {
  float x, y;
  uint32_t key, lead;
};

// pcl::VoxelGrid's key (oracle/cfear_oracle.cpp::voxel_grid): floor in float, minus the box's corner in float
__device__ __forceinline__ uint32_t va_key(const float x, const float y, const VaGrid& g) {
  const int ijk0 = (int)(floorf(x * g.inv_leaf) - (float)g.min_bx);
  const int ijk1 = (int)(floorf(y * g.inv_leaf) - (float)g.min_by);
  return (uint32_t)(ijk0 + ijk1 * g.div_bx);
}

// lanes without a source keep their own value: the identity of min and max
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float va_dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
template <bool MAX>
__device__ __forceinline__ float va_wave_minmax(float v) {
  auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); };
  v = op(v, va_dpp_f32<0x111>(v));                        // row_shr:1, 2, 4, 8, then the row totals (common.hpp)
  v = op(v, va_dpp_f32<0x112>(v));
  v = op(v, va_dpp_f32<0x114>(v));
  v = op(v, va_dpp_f32<0x118>(v));
  v = op(v, va_dpp_f32<0x142, 0xa>(v));
  v = op(v, va_dpp_f32<0x143, 0xc>(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// maximum of non-negative doubles over the wavefront
__device__ __forceinline__ double va_wave_max_f64(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  v = fmax(v, dpp_f64<0x140>(v));
  return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)), fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// points [t0, t0 + m) of the scan into the tile, with their keys and, where `lead` is given, their leader flags
__device__ __forceinline__ void va_stage(VaPoint* tile, const float* pts, const uint8_t* lead, const int t0, const int m, const VaGrid& g) {
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += kVaThreads) {
    const g_f32x2 p = gload<g_f32x2>(pts + 4 * (size_t)(t0 + j));
    VaPoint q;
    q.x = p.x; q.y = p.y;
    q.key = va_key(p.x, p.y, g);
    q.lead = lead ? (uint32_t)gload<uint8_t>(lead + t0 + j) : 0u;
    tile[j] = q;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kVaThreads) void voxel_leaders_kernel(const float* __restrict__ xyzi, const VaIn* __restrict__ ins, const int n_scans,
                                                                   const float inv_leaf, VaScan* __restrict__ scans, int32_t* __restrict__ leaders,
                                                                   uint8_t* __restrict__ lead_flag) {
  __shared__ VaPoint tile[kVaTile];
  __shared__ float red[4][4];
  __shared__ int wsum[4];
  __shared__ int bad;
  const int s = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
  if (s >= n_scans) return;
  const VaIn in = ins[s];
  VaScan out = {in.status, 0, 0, 0, 0, 0};
  if (in.status != CFEAR_OK) {                             // (block-uniform)
    if (tid == 0) scans[s] = out;
    return;
  }
  const int n = in.n;
  const float* pts = xyzi + 4 * in.off;
  // bounding box, and whether every coordinate is finite
  if (tid == 0) bad = 0;
  float mnx = FLT_MAX, mny = FLT_MAX, mxx = -FLT_MAX, mxy = -FLT_MAX;
  bool finite = true;
  for (int i = tid; i < n; i += kVaThreads) {
    const g_f32x2 p = gload<g_f32x2>(pts + 4 * (size_t)i);
    finite = finite && isfinite(p.x) && isfinite(p.y);
    mnx = fminf(mnx, p.x); mxx = fmaxf(mxx, p.x);
    mny = fminf(mny, p.y); mxy = fmaxf(mxy, p.y);
  }
  mnx = va_wave_minmax<false>(mnx); mny = va_wave_minmax<false>(mny);
  mxx = va_wave_minmax<true>(mxx); mxy = va_wave_minmax<true>(mxy);
  __syncthreads();
  if ((tid & 63) == 0) { red[w][0] = mnx; red[w][1] = mny; red[w][2] = mxx; red[w][3] = mxy; }
  if (!finite) bad = 1;
  __syncthreads();
  mnx = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
  mny = fminf(fminf(red[0][1], red[1][1]), fminf(red[2][1], red[3][1]));
  mxx = fmaxf(fmaxf(red[0][2], red[1][2]), fmaxf(red[2][2], red[3][2]));
  mxy = fmaxf(fmaxf(red[0][3], red[1][3]), fmaxf(red[2][3], red[3][3]));
  if (bad) {
    out.status = CFEAR_ERR_INVALID_ARGUMENT;
    if (tid == 0) scans[s] = out;
    return;
  }
  const float f0 = floorf(mnx * inv_leaf), f1 = floorf(mxx * inv_leaf), f2 = floorf(mny * inv_leaf), f3 = floorf(mxy * inv_leaf);
  const bool fits = fabsf(f0) <= kVaMaxIndex && fabsf(f1) <= kVaMaxIndex && fabsf(f2) <= kVaMaxIndex && fabsf(f3) <= kVaMaxIndex;
  VaGrid g = {inv_leaf, 0, 0, 1};
  if (fits) { g.min_bx = (int)f0; g.min_by = (int)f2; g.div_bx = (int)f1 - (int)f0 + 1; }
  if (!fits || (int64_t)g.div_bx * (int64_t)((int)f3 - g.min_by + 1) > 2147483647ll) {
    out.status = CFEAR_ERR_CAPACITY;
    if (tid == 0) scans[s] = out;
    return;
  }
  // leaders: point i leads its voxel if no point before it has its key.  This thread's points: tid, tid + 256, ...
  const uint32_t* tkey = &tile[0].key;
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += kVaThreads) {
    const int i = i0 + tid, end = min(n, i0 + kVaThreads);
    const bool live = i < n;
    uint32_t key = 0;
    if (live) { const g_f32x2 p = gload<g_f32x2>(pts + 4 * (size_t)i); key = va_key(p.x, p.y, g); }
    bool dup = false;
    for (int t0 = 0; t0 < end; t0 += kVaTile) {
      const int m = min(kVaTile, end - t0);
      va_stage(tile, pts, nullptr, t0, m, g);
      const int lim = live ? min(m, i - t0) : 0;
      for (int j = 0; j < lim; j++) dup = dup || tkey[4 * j] == key;
    }
    const int flag = live && !dup;
    const int incl = wave_incl_scan_i32(flag);
    __syncthreads();                                       // the previous chunk's readers are done with wsum
    if ((tid & 63) == 63) wsum[w] = incl;
    __syncthreads();
    int before = base;
    for (int k = 0; k < w; k++) before += wsum[k];
    if (flag) leaders[in.scr + before + incl - 1] = i;
    if (live) lead_flag[in.scr + i] = (uint8_t)flag;
    base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
  }
  out.n_vox = base; out.min_bx = g.min_bx; out.min_by = g.min_by; out.div_bx = g.div_bx;
  if (tid == 0) scans[s] = out;
}

__global__ __launch_bounds__(kVaThreads) void voxel_audit_kernel(const float* __restrict__ xyzi, const VaIn* __restrict__ ins,
                                                                 const VaScan* __restrict__ scans, const int n_scans, const float inv_leaf,
                                                                 const float r2, const int32_t* __restrict__ leaders,
                                                                 const uint8_t* __restrict__ lead_flag, cfear_voxel_audit_record* __restrict__ records,
                                                                 cfear_voxel_audit_voxel* __restrict__ voxels, const int64_t voxel_cap) {
  __shared__ VaPoint tile[kVaTile];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (s >= n_scans) return;
  const VaIn in = ins[s];
  const VaScan sc = scans[s];
  cfear_voxel_audit_record* rec = records + s;             // zeroed on the stream before the launch
  if (tid == 0) { rec->status = sc.status; rec->n_points = in.n; rec->n_voxels = sc.n_vox; }
  if (sc.status != CFEAR_OK) return;                       // (block-uniform)
  const int n = in.n, n_vox = sc.n_vox;
  const float* pts = xyzi + 4 * in.off;
  const uint8_t* flags = lead_flag + in.scr;
  const VaGrid g = {inv_leaf, sc.min_bx, sc.min_by, sc.div_bx};
  const double u = 0x1p-24, r2d = (double)r2;
  const int n_tiles = (n + kVaTile - 1) / kVaTile;
  int c_differ = 0, c_pairs = 0, c_exposed = 0, c_thr = 0, c_changed = 0, c_maxpts = 0;
  double c_maxe = 0.0;
  for (int v0 = 0; v0 < n_vox; v0 += kVaThreads) {         // this thread's voxels: leaders tid, tid + 256, ...
    const int v = v0 + tid;
    const bool live = v < n_vox;
    uint32_t key = 0xffffffffu;                            // (no voxel has it: keys stay below 2^31)
    if (live) {
      const g_f32x2 p = gload<g_f32x2>(pts + 4 * (size_t)gload<int32_t>(leaders + in.scr + v));
      key = va_key(p.x, p.y, g);
    }
    // first to last: the float sums of this library's order, S and A of the enclosure, the voxel's rank among the keys
    float fx = 0.f, fy = 0.f;
    double Sx = 0.0, Sy = 0.0, Ax = 0.0, Ay = 0.0;
    int cnt = 0, rank = 0;
    for (int t = 0; t < n_tiles; t++) {
      const int t0 = t * kVaTile, m = min(kVaTile, n - t0);
      va_stage(tile, pts, flags, t0, m, g);
      for (int j = 0; j < m; j++) {
        const VaPoint q = tile[j];
        if (q.key == key) {
          fx += q.x; fy += q.y;
          Sx += (double)q.x; Sy += (double)q.y;
          Ax += fabs((double)q.x); Ay += fabs((double)q.y);
          cnt++;
        }
        rank += (q.lead != 0u) & (q.key < key);
      }
    }
    // last to first
    float bx = 0.f, by = 0.f;
    for (int t = n_tiles - 1; t >= 0; t--) {
      const int t0 = t * kVaTile, m = min(kVaTile, n - t0);
      va_stage(tile, pts, nullptr, t0, m, g);
      for (int j = m - 1; j >= 0; j--) {
        const VaPoint q = tile[j];
        if (q.key == key) { bx += q.x; by += q.y; }
      }
    }
    float cfx = 0.f, cfy = 0.f, crx = 0.f, cry = 0.f;
    double ex = 0.0, ey = 0.0, lox = 0.0, hix = 0.0, loy = 0.0, hiy = 0.0;
    if (live) {
      const float fn = (float)cnt;
      cfx = fx / fn; cfy = fy / fn; crx = bx / fn; cry = by / fn;
      const double nd = (double)cnt, nm1 = (double)(cnt - 1);
      const double gam = (nm1 * u) / (1.0 - nm1 * u);
      const double midx = Sx / nd, midy = Sy / nd;
      const double tx = (gam * Ax) / nd, ty = (gam * Ay) / nd;
      ex = (tx + u * (fabs(midx) + tx)) + 0x1p-40 * (fabs(midx) + 1.0);
      ey = (ty + u * (fabs(midy) + ty)) + 0x1p-40 * (fabs(midy) + 1.0);
      lox = midx - ex; hix = midx + ex; loy = midy - ey; hiy = midy + ey;
    }
    // every point of the scan against the enclosure, and against the two centroids with FLANN's float test
    int sure_in = 0, exposed = 0, changed = 0;
    for (int t = 0; t < n_tiles; t++) {
      const int t0 = t * kVaTile, m = min(kVaTile, n - t0);
      va_stage(tile, pts, nullptr, t0, m, g);
      if (!live) continue;
      for (int j = 0; j < m; j++) {
        const VaPoint q = tile[j];
        const double px = (double)q.x, py = (double)q.y;
        const double nx = fmax(fmax(lox - px, px - hix), 0.0), ny = fmax(fmax(loy - py, py - hiy), 0.0);
        const double fxd = fmax(px - lox, hix - px), fyd = fmax(py - loy, hiy - py);
        const double d2min = nx * nx + ny * ny, d2max = fxd * fxd + fyd * fyd;
        const bool in_all = d2max * (1.0 + 8.0 * u) < r2d, out_all = d2min * (1.0 - 8.0 * u) >= r2d;
        sure_in += in_all;
        exposed += !in_all && !out_all;
        float dx = cfx - q.x, dy = cfy - q.y;
        float d = dx * dx;
        d += dy * dy;
        const bool mf = d < r2;
        dx = crx - q.x; dy = cry - q.y;
        d = dx * dx;
        d += dy * dy;
        changed |= mf != (d < r2);
      }
    }
    if (!live) continue;
    const bool differ = __float_as_uint(cfx) != __float_as_uint(crx) || __float_as_uint(cfy) != __float_as_uint(cry);
    c_differ += differ;
    c_pairs += exposed;
    c_exposed += exposed > 0;
    c_thr += sure_in < 6 && sure_in + exposed >= 6;
    c_changed += changed;
    c_maxpts = max(c_maxpts, cnt);
    c_maxe = fmax(c_maxe, fmax(ex, ey));
    const int64_t row = in.voff + rank;
    if (voxels && row < voxel_cap) {
      cfear_voxel_audit_voxel o;
      o.key = key; o.n_points = cnt;
      o.c_fwd[0] = cfx; o.c_fwd[1] = cfy; o.c_rev[0] = crx; o.c_rev[1] = cry;
      o.e[0] = ex; o.e[1] = ey;
      o.n_sure_in = sure_in; o.n_exposed = exposed; o.changed_reversed = changed; o.pad = 0;
      voxels[row] = o;
    }
  }
  // the wavefront's sums and maxima, then one atomic per counter: integers and a maximum, so no order shows
  c_differ = wave_sum_i32(c_differ); c_pairs = wave_sum_i32(c_pairs); c_exposed = wave_sum_i32(c_exposed);
  c_thr = wave_sum_i32(c_thr); c_changed = wave_sum_i32(c_changed);
  c_maxpts = __builtin_amdgcn_readlane(wave_incl_scan_max_i32(c_maxpts), 63);
  c_maxe = va_wave_max_f64(c_maxe);
  if ((tid & 63) == 0) {
    atomicAdd(&rec->n_centroids_reversed_differ, c_differ); atomicAdd(&rec->n_pairs_exposed, c_pairs);
    atomicAdd(&rec->n_voxels_exposed, c_exposed); atomicAdd(&rec->n_voxels_exposed_at_threshold, c_thr);
    atomicAdd(&rec->n_voxels_changed_reversed, c_changed); atomicMax(&rec->max_voxel_points, c_maxpts);
    atomicMax((unsigned long long*)&rec->max_halfwidth, (unsigned long long)__double_as_longlong(c_maxe));   // non-negative: the bits order as the values
  }
}

}  // namespace

extern "C" void cfear_voxel_audit_params_default(cfear_voxel_audit_params* p) {
  if (!p) return;
  p->radius = 3.0f;
  p->pad = 0.f;
  p->downsample_factor = 1.0;
}

extern "C" int cfear_voxel_order_audit_batch(cfear_ctx* ctx, const float* xyzi, const int64_t* offsets, const int32_t* lengths, int32_t n_scans,
                                             const cfear_voxel_audit_params* par, cfear_voxel_audit_record* records,
                                             cfear_voxel_audit_voxel* voxels, int64_t voxel_cap, int64_t* n_voxels_out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!xyzi || !lengths || !par || !records) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if (n_scans < 0 || voxel_cap < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "n_scans and voxel_cap must not be negative");
  if (!std::isfinite(par->radius) || !(par->radius > 0.f) || !std::isfinite(par->downsample_factor) || !(par->downsample_factor > 0.0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "radius and downsample_factor must be finite and greater than 0");
  const float leaf = (float)(par->radius / par->downsample_factor);            // pointnormal.cpp:279
  const float inv_leaf = 1.0f / leaf;                                          // Array4f::Ones() / leaf
  const float r2 = (float)((double)par->radius * (double)par->radius);         // KdTreeFLANN::radiusSearch
  if (!(leaf > 0.f) || !std::isfinite(inv_leaf) || !std::isfinite(r2))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "radius / downsample_factor is not a float leaf size");
  int64_t span = 0, total = 0;
  for (int s = 0; s < n_scans; s++) {
    if (lengths[s] < 0 || (offsets && offsets[s] < 0))
      return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "scan %d: negative length or offset", s);
    span = std::max(span, (offsets ? offsets[s] : total) + lengths[s]);
    total += lengths[s];
  }
  if (memory_kind({records, voxels}) < 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "records and voxels must both be host or both be device memory");
  if (n_scans == 0) {
    if (n_voxels_out) *n_voxels_out = 0;
    return CFEAR_OK;
  }
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  HostStage st(ctx, kWsVoxelAudit);
  const size_t in_bytes = (size_t)n_scans * sizeof(VaIn);
  VaIn* h_in = (VaIn*)st.pinned(in_bytes);
  if (!h_in) return CFEAR_ERR_HIP;
  int64_t run = 0, scr = 0;
  for (int s = 0; s < n_scans; s++) {
    const int n = lengths[s];
    const bool held = n > 0 && n <= kVaMaxPoints;
    h_in[s] = VaIn{offsets ? offsets[s] : run, scr, 0, n, n == 0 ? CFEAR_ERR_EMPTY_CLOUD : held ? CFEAR_OK : CFEAR_ERR_CAPACITY};
    run += n;
    if (held) scr += n;                                    // leaders and flags of the scans the kernels take
  }
  const float* d_xyzi;
  VaIn* d_in;
  VaScan* d_scan;
  int32_t* d_lead;
  uint8_t* d_flag;
  cfear_voxel_audit_record* d_rec;
  cfear_voxel_audit_voxel* d_vox = nullptr;
  st.in(d_xyzi, xyzi, (size_t)span * 16);
  st.piece(d_in, in_bytes);
  st.piece(d_scan, (size_t)n_scans * sizeof(VaScan));
  st.piece(d_lead, (size_t)scr * 4);
  st.piece(d_flag, (size_t)scr);
  st.out(d_rec, records, (size_t)n_scans * sizeof(cfear_voxel_audit_record));
  const bool rows = voxels && voxel_cap > 0, rows_host = rows && st.is_host(voxels);
  if (rows_host) st.piece(d_vox, (size_t)voxel_cap * sizeof(cfear_voxel_audit_voxel));   // copied back as far as it was written
  else if (rows) d_vox = voxels;
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(st.upload(d_in, h_in, in_bytes));
  CFEAR_HIP_CHECK(ctx, hipMemsetAsync(d_rec, 0, (size_t)n_scans * sizeof(cfear_voxel_audit_record), ctx->stream));
  {
    ProfScope ps(ctx, "voxel_leaders");
    hipLaunchKernelGGL(voxel_leaders_kernel, dim3(n_scans), dim3(kVaThreads), 0, ctx->stream, d_xyzi, d_in, (int)n_scans, inv_leaf, d_scan, d_lead,
                       d_flag);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  // host half: where every scan's rows start, and the first status
  std::vector<VaScan> h_scan(n_scans);
  st.fetch(h_scan.data(), d_scan, (size_t)n_scans * sizeof(VaScan));
  CFEAR_CHECK(st.wait());
  int64_t n_rows = 0;
  int first = CFEAR_OK;
  for (int s = 0; s < n_scans; s++) {
    h_in[s].voff = n_rows;
    n_rows += h_scan[s].n_vox;
    if (first == CFEAR_OK) first = h_scan[s].status;
  }
  CFEAR_CHECK(st.upload(d_in, h_in, in_bytes));
  {
    ProfScope ps(ctx, "voxel_audit");
    hipLaunchKernelGGL(voxel_audit_kernel, dim3(n_scans), dim3(kVaThreads), 0, ctx->stream, d_xyzi, d_in, d_scan, (int)n_scans, inv_leaf, r2, d_lead,
                       d_flag, d_rec, d_vox, rows ? voxel_cap : (int64_t)0);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  if (rows_host && n_rows > 0) st.back(voxels, d_vox, (size_t)std::min(n_rows, voxel_cap) * sizeof(cfear_voxel_audit_voxel));
  CFEAR_CHECK(st.finish());
  if (n_voxels_out) *n_voxels_out = n_rows;
  if (first != CFEAR_OK) return cfear_set_error(ctx, first, "a scan was not audited (the records carry the statuses; the others are complete)");
  if (voxels && n_rows > voxel_cap)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "%lld voxels, the table holds %lld (the records are complete)", (long long)n_rows,
                           (long long)voxel_cap);
  return CFEAR_OK;
}
