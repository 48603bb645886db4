// kstrong_legacy.hip -- the legacy k_strongest_filter / InsertStrongestK (radar_filters.cpp:25-78; CorAl's standalone
// kstrongRadar, coral_alignment_quality/src/alignment_checker/ScanType.cpp:104-114).  Different rule than StructuredKStrongest
// (SURVEY App. C): the first bin f with intensity >= z_min sets a floor m0 -- later bins <= the list's minimum are
// rejected even while the list is not full -- and ties at the cut keep the SMALLER ranges.  In closed form: with D = the
// bins after f with intensity > m0, the row keeps the k largest of D under (intensity, -range), plus f iff |D| < k,
// in descending intensity / ascending range order.  "k largest under (intensity, -range)" is StructuredKStrongest on the
// REVERSED row, so the tuned sweep (kstrong.hip, through cfear_kstrong_device) does the selection: legacy_prepare_kernel
// writes the row reversed with everything outside D zeroed, the sweep runs with z_min = 1, and legacy_cloud_kernel undoes
// the reversal, appends f and converts to PointXYZI.
#include <cmath>

#include "polar_common.hpp"

namespace {

constexpr int kLegacyMaxGridY = 65535;     // images per launch of legacy_prepare_kernel: it has the image on gridDim.y

__global__ __launch_bounds__(256) void legacy_prepare_kernel(const uint8_t* __restrict__ polar, int rows, int cols, int stride,
                                                             long long batch_stride, int u_z, uint8_t* __restrict__ rev,
                                                             int rev_stride, int32_t* __restrict__ first /*[batch][rows][2]*/) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long grow = (long long)blockIdx.x * 4 + wave;
  const int b = blockIdx.y;
  if (grow >= rows) return;
  const int r = (int)grow;
  const uint8_t* rowp = polar + (long long)b * batch_stride + (long long)r * stride;
  int fpos = 0x7fffffff;                                   // first bin with intensity >= z_min
  for (int i0 = 0; i0 < cols && fpos == 0x7fffffff; i0 += 64) {
    const int i = i0 + lane;
    const bool c = i < cols && (int)rowp[i] >= u_z;
    const unsigned long long bal = __ballot(c);
    if (bal) fpos = i0 + __ffsll((long long)bal) - 1;
  }
  const int m0 = fpos < cols ? (int)rowp[fpos] : 255;
  uint8_t* out = rev + ((long long)b * rows + r) * rev_stride;
  for (int i = lane; i < cols; i += 64) {
    const int v = rowp[i];
    out[cols - 1 - i] = (i > fpos && v > m0) ? (uint8_t)v : (uint8_t)0;
  }
  if (lane == 0) { first[((long long)b * rows + r) * 2] = fpos < cols ? fpos : -1; first[((long long)b * rows + r) * 2 + 1] = m0; }
}

// one workgroup per image: per-row output counts -> offsets -> points
__global__ __launch_bounds__(256) void legacy_cloud_kernel(const int32_t* __restrict__ sel_range, const uint8_t* __restrict__ sel_int,
                                                           const int32_t* __restrict__ sel_count, const int32_t* __restrict__ first,
                                                           const float* __restrict__ cosf_t, const float* __restrict__ sinf_t,
                                                           int rows, int cols, int k, double range_res, double min_d2,
                                                           float* __restrict__ xyzi, int32_t* __restrict__ n_points, int cap) {
  extern __shared__ int32_t row_off[];                    // [rows + 1]
  __shared__ int32_t wave_tot[4];
  __shared__ int32_t run_base;
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  auto point = [&](int r, int j, int cnt, float4& p) -> bool {    // j-th entry of row r in the reference's list order
    int bin, inten;
    if (j < cnt) {                                         // descending: the sweep's list reversed; undo the row reversal
      const long long e = ((long long)b * rows + r) * k + (cnt - 1 - j);
      bin = cols - 1 - sel_range[e];
      inten = sel_int[e];
    } else {                                               // f, the floor-setting first bin (only while |D| < k)
      bin = first[((long long)b * rows + r) * 2];
      inten = first[((long long)b * rows + r) * 2 + 1];
    }
    p.x = (float)(range_res * bin * cosf_t[r]);            // :62-63
    p.y = (float)(range_res * bin * sinf_t[r]);
    p.z = 0.f;
    p.w = (float)inten;
    return (double)(p.x * p.x + p.y * p.y) > min_d2;       // :71
  };
  auto row_entries = [&](int r) {
    const int cnt = sel_count[(long long)b * rows + r];
    const bool has_f = first[((long long)b * rows + r) * 2] >= 0 && cnt < k;
    return cnt + (has_f ? 1 : 0);
  };
  if (threadIdx.x == 0) run_base = 0;
  __syncthreads();
  for (int r0 = 0; r0 < rows; r0 += 256) {
    const int r = r0 + threadIdx.x;
    int v = 0;
    if (r < rows) {
      const int cnt = sel_count[(long long)b * rows + r], ne = row_entries(r);
      float4 p;
      for (int j = 0; j < ne; j++) v += point(r, j, cnt, p) ? 1 : 0;
    }
    const int incl = wave_incl_scan_i32(v);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int off = run_base;
    for (int wv = 0; wv < wave; wv++) off += wave_tot[wv];
    if (r < rows) row_off[r] = off + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) run_base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_points[b] = run_base;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const int cnt = sel_count[(long long)b * rows + r], ne = row_entries(r);
    int o = row_off[r];
    for (int j = 0; j < ne; j++) {
      float4 p;
      if (point(r, j, cnt, p)) {
        if (o < cap) ((float4*)xyzi)[(long long)b * cap + o] = p;
        o++;
      }
    }
  }
}

}  // namespace

extern "C" int cfear_filter_kstrongest_legacy(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, int32_t k_strongest,
                                              double z_min, double range_res, double min_distance, float* xyzi, int32_t* n_points,
                                              int32_t cap_points) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!polar || !xyzi || !n_points || cap_points <= 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_desc(ctx, desc));
  if (k_strongest < 1 || k_strongest > kMaxK) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k_strongest must be in [1,%d]", kMaxK);
  if (!(range_res > 0.0)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "range_res must be > 0");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, cols = desc->cols, batch = desc->batch, k = k_strongest;
  HostStage st(ctx, kWsFilter);
  const uint8_t* d_polar;
  const cfear_polar_desc dd = st.images(d_polar, polar, *desc);
  float* d_xyzi;
  int32_t* d_np;
  st.out(d_xyzi, xyzi, (size_t)batch * cap_points * 16);
  st.out(d_np, n_points, (size_t)batch * 4);
  if (st.mixed())
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar, xyzi and n_points must all be host or all be device memory");
  // scratch: reversed masked images | first-bin records | sel arrays | float trig tables
  const int rev_stride = (cols + 15) / 16 * 16;
  const size_t nsel = (size_t)batch * rows * k;
  uint8_t* d_rev;
  int32_t* d_first;
  float* d_trig;
  cfear_kstrong_out o{};
  st.piece(d_rev, (size_t)batch * rows * rev_stride);
  st.piece(d_first, (size_t)batch * rows * 8);
  st.piece(o.sel_range, nsel * 4);
  st.piece(o.sel_intensity, nsel);
  st.piece(o.sel_count, (size_t)batch * rows * 4);
  st.piece(d_trig, (size_t)rows * 8);
  CFEAR_CHECK(st.carve());
  float* h = (float*)st.record((size_t)rows * 8);          // host cosf / sinf of the FLOAT theta: bit-exact with glibc
  for (int bearing = 0; bearing < rows; bearing++) {
    const float theta = ((float)(bearing + 1) / rows) * 2 * M_PI;            // radar_filters.cpp:52
    h[bearing] = std::cos(theta);
    h[rows + bearing] = std::sin(theta);
  }
  CFEAR_CHECK(st.upload(d_trig, h, (size_t)rows * 8));
  int u_z = (int)std::ceil(z_min);                         // uchar v < z_min  <=>  v < ceil(z_min)
  u_z = std::max(0, std::min(256, u_z));
  {
    ProfScope ps(ctx, "kstrong_legacy_prepare");
    const long long bstride = batch > 1 ? (long long)dd.batch_stride : (long long)rows * desc->stride;
    for (int b0 = 0; b0 < batch; b0 += kLegacyMaxGridY)
      hipLaunchKernelGGL(legacy_prepare_kernel, dim3((rows + 3) / 4, std::min(kLegacyMaxGridY, batch - b0)), dim3(256), 0, ctx->stream,
                         d_polar + b0 * bstride, rows, cols, desc->stride, bstride, u_z, d_rev + (size_t)b0 * rows * rev_stride, rev_stride,
                         d_first + (size_t)b0 * rows * 2);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  cfear_polar_desc rd{rows, cols, rev_stride, batch, (int64_t)rows * rev_stride};
  cfear_kstrong_params kp{k, 1.0f, 1.0f, 0.0f, 0};
  CFEAR_CHECK(cfear_kstrong_device(ctx, d_rev, &rd, &kp, &o));
  {
    ProfScope ps(ctx, "kstrong_legacy_cloud");
    hipLaunchKernelGGL(legacy_cloud_kernel, dim3(batch), dim3(256), (size_t)(rows + 1) * 4, ctx->stream, o.sel_range, o.sel_intensity,
                       o.sel_count, d_first, d_trig, d_trig + rows, rows, cols, k, range_res, min_distance * min_distance, d_xyzi, d_np,
                       cap_points);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  CFEAR_CHECK(st.finish());
  if (st.any_host())
    for (int b = 0; b < batch; b++)
      if (n_points[b] > cap_points) return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "image %d: %d points > cap_points %d", b, n_points[b], cap_points);
  return CFEAR_OK;
}
