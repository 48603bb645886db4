// cartesian.hip -- the Cartesian radar image and CorAlCartQuality on gfx950.
//
// Replaces (coral_alignment_quality/src/alignment_checker):
//   CartesianRadar::CartesianRadar: convertTo(CV_32F, 1 / 255.0) + radar_polar_to_cartesian      ScanType.cpp:191-209
//   radar_polar_to_cartesian: two float maps per Cartesian pixel, cv::remap                       Utils.cpp:255-323
//   RotoTranslation: warpAffine(getRotationMatrix2D), then warpAffine of its output by (tx, ty)   Utils.cpp:325-339
//   CorAlCartQuality: cv::sum(cv::absdiff(warped source, reference))                              AlignmentQuality.cpp:356-386
// The arithmetic of OpenCV's remap / warpAffine / getRotationMatrix2D / convertTo is restated from knowledge of OpenCV 4.2
// (tests/cart_cpu.py is the definition, DESIGN.md 4.13 lists what is not pinned).
//
// Kernel design.  Everything that depends on the geometry alone is done once on the HOST: the float maps (atan2f of the host's
// libm -- no device transcendental touches a coordinate) quantised to 1/32 pixel, 8 bytes per Cartesian pixel, kept in the
// context.  polar_to_cart_kernel is then a pure gather: one thread per pixel, four byte loads, one multiply each (the
// 256-entry convertTo table is float(u8) * float(1 / 255.0), a single rounding, so the multiply IS the table), the weighted
// sum.  cart_warp_kernel fuses the two warps: an output pixel's four taps into the rotated image are evaluated on the fly
// from the source (at most 16 reads); the rotated pixel is a function of its coordinates only, so the result is bit-equal to
// materialising it.  A job is split over ceil(W^2 / 4096) workgroups -- a split that depends on W only -- each reduces
// |warped - ref| in double per thread (stride 256), over a fixed DPP tree and over its four waves in order; cart_sum_kernel
// adds a job's partial sums the same way and writes the record.  No atomics; every store is a vector store.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <map>
#include <vector>

#include "common.hpp"

namespace {

constexpr int kCartThreads = 256;
constexpr int kCartChunk = 4096;                         // pixels per workgroup of cart_warp_kernel: 16 per thread
constexpr int kCartMaxGridY = 65535;
static_assert(CFEAR_CART_MAX_WIDTH == 4096, "limit stated in cfear_hip.h");

struct CartImageArgs {
  const uint8_t* polar;
  const unsigned long long* map;      // [W * W]: {ix (low 16, signed) | iy (high 16, signed), fy * 32 + fx}
  float* cart;
  int32_t rows, cols, stride, W, batch;
  long long batch_stride;
  float k255;                         // float(1 / 255.0)
};

struct CartJobDev {
  const float* src;
  const float* ref;
  double R[6];                        // the inverted rotation matrix
  double T[6];                        // the inverted translation matrix
  int32_t status, pad;
};

struct CartWarpArgs {
  const CartJobDev* jobs;
  double* partial;                    // [n_jobs][nb]
  float* warped;                      // nullable
  cfear_cart_result* results;
  int32_t n_jobs, W, nb, pad;
};

// ((S00 w0 + S01 w1) + S10 w2) + S11 w3 with the weights of OpenCV's BilinearTab_f; taps outside the image read 0
__device__ __forceinline__ float blend(float s00, float s01, float s10, float s11, int fx, int fy) {
  const float ax = (float)fx * 0.03125f, ay = (float)fy * 0.03125f;
  const float w0 = (1.0f - ay) * (1.0f - ax), w1 = (1.0f - ay) * ax, w2 = ay * (1.0f - ax), w3 = ay * ax;   // exact
  return ((s00 * w0 + s01 * w1) + s10 * w2) + s11 * w3;
}

__global__ __launch_bounds__(kCartThreads) void polar_to_cart_kernel(const CartImageArgs a) {
  const int npix = a.W * a.W;
  const int p = blockIdx.x * kCartThreads + threadIdx.x;
  if (p >= npix) return;
  const unsigned long long m = gload<unsigned long long>(a.map + p);
  const int ix = (int)(short)(m & 0xFFFFu), iy = (int)(short)((m >> 16) & 0xFFFFu);
  const int fxy = (int)((m >> 32) & 0x3FFu);
  const bool none = ix >= a.cols || ix + 1 < 0 || iy >= a.rows || iy + 1 < 0;
  const bool x0 = ix >= 0 && ix < a.cols, x1 = ix + 1 >= 0 && ix + 1 < a.cols;
  const bool y0 = iy >= 0 && iy < a.rows, y1 = iy + 1 >= 0 && iy + 1 < a.rows;
  const long long o00 = (long long)iy * a.stride + ix, o10 = o00 + a.stride;
  for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
    float v = 0.0f;
    if (!none) {
      const uint8_t* img = a.polar + (long long)b * a.batch_stride;
      const float s00 = (x0 && y0) ? (float)gload<uint8_t>(img + o00) * a.k255 : 0.0f;
      const float s01 = (x1 && y0) ? (float)gload<uint8_t>(img + o00 + 1) * a.k255 : 0.0f;
      const float s10 = (x0 && y1) ? (float)gload<uint8_t>(img + o10) * a.k255 : 0.0f;
      const float s11 = (x1 && y1) ? (float)gload<uint8_t>(img + o10 + 1) * a.k255 : 0.0f;
      v = blend(s00, s01, s10, s11, fxy & 31, fxy >> 5);
    }
    gstore<float>(a.cart + (size_t)b * npix + p, v);
  }
}

// cvRound of a double that is known to fit an int
__device__ __forceinline__ int round_i32(double v) { return (int)rint(v); }

__device__ __forceinline__ float sample(const float* img, int W, int X, int Y) {
  const int ix = X >> 5, iy = Y >> 5;
  if (ix >= W || ix + 1 < 0 || iy >= W || iy + 1 < 0) return 0.0f;
  const bool x0 = ix >= 0, x1 = ix + 1 < W, y0 = iy >= 0, y1 = iy + 1 < W;
  const long long o = (long long)iy * W + ix;
  const float s00 = (x0 && y0) ? gload<float>(img + o) : 0.0f;
  const float s01 = (x1 && y0) ? gload<float>(img + o + 1) : 0.0f;
  const float s10 = (x0 && y1) ? gload<float>(img + o + W) : 0.0f;
  const float s11 = (x1 && y1) ? gload<float>(img + o + W + 1) : 0.0f;
  return blend(s00, s01, s10, s11, X & 31, Y & 31);
}

__global__ __launch_bounds__(kCartThreads) void cart_warp_kernel(const CartWarpArgs a) {
  __shared__ double red[kCartThreads / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int W = a.W, npix = W * W, blk = blockIdx.x;
  for (int j = blockIdx.y; j < a.n_jobs; j += gridDim.y) {
    const CartJobDev* jb = a.jobs + j;
    const int status = gload<int32_t>(&jb->status);
    const float* src = (const float*)gload<unsigned long long>(&jb->src);
    const float* ref = (const float*)gload<unsigned long long>(&jb->ref);
    double R[6], T[6];
#pragma unroll
    for (int k = 0; k < 6; k++) { R[k] = gload<double>(&jb->R[k]); T[k] = gload<double>(&jb->T[k]); }
    double acc = 0.0;
    for (int q = 0; q < kCartChunk / kCartThreads; q++) {
      const int p = blk * kCartChunk + q * kCartThreads + tid;
      if (p >= npix) break;
      float out = 0.0f;
      if (status == CFEAR_OK) {
        const int y = p / W, x = p - y * W;
        // the translation warp's tap into the rotated image: 1/1024-pixel integers, + 16, >> 5 (warpAffine, INTER_LINEAR)
        const int X = (round_i32((T[1] * (double)y + T[2]) * 1024.0) + 16 + round_i32(T[0] * (double)x * 1024.0)) >> 5;
        const int Y = (round_i32((T[4] * (double)y + T[5]) * 1024.0) + 16 + round_i32(T[3] * (double)x * 1024.0)) >> 5;
        const int ix = X >> 5, iy = Y >> 5;
        if (!(ix >= W || ix + 1 < 0 || iy >= W || iy + 1 < 0)) {
          float r[2][2];
          int ad[2], bd[2], x0[2], y0[2];
#pragma unroll
          for (int t = 0; t < 2; t++) {
            const double u = (double)min(max(ix + t, 0), W - 1), v = (double)min(max(iy + t, 0), W - 1);
            ad[t] = round_i32(R[0] * u * 1024.0);
            bd[t] = round_i32(R[3] * u * 1024.0);
            x0[t] = round_i32((R[1] * v + R[2]) * 1024.0) + 16;
            y0[t] = round_i32((R[4] * v + R[5]) * 1024.0) + 16;
          }
#pragma unroll
          for (int tv = 0; tv < 2; tv++)
#pragma unroll
            for (int tu = 0; tu < 2; tu++) {
              const bool in = ix + tu >= 0 && ix + tu < W && iy + tv >= 0 && iy + tv < W;
              r[tv][tu] = in ? sample(src, W, (x0[tv] + ad[tu]) >> 5, (y0[tv] + bd[tu]) >> 5) : 0.0f;
            }
          out = blend(r[0][0], r[0][1], r[1][0], r[1][1], X & 31, Y & 31);
        }
        acc += (double)fabsf(out - gload<float>(ref + p));
      }
      if (a.warped) gstore<float>(a.warped + (size_t)j * npix + p, out);
    }
    acc = wave_sum_lane63_f64(acc);
    if (lane == 63) red[wave] = acc;
    __syncthreads();
    if (tid == 0) gstore<double>(a.partial + (size_t)j * a.nb + blk, ((red[0] + red[1]) + red[2]) + red[3]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void cart_sum_kernel(const CartWarpArgs a) {
  const int j = blockIdx.x, lane = threadIdx.x;
  double acc = 0.0;
  for (int b = lane; b < a.nb; b += 64) acc += gload<double>(a.partial + (size_t)j * a.nb + b);
  acc = wave_sum_lane63_f64(acc);
  if (lane == 63) {
    cfear_cart_result r;
    r.status = gload<int32_t>(&a.jobs[j].status);
    r.abs_diff = r.status == CFEAR_OK ? acc : 0.0;
    r.pad = 0;
    a.results[j] = r;
  }
}

// The fixed-point map of radar_polar_to_cartesian + cv::remap's float -> short conversion (Utils.cpp:258-308).  Host code:
// this file is built without fused multiply-adds and float expressions are evaluated in float.
void build_cart_map(int rows, int W, float radar_resolution, float cart_resolution, std::vector<unsigned long long>& out) {
  float cart_min_range = (W / 2) * cart_resolution;
  if (W % 2 == 0) cart_min_range = (W / 2 - 0.5) * cart_resolution;
  const double az0 = ((double)1 / rows) * 2 * M_PI, az_last = ((double)rows / rows) * 2 * M_PI;
  const double azimuth_step = (az_last - az0) / (unsigned)(rows - 1);
  auto quantise = [](float v, int& i, int& f) {              // cvRound(v * 32), >> 5 saturated to short, & 31
    if (!(std::fabs(v) < 16777216.0f)) { i = 32767; f = 0; return; }   // outside on either side of the saturation
    const int s = (int)lrintf(v * 32.0f);
    i = std::min(std::max(s >> 5, -32768), 32767);
    f = s & 31;
  };
  out.resize((size_t)W * W);
  std::vector<float> map_y((size_t)W);
  for (int j = 0; j < W; j++) map_y[j] = -1 * cart_min_range + j * cart_resolution;
  for (int i = 0; i < W; i++) {
    const float x = cart_min_range - i * cart_resolution;
    for (int j = 0; j < W; j++) {
      const float y = map_y[j];
      float r = (std::sqrt((double)x * (double)x + (double)y * (double)y) - radar_resolution / 2) / radar_resolution;
      if (r < 0) r = 0;
      float theta = atan2f(y, x);
      if (theta < 0) theta += 2 * M_PI;
      const float angle = (theta - az0) / azimuth_step;
      int ix, fx, iy, fy;
      quantise(r, ix, fx);
      quantise(angle, iy, fy);
      out[(size_t)i * W + j] = (unsigned long long)(uint16_t)(int16_t)ix | ((unsigned long long)(uint16_t)(int16_t)iy << 16) |
                               ((unsigned long long)(fy * 32 + fx) << 32);
    }
  }
}

bool good_resolution(float v) { return v > 0.0f && v <= FLT_MAX; }

// warpAffine's inversion of a forward matrix (no WARP_INVERSE_MAP), in double
void invert_affine(double M[6]) {
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D;
  M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
}

}  // namespace

extern "C" void cfear_cart_params_default(cfear_cart_params* par) {
  if (!par) return;
  par->radar_resolution = 0.04328f;
  par->cart_resolution = 0.2384f;
  par->cart_pixel_width = 300;
  par->pad = 0;
}

extern "C" int cfear_polar_to_cartesian(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                        const cfear_cart_params* par, float* cart) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!polar || !desc || !par || !cart) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar_to_cartesian: null argument");
  if (desc->rows <= 0 || desc->cols <= 0 || desc->stride < desc->cols || desc->batch <= 0 ||
      (desc->batch > 1 && desc->batch_stride < (int64_t)desc->rows * desc->stride))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar_to_cartesian: bad polar descriptor");
  if (desc->rows < 2 || desc->rows > 32767 || desc->cols > 32767)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar_to_cartesian: %d x %d sweeps: rows must be in [2, 32767], cols <= 32767",
                           desc->rows, desc->cols);
  const int W = par->cart_pixel_width;
  if (W < 1 || W > CFEAR_CART_MAX_WIDTH)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar_to_cartesian: cart_pixel_width must be in [1, %d]", CFEAR_CART_MAX_WIDTH);
  if (!good_resolution(par->radar_resolution) || !good_resolution(par->cart_resolution))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar_to_cartesian: resolutions must be finite and > 0");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, batch = desc->batch;
  const size_t npix = (size_t)W * W, map_bytes = npix * 8;

  std::vector<unsigned long long> h_map;                   // outlives the stage, which waits for its upload
  HostStage st(ctx, kWsCart);
  CartImageArgs a{};
  const cfear_polar_desc dd = st.images(a.polar, polar, *desc);
  st.out(a.cart, cart, (size_t)batch * npix * sizeof(float));
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "polar_to_cartesian: the sweeps and the images must be all host or all device");
  CFEAR_CHECK(st.carve());
  const bool cached = ctx->cart_map_w == W && ctx->cart_map_rows == rows && ctx->cart_map_radar_res == par->radar_resolution &&
                      ctx->cart_map_cart_res == par->cart_resolution && ctx->ws[kWsCartMap].p;
  if (!cached) {
    ctx->cart_map_w = 0;
    void* d_map = cfear_workspace(ctx, kWsCartMap, map_bytes);
    if (!d_map) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
    build_cart_map(rows, W, par->radar_resolution, par->cart_resolution, h_map);
    CFEAR_CHECK(st.upload(d_map, h_map.data(), map_bytes));
    ctx->cart_map_w = W; ctx->cart_map_rows = rows;
    ctx->cart_map_radar_res = par->radar_resolution; ctx->cart_map_cart_res = par->cart_resolution;
  }
  a.map = (const unsigned long long*)ctx->ws[kWsCartMap].p.get();
  a.rows = rows; a.cols = desc->cols; a.stride = dd.stride; a.W = W; a.batch = batch;
  a.batch_stride = batch > 1 ? dd.batch_stride : (long long)rows * dd.stride;
  a.k255 = (float)(1 / 255.0);
  {
    ProfScope ps(ctx, "polar_to_cartesian");
    hipLaunchKernelGGL(polar_to_cart_kernel, dim3((unsigned)((npix + kCartThreads - 1) / kCartThreads), (unsigned)std::min(batch, kCartMaxGridY)),
                       dim3(kCartThreads), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}

extern "C" int cfear_cart_quality_batch(cfear_ctx* ctx, const cfear_cart_job* jobs, int32_t n_jobs, int32_t cart_pixel_width,
                                        float image_res, cfear_cart_result* results, float* warped) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!jobs || !results || n_jobs < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cart_quality: null argument");
  const int W = cart_pixel_width;
  if (W < 1 || W > CFEAR_CART_MAX_WIDTH)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cart_quality: cart_pixel_width must be in [1, %d]", CFEAR_CART_MAX_WIDTH);
  if (!good_resolution(image_res)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cart_quality: image_res must be finite and > 0");
  if (n_jobs == 0) return CFEAR_OK;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const size_t npix = (size_t)W * W, img_bytes = npix * sizeof(float);
  const int nb = (int)((npix + kCartChunk - 1) / kCartChunk);

  HostStage st(ctx, kWsCart);
  std::map<const float*, const float*> dev_of;              // every distinct image is staged once (node addresses are stable)
  for (int j = 0; j < n_jobs; j++) {
    if (!jobs[j].src || !jobs[j].ref) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cart_quality: job %d: null image", j);
    for (const float* p : {jobs[j].src, jobs[j].ref}) {
      auto ins = dev_of.emplace(p, nullptr);
      if (ins.second) st.in(ins.first->second, p, img_bytes);
    }
  }
  const size_t job_bytes = (size_t)n_jobs * sizeof(CartJobDev);
  CartWarpArgs a{};
  char* d_jobs;
  st.piece(d_jobs, job_bytes);
  st.piece(a.partial, (size_t)n_jobs * nb * sizeof(double));
  st.out(a.results, results, (size_t)n_jobs * sizeof(cfear_cart_result));
  if (warped) st.out(a.warped, warped, (size_t)n_jobs * img_bytes);
  CFEAR_CHECK(st.carve());
  CartJobDev* hj = (CartJobDev*)st.pinned(job_bytes);
  if (!hj) return CFEAR_ERR_HIP;
  const float c = (float)((W - 1) / 2.0);                   // cv::Point2f center((cols - 1) / 2.0, (rows - 1) / 2.0)
  for (int j = 0; j < n_jobs; j++) {
    const cfear_cart_job& jb = jobs[j];
    CartJobDev& o = hj[j];
    o.src = dev_of[jb.src]; o.ref = dev_of[jb.ref];
    o.pad = 0;
    const float tx = (float)jb.x / image_res, ty = (float)jb.y / image_res;
    const bool finite = std::fabs(jb.x) <= DBL_MAX && std::fabs(jb.y) <= DBL_MAX && std::fabs(jb.yaw) <= DBL_MAX;
    if (!finite || !(std::fabs(tx) <= 1048576.0f) || !(std::fabs(ty) <= 1048576.0f)) {
      o.status = CFEAR_ERR_INVALID_ARGUMENT;
      for (int k = 0; k < 6; k++) o.R[k] = o.T[k] = 0.0;
      continue;
    }
    o.status = CFEAR_OK;
    // getRotationMatrix2D(center, angle = the yaw as it comes, scale 1.0)
    const double angle = jb.yaw * (M_PI / 180);
    const double alpha = std::cos(angle), beta = std::sin(angle);
    o.R[0] = alpha; o.R[1] = beta; o.R[2] = (1 - alpha) * c - beta * c;
    o.R[3] = -beta; o.R[4] = alpha; o.R[5] = beta * c + (1 - alpha) * c;
    invert_affine(o.R);
    o.T[0] = 1.0; o.T[1] = 0.0; o.T[2] = tx;
    o.T[3] = 0.0; o.T[4] = 1.0; o.T[5] = ty;
    invert_affine(o.T);
  }
  CFEAR_CHECK(st.upload(d_jobs, hj, job_bytes));
  a.jobs = (const CartJobDev*)d_jobs;
  a.n_jobs = n_jobs; a.W = W; a.nb = nb;
  {
    ProfScope ps(ctx, "cart_quality");
    hipLaunchKernelGGL(cart_warp_kernel, dim3((unsigned)nb, (unsigned)std::min(n_jobs, kCartMaxGridY)), dim3(kCartThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(cart_sum_kernel, dim3((unsigned)n_jobs), dim3(64), 0, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return st.finish();
}
