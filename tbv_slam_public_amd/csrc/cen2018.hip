// cen2018.hip -- Cen and Newman's 2018 radar landmark detector as a batched polar filter on gfx950.
//
// Replaces (coral_alignment_quality/src/alignment_checker/):
//   cen2018features                Utils.cpp:348-434
//   Cen2018Radar::Cen2018Radar     ScanType.cpp:68-88   (convertTo(CV_32F, 1/255.0) and the polar -> Cartesian loop)
//
// Every float operation rounds on its own, in the reference's order (the library is built -ffp-contract=off; `/` and
// sqrt are correctly rounded).  Three kernels per chunk of images (a chunk is sized to stay in the Infinity Cache, so the
// sweeps come from HBM once):
//   cen2018_stats_kernel   ONE LANE PER ROW.  The two float sums of a row -- the mean, and the noise level over the bins
//     below it -- are serial chains of `cols` terms whose order fixes mean and sigma to the bit; a wavefront that gave such
//     a chain to one lane would idle 63.  Here 64 rows advance together, each lane streaming its own row in 16-byte pieces.
//   cen2018_rows_kernel    one wavefront per row, no workgroup barrier.  q = f - mean is staged ONCE in LDS with the
//     BORDER_REFLECT101 halo materialised; a lane then takes 8 consecutive bins, pulls the 8 + taps - 1 floats they need
//     into registers and runs the tap sums from there (taps ascending, multiply and add separate): 7 LDS dwords per bin
//     instead of one per tap, the taps themselves wave-uniform.  The two Gaussians of a bin are first estimated in float
//     (v_exp_f32); the estimate decides y > thres wherever it is further from thres than its own error bound, and only the
//     remaining bins (a few in 10^5) pay the fp64 exp the reference calls.  The row's y > thres bitmap is built in LDS;
//     every run end finds its run's start there and marks the run's element len / 2 in a second bitmap.
//   cen2018_cloud_kernel   compaction in (row, bin) order without atomics: per image a scan of the rows' counts, then one
//     wavefront per row turns the marked bins into targets and PointXYZI (fp64 with the host-computed cos / sin tables).
// Rows are read with 16-byte loads only where all 16 bytes lie inside the row, and byte by byte elsewhere (ragged widths,
// odd strides, rows narrower than a piece): nothing is read beyond a row's own `cols` bytes.
#include <cmath>

#include "common.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kCenMaxCols = 8192;
constexpr int kCenMaxSigma = 341;          // 3 * 341 = 1023 taps
constexpr int kCenRowsWaves = 2;           // wavefronts (rows) per workgroup of cen2018_rows_kernel
constexpr int kCenBinsPerLane = 8;
constexpr int kCenPass = 64 * kCenBinsPerLane;
constexpr int kCenCloudSplit = 4;
constexpr size_t kCenChunkBytes = 64u << 20;   // image bytes per chunk: stats + rows read it twice, the second time on-die
constexpr int kCenMaxGridY = 65535;            // images per chunk: cen2018_rows_kernel has the image on gridDim.y

struct CenArgs {
  const uint8_t* polar;
  int rows, cols, stride, batch;
  long long batch_stride;
  int fsize, mu, min_range_bins;
  float zq;
  const float* taps;                 // [fsize]
  float* stats;                      // [batch][rows][2]: mean, sigma
  unsigned long long* tgt_bits;      // [batch][rows][words]: bit = the bin is a target
  int32_t* tgt_count;                // [batch][rows]
  uint8_t* det_mask;                 // optional [batch][rows][cols]
  int words;                         // 64-bin words per row
  int qlen;                          // floats of a wavefront's staged row (halo and read-ahead included)
  int lds_words;                     // 64-bin words of a wavefront's LDS bitmaps
  int per_wave;                      // LDS bytes per wavefront
  // cloud
  const double* cos_t;
  const double* sin_t;
  double range_res;
  float* xyzi;
  int32_t* n_points;
  int32_t* targets;
  int cap_points;
};

__device__ __forceinline__ float cen_f(uint32_t byte) { return (float)byte * (float)(1 / 255.0); }   // convertTo(CV_32F, 1/255.0)

// fn(f[j]) for j = 0 .. cols - 1 in order, on one lane
template <typename F>
__device__ __forceinline__ void cen_row_serial(const uint8_t* rowp, int cols, F&& fn) {
  int j = 0;
  if ((((uintptr_t)rowp) & 3) == 0) {
    for (; j + 16 <= cols; j += 16) {
      const u32x4 v = *(const u32x4*)(rowp + j);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int d = 0; d < 4; d++)
#pragma unroll
        for (int by = 0; by < 4; by++) fn(cen_f((w[d] >> (8 * by)) & 0xffu));
    }
  }
  for (; j < cols; j++) fn(cen_f(rowp[j]));
}

__global__ __launch_bounds__(256) void cen2018_stats_kernel(const CenArgs a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)a.batch * a.rows) return;
  const int b = (int)(t / a.rows), r = (int)(t - (long long)b * a.rows);
  const uint8_t* rowp = a.polar + (long long)b * a.batch_stride + (long long)r * a.stride;
  float mean = 0.f;                                                          // Utils.cpp:355-359
  cen_row_serial(rowp, a.cols, [&](float f) { mean += f; });
  mean /= (float)a.cols;
  float acc = 0.f;                                                           // Utils.cpp:381-394
  int nonzero = 0;
  cen_row_serial(rowp, a.cols, [&](float f) {
    const float n = f - mean;
    if (n < 0.f) { acc += 2.f * (n * n); nonzero++; }
  });
  // sqrt in double, rounded once more: equal to the correctly rounded float root (53 >= 2 * 24 + 2)
  const float sigma = nonzero ? (float)sqrt((double)(acc / (float)nonzero)) : 0.034f;
  a.stats[t * 2] = mean;
  a.stats[t * 2 + 1] = sigma;
}

__device__ __forceinline__ void cen_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// y > thres for one bin (Utils.cpp:403-407).  The float estimate differs from the reference's y by at most
// (|q| + 2 |p|) (delta + 4 ulp), delta <= 3e-7 the absolute error of exp through v_exp_f32 for arguments <= 0 (the argument's
// own rounding included: x e^-x <= 0.37); the bound below leaves a factor of four.  Inside it -- and for anything that is
// not a number -- the reference's own evaluation decides: exp in fp64, rounded to float once.
__device__ __forceinline__ bool cen_detect(float q, float p, float sigma, float thres) {
  const float d = (q - p) / sigma, e = p / sigma;
  {
    const float nq = __expf(-0.5f * (d * d)), np = __expf(-0.5f * (e * e));
    const float y = q * (1.f - nq) + p * (nq - np);
    const float bound = 2e-6f * (fabsf(q) + 2.f * fabsf(p));
    if (fabsf(y - thres) > bound) return y > thres;
  }
  const double dd = (double)d, ee = (double)e;
  const float nqp = (float)exp(-0.5 * (dd * dd));
  const float npp = (float)exp(-0.5 * (ee * ee));
  const float bb = nqp - npp;
  const float y = q * (1.f - nqp) + p * bb;
  return y > thres;
}

// FS = the number of taps (compile time: they sit in scalar registers and the window in vector registers), 0 = any number
// (taps and window read from LDS, a lane per bin).
template <int FS>
__global__ __launch_bounds__(64 * kCenRowsWaves) void cen2018_rows_kernel(const CenArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * kCenRowsWaves + wave;
  if (r >= a.rows) return;                                   // no workgroup barrier below
  const int b = blockIdx.y;
  const int cols = a.cols, mu = a.mu, fsize = a.fsize;
  float* qpad = (float*)(smem + (size_t)wave * a.per_wave);                   // qpad[mu + j] = q[j], j in [-mu, cols + mu)
  unsigned long long* bits = (unsigned long long*)(qpad + a.qlen);           // [lds_words] y > thres
  unsigned long long* tbits = bits + a.lds_words;                            // [lds_words] targets
  float* taps_l = (float*)(tbits + a.lds_words);                             // [fsize] (FS == 0)
  const uint8_t* rowp = a.polar + (long long)b * a.batch_stride + (long long)r * a.stride;
  const long long row = (long long)b * a.rows + r;
  const float mean = a.stats[row * 2], sigma = a.stats[row * 2 + 1];
  const float thres = a.zq * sigma;                                          // Utils.cpp:401

  // ---- stage q (Utils.cpp:360-362) and its BORDER_REFLECT101 halo --------------------------------------------------
  if ((((uintptr_t)rowp) & 3) == 0) {
    for (int j = lane * 4; j < cols; j += 256) {
      if (j + 4 <= cols) {
        const uint32_t w = *(const uint32_t*)(rowp + j);
#pragma unroll
        for (int by = 0; by < 4; by++) qpad[mu + j + by] = cen_f((w >> (8 * by)) & 0xffu) - mean;
      } else {
        for (int jj = j; jj < cols; jj++) qpad[mu + jj] = cen_f(rowp[jj]) - mean;
      }
    }
  } else {
    for (int j = lane; j < cols; j += 64) qpad[mu + j] = cen_f(rowp[j]) - mean;
  }
  for (int w = lane; w < a.lds_words; w += 64) tbits[w] = 0ull;
  if (FS == 0)
    for (int k = lane; k < fsize; k += 64) taps_l[k] = a.taps[k];
  cen_wave_sync();
  for (int h = 1 + lane; h <= mu; h += 64) {                // 3 * sigma_gauss <= cols: one reflection
    qpad[mu - h] = qpad[mu + h];
    qpad[mu + cols - 1 + h] = qpad[mu + cols - 1 - h];
  }
  cen_wave_sync();

  // ---- filtered row (filter2D, Utils.cpp:378) and the detection bitmap (Utils.cpp:402-407) ---------------------------
  if (FS > 0) {
    constexpr int FSX = FS > 0 ? FS : 1;
    constexpr int J = kCenBinsPerLane, W = J + FSX - 1, WP = (W + 3) & ~3, MU = FSX / 2;
    float wk[FSX];
#pragma unroll
    for (int k = 0; k < FSX; k++) wk[k] = a.taps[k];        // wave-uniform
    for (int j00 = 0; j00 < cols; j00 += kCenPass) {
      const int j0 = j00 + lane * J;
      float win[WP];
#pragma unroll
      for (int t = 0; t < WP; t += 4) {
        const float4 v = *(const float4*)(qpad + j0 + t);    // inside qlen for every lane (see cen_qlen)
        win[t] = v.x; win[t + 1] = v.y; win[t + 2] = v.z; win[t + 3] = v.w;
      }
      float acc[J];
#pragma unroll
      for (int o = 0; o < J; o++) acc[o] = 0.f;
#pragma unroll
      for (int t = 0; t < W; t++)
#pragma unroll
        for (int o = 0; o < J; o++) {
          const int k = t - o;                               // ascending in t for every bin o
          if (k >= 0 && k < FSX) acc[o] = acc[o] + wk[k] * win[t];
        }
      uint32_t mb = 0;
#pragma unroll
      for (int o = 0; o < J; o++) {
        const int j = j0 + o;
        if (j >= a.min_range_bins && j < cols && cen_detect(win[MU + o], acc[o], sigma, thres)) mb |= 1u << o;
      }
      ((uint8_t*)bits)[j0 >> 3] = (uint8_t)mb;               // j0 < lds_words * 64
    }
  } else {
    for (int j00 = 0; j00 < a.lds_words * 64; j00 += 64) {
      const int j = j00 + lane;
      bool det = false;
      if (j < cols) {
        float acc = 0.f;
        for (int k = 0; k < fsize; k++) acc = acc + taps_l[k] * qpad[j + k];
        det = j >= a.min_range_bins && cen_detect(qpad[mu + j], acc, sigma, thres);
      }
      const unsigned long long bal = __ballot(det);
      if (lane == 0) bits[j00 >> 6] = bal;
    }
  }
  cen_wave_sync();

  // ---- one target per run (Utils.cpp:407-415): the run's end finds its start, element len / 2 is marked --------------
  if (a.det_mask) {
    uint8_t* mrow = a.det_mask + row * cols;
    for (int j = lane; j < cols; j += 64) mrow[j] = (uint8_t)((bits[j >> 6] >> (j & 63)) & 1ull);
  }
  int n_tgt = 0;
  for (int w0 = 0; w0 < a.words; w0 += 64) {
    const int wd = w0 + lane;
    const unsigned long long word = wd < a.words ? bits[wd] : 0ull;           // bins >= cols are clear
    const unsigned long long next = wd + 1 < a.words ? (bits[wd + 1] & 1ull) : 0ull;
    unsigned long long ends = word & ~((word >> 1) | (next << 63));
    while (ends) {
      const int e = __ffsll((long long)ends) - 1;
      ends &= ends - 1;
      const unsigned long long zeros_below = ~word & ((1ull << e) - 1ull);
      int start;
      if (zeros_below) {
        start = wd * 64 + (64 - __clzll((long long)zeros_below));
      } else {
        start = 0;
        for (int pw = wd - 1; pw >= 0; pw--) {
          const unsigned long long z = ~bits[pw];
          if (z) { start = pw * 64 + (64 - __clzll((long long)z)); break; }
        }
      }
      const int end = wd * 64 + e, len = end - start + 1;
      const int tgt = start + len / 2;                        // peak_points[peak_points.size() / 2]
      atomicOr(&tbits[tgt >> 6], 1ull << (tgt & 63));
      n_tgt++;
    }
  }
  n_tgt = wave_sum_i32(n_tgt);
  cen_wave_sync();
  for (int w = lane; w < a.words; w += 64) a.tgt_bits[row * a.words + w] = tbits[w];
  if (lane == 0) a.tgt_count[row] = n_tgt;
}

// Compaction in (row, bin) order: grid = (image, row slices).  Every workgroup scans all row counts and emits the rows of
// its slice, one wavefront per row: lane w lists the marked bins of word w in LDS (a wave scan of the popcounts places
// them), then one target per lane becomes a point.
__global__ __launch_bounds__(256) void cen2018_cloud_kernel(const CenArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int32_t* row_off = (int32_t*)smem;
  __shared__ int32_t wave_tot[4];
  __shared__ int32_t run_base;
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) run_base = 0;
  __syncthreads();
  for (int r0 = 0; r0 < a.rows; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const int v = r < a.rows ? a.tgt_count[(long long)b * a.rows + r] : 0;
    const int incl = wave_incl_scan_i32(v);
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int off = run_base;
    for (int wv = 0; wv < wave; wv++) off += wave_tot[wv];
    if (r < a.rows) row_off[r] = off + incl - v;
    __syncthreads();
    if (threadIdx.x == 0) run_base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    __syncthreads();
  }
  if (threadIdx.x == 0 && blockIdx.y == 0) a.n_points[b] = run_base;
  const uint8_t* img = a.polar + (long long)b * a.batch_stride;
  const int rows_per = (a.rows + (int)gridDim.y - 1) / (int)gridDim.y;
  const int rbeg = blockIdx.y * rows_per, rend = min(a.rows, rbeg + rows_per);
  unsigned short* dlist = (unsigned short*)(row_off + a.rows + 1) + (size_t)wave * 64 * 64;   // [64 words x 64 bits]
  for (int r = rbeg + wave; r < rend; r += 4) {
    const double cos_t = a.cos_t[r], sin_t = a.sin_t[r];
    int base = row_off[r];
    for (int w0 = 0; w0 < a.words; w0 += 64) {
      const int wd = w0 + lane;
      unsigned long long bits = wd < a.words ? a.tgt_bits[((long long)b * a.rows + r) * a.words + wd] : 0ull;
      const int pc = __popcll(bits);
      const int incl = wave_incl_scan_i32(pc);
      const int n = __builtin_amdgcn_readlane(incl, 63);
      int off = incl - pc;
      while (bits) {
        dlist[off++] = (unsigned short)(wd * 64 + __ffsll((long long)bits) - 1);
        bits &= bits - 1;
      }
      cen_wave_sync();
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane, idx = base + j;
        if (j < n && idx < a.cap_points) {
          const int bin = dlist[j];
          const double range = a.range_res * (double)bin;                   // ScanType.cpp:80: the bin EDGE
          float4 p;
          p.x = (float)(range * cos_t);                                     // ScanType.cpp:81-83
          p.y = (float)(range * sin_t);
          p.z = 0.f;
          p.w = (float)img[(long long)r * a.stride + bin];
          ((float4*)a.xyzi)[(long long)b * a.cap_points + idx] = p;
          if (a.targets) {
            a.targets[((long long)b * a.cap_points + idx) * 2] = r;
            a.targets[((long long)b * a.cap_points + idx) * 2 + 1] = bin;
          }
        }
      }
      cen_wave_sync();
      base += n;
    }
  }
}

int cen_lds_words(int cols) { return (cols + kCenPass - 1) / kCenPass * (kCenPass / 64); }
// the staged row: the halo, and what the last lane of the last pass reads ahead (bins that do not exist; never used)
int cen_qlen(int cols, int fsize) { return cen_lds_words(cols) * 64 + ((fsize + kCenBinsPerLane - 1 + 3) & ~3) + 4; }

}  // namespace

extern "C" void cfear_cen2018_params_default(cfear_cen2018_params* par) {
  if (!par) return;
  par->zq = 3.0f;                 // ScanType.cpp:72
  par->sigma_gauss = 17;
  par->min_range_bins = 2;        // int(sensor_min_distance = 2.5), used as a bin index (Utils.cpp:402)
  par->pad = 0;
  par->range_res = 0.04328;       // ScanType.h:62
}

extern "C" int cfear_filter_cen2018(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                    const cfear_cen2018_params* par, float* xyzi, int32_t* n_points, int32_t cap_points,
                                    int32_t* targets, uint8_t* det_mask, float* row_stats) {
  if (!polar || !desc || !par || !xyzi || !n_points || cap_points <= 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: null argument");
  if (desc->rows <= 0 || desc->cols <= 0 || desc->stride < desc->cols || desc->batch <= 0 ||
      (desc->batch > 1 && desc->batch_stride < (int64_t)desc->rows * desc->stride))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: bad polar descriptor");
  if (desc->cols > kCenMaxCols) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: cols > %d unsupported", kCenMaxCols);
  if (par->sigma_gauss < 1 || par->sigma_gauss % 2 == 0 || par->sigma_gauss > kCenMaxSigma)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: sigma_gauss must be odd and in [1, %d]", kCenMaxSigma);
  if (3 * par->sigma_gauss > desc->cols)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: %d taps do not fit %d bins", 3 * par->sigma_gauss, desc->cols);
  if (par->min_range_bins < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: min_range_bins < 0");
  if (!std::isfinite(par->zq) || !std::isfinite(par->range_res))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: zq and range_res must be finite");
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, cols = desc->cols, batch = desc->batch;
  const int fsize = 3 * par->sigma_gauss, mu = fsize / 2, words = (cols + 63) / 64;

  // the taps (Utils.cpp:366-376): exp in double with the host's libm, a serial float sum, one multiply per tap
  HostStage st(ctx, kWsFilter);
  float* h_taps = (float*)st.record((size_t)fsize * sizeof(float));
  {
    const float sig_sqr = (float)(par->sigma_gauss * par->sigma_gauss);
    float s = 0.f;
    for (int i = 0; i < fsize; i++) {
      h_taps[i] = (float)std::exp(-0.5 * (i - mu) * (i - mu) / sig_sqr);
      s += h_taps[i];
    }
    const float inv = (float)(1.0 / (double)s);             // Mat /= s (UNPINNED against OpenCV: DESIGN.md)
    for (int i = 0; i < fsize; i++) h_taps[i] = h_taps[i] * inv;
  }
  const size_t img_bytes = (size_t)rows * desc->stride;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(batch, kCenMaxGridY), kCenChunkBytes / std::max<size_t>(1, img_bytes)));

  CenArgs a{};
  const cfear_polar_desc dd = st.images(a.polar, polar, *desc);
  float* d_taps;
  int32_t* d_np;
  st.out(a.xyzi, xyzi, (size_t)batch * cap_points * 16);
  st.out(d_np, n_points, (size_t)batch * 4);
  if (targets) st.out(a.targets, targets, (size_t)batch * cap_points * 8);
  if (det_mask) st.out(a.det_mask, det_mask, (size_t)batch * rows * cols);
  st.out(a.stats, row_stats, (size_t)batch * rows * 8);     // a null row_stats gets a piece that is not copied back
  st.piece(d_taps, (size_t)fsize * sizeof(float));
  st.piece(a.tgt_bits, (size_t)chunk * rows * words * 8);
  st.piece(a.tgt_count, (size_t)chunk * rows * 4);
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2018: the image and the outputs must be all host or all device");
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(st.upload(d_taps, h_taps, (size_t)fsize * sizeof(float)));
  double *d_cos = nullptr, *d_sin = nullptr;
  CFEAR_CHECK(cfear_trig_tables(ctx, rows, &d_cos, &d_sin));

  a.rows = rows; a.cols = cols; a.stride = dd.stride;
  a.batch_stride = batch > 1 ? dd.batch_stride : (long long)img_bytes;
  a.fsize = fsize; a.mu = mu; a.min_range_bins = par->min_range_bins; a.zq = par->zq;
  a.taps = d_taps; a.words = words;
  a.lds_words = cen_lds_words(cols);
  a.qlen = cen_qlen(cols, fsize);
  a.per_wave = (a.qlen * 4 + a.lds_words * 16 + ((fsize + 3) & ~3) * 4 + 15) & ~15;
  a.cos_t = d_cos; a.sin_t = d_sin; a.range_res = par->range_res; a.cap_points = cap_points;
  typedef void (*RowsFn)(const CenArgs);
  const RowsFn rows_fn = fsize == 51 ? cen2018_rows_kernel<51> : fsize == 15 ? cen2018_rows_kernel<15> : cen2018_rows_kernel<0>;
  const size_t rows_lds = (size_t)a.per_wave * kCenRowsWaves;
  const size_t cloud_lds = (size_t)(rows + 1) * 4 + 4 * 64 * 64 * 2;
  if (rows_lds > 160 * 1024 || cloud_lds > 160 * 1024)
    return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "cen2018: %d x %d images with %d taps do not fit the LDS", rows, cols, fsize);
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)rows_fn, rows_lds));
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)cen2018_cloud_kernel, cloud_lds));

  const CenArgs base = a;
  for (int b0 = 0; b0 < batch; b0 += chunk) {
    CenArgs c = base;
    c.batch = std::min(chunk, batch - b0);
    c.polar = base.polar + (long long)b0 * base.batch_stride;
    c.stats = base.stats + (size_t)b0 * rows * 2;
    c.xyzi = base.xyzi + (size_t)b0 * cap_points * 4;
    c.n_points = d_np + b0;
    if (base.targets) c.targets = base.targets + (size_t)b0 * cap_points * 2;
    if (base.det_mask) c.det_mask = base.det_mask + (size_t)b0 * rows * cols;
    {
      ProfScope ps(ctx, "cen2018_stats");
      const long long n_rows = (long long)c.batch * rows;
      hipLaunchKernelGGL(cen2018_stats_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, c);
    }
    {
      ProfScope ps(ctx, "cen2018_rows");
      hipLaunchKernelGGL(rows_fn, dim3((rows + kCenRowsWaves - 1) / kCenRowsWaves, c.batch), dim3(64 * kCenRowsWaves), rows_lds,
                         ctx->stream, c);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());                 // the cloud kernel trusts what the row kernel leaves in the scratch
    {
      ProfScope ps(ctx, "cen2018_cloud");
      hipLaunchKernelGGL(cen2018_cloud_kernel, dim3(c.batch, kCenCloudSplit), dim3(256), cloud_lds, ctx->stream, c);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  std::vector<int32_t> counts((size_t)batch);
  st.fetch(counts.data(), d_np, (size_t)batch * 4);
  CFEAR_CHECK(st.finish());
  for (int b = 0; b < batch; b++)
    if (counts[b] > cap_points)
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "cen2018: image %d: %d targets > cap_points %d", b, counts[b], cap_points);
  return CFEAR_OK;
}
