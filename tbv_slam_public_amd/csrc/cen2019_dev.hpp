// cen2019_dev.hpp -- what cen2019.hip (the detector) and cen2019_audit.hip (which of its landmarks hang on the sort's tie
// order) share: the limits, the kernels' argument record, the device helpers of a staged row and of its bitmaps, the
// per-run segmented maximum, and the detector's kernel chain as host launchers.
#pragma once
#include "common.hpp"

typedef uint32_t c19_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned long long c19_u64;

constexpr int kC19MaxCols = 8192;
constexpr long long kC19MaxPixels = 1ll << 22;   // the fp64 sum of f is exact in any order up to here
constexpr int kC19CloudSplit = 4;
constexpr size_t kC19CloudLists = 4 * 64 * 64 * 2;                          // cen2019_cloud_kernel: a bin list per wavefront
constexpr int kC19MaxRows = (int)((160 * 1024 - kC19CloudLists - 8 * 1024) / 4) - 1;   // ... an offset per row, and its static tables
constexpr size_t kC19ChunkBytes = 64u << 20;     // image bytes per chunk
constexpr size_t kC19KeyBytes = 256u << 20;      // selection-buffer bytes per chunk (8 per pixel; the audit: 16)
constexpr int kC19MaxGridY = 65535;              // images per chunk: the row kernels have the image on gridDim.y
constexpr unsigned kC19None = 0xffffu;
constexpr uint32_t kC19FlatMask = 0x3fffffu;     // 22 bits of flat index in a key
constexpr int kC19Digit = 11, kC19Bins = 1 << kC19Digit, kC19Passes = 5;   // the radix select of the cut

struct C19Args {
  const uint8_t* polar;
  int rows, cols, stride, batch;
  long long batch_stride;
  int max_points, min_range_bins;
  int words;                         // 64-bin words per row
  int rowb_bytes;                    // LDS bytes of a staged row
  int per_wave;                      // LDS bytes per wavefront of the kernel being launched
  int tie_rev;                       // 0: equal h in ascending flat index (the library's order); 1: descending (the audit's witness)
  // scratch, per chunk
  float* row_maxg;                   // [batch][rows]
  double* row_sum;                   // [batch][rows]: sum of f, then sum of h
  float* img;                        // [batch][4]: mean, float(1 / maxg), mean_h, maxg
  c19_u64* keys;                     // [batch][rows][cols]: a row's fresh keys at the start of its piece
  int32_t* row_cnt;                  // [batch][rows][4]: candidates, fresh, processed, targets
  c19_u64* row_minkey;               // [batch][rows]: the smallest processed key
  c19_u64* cut;                      // [batch]: K
  c19_u64* mark_bits;                // [batch][rows][words]: R
  c19_u64* hpos_bits;                // [batch][rows][words]: h > 0
  c19_u64* tgt_bits;                 // [batch][rows][words]
  // outputs
  uint8_t* region_mask;              // optional [batch][rows][cols]
  float* image_stats;                // optional [batch][4]
  int32_t* counts;                   // optional [batch][3]
  const double* cos_t;
  const double* sin_t;
  double range_res;
  float* xyzi;
  int32_t* n_points;
  int32_t* targets;
  int cap_points;
};

struct C19Select {
  c19_u64 prefix;                    // the digits chosen so far
  int rank;                          // the key wanted is the rank-th largest of those that match prefix
  int active;                        // 0: the cutoff is not binding (or max_points == 0), a.cut is final
};

// ---- cen2019.hip's kernels, launched on ctx->stream over one chunk (c.batch sweeps) -------------------------------------------------
// the refusals of cfear_filter_cen2019 that do not concern its outputs; CFEAR_OK or the error, set
int c19_check_input(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, const cfear_cen2019_params* par);
// range, image, hsum, image: c.img (mean, 1 / maxg, mean_h, maxg) of every sweep
int c19_launch_stats(cfear_ctx* ctx, const C19Args& c);
// the radix select alone: c.cut from c.keys and c.row_cnt[..][1]
void c19_launch_select(cfear_ctx* ctx, const C19Args& c, C19Select* d_sel, int* d_hist);
// fresh, select, mark, emit under the tie order c.tie_rev: c.row_cnt, c.row_minkey, c.cut, c.mark_bits, c.hpos_bits, c.tgt_bits
int c19_launch_detect(cfear_ctx* ctx, const C19Args& c, C19Select* d_sel, int* d_hist);
// wavefronts (rows) per workgroup of a row kernel whose wavefront needs per_wave bytes of LDS: up to 4, within 64 KB
inline int c19_waves(int per_wave) { return std::max(1, std::min(4, (64 * 1024) / per_wave)); }
// LDS of a wavefront of the fresh kernel: rowb | neg u64 [words + 1] | cand u64 [words] | tail u64 [64] | prevz, nextz int
// [words + 1] each | bound int [64] | runtop u16 [cols].  A key is recomputed from the row's bytes wherever it is needed (a
// run's own candidates, three per run, the fresh ones): a table of them would halve the wavefronts a compute unit holds.
__host__ __device__ inline int c19_fresh_lds(int cols, int words, int rowb_bytes) {
  return rowb_bytes + (2 * words + 1 + 64) * 8 + (2 * (words + 1) + 64) * 4 + ((cols * 2 + 15) & ~15);
}

#ifdef __HIPCC__
static __device__ __forceinline__ float c19_f(uint32_t byte) { return (float)byte * (float)(1 / 255.0); }   // convertTo(CV_32F, 1/255.0)

static __device__ __forceinline__ void c19_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static __device__ __forceinline__ c19_u64 c19_wave_max_u64(c19_u64 v) {
  for (int o = 32; o; o >>= 1) {
    const c19_u64 t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  return v;
}
static __device__ __forceinline__ float c19_wave_max_f32(float v) {
  for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// the row's bytes into LDS; the caller synchronises the wavefront
static __device__ __forceinline__ void c19_stage_row(const uint8_t* rowp, int cols, uint8_t* rowb, int lane) {
  int done = 0;
  if ((((uintptr_t)rowp) & 3) == 0) {
    done = cols & ~15;
    for (int j = lane * 16; j < done; j += 64 * 16) *(c19_u32x4*)(rowb + j) = *(const c19_u32x4*)(rowp + j);
  }
  for (int j = done + lane; j < cols; j += 64) rowb[j] = rowp[j];
}

// |f[j + 1] - f[j - 1]| with BORDER_REFLECT101: 0 in the first and the last bin (Utils.cpp:499-504)
static __device__ __forceinline__ float c19_grad(const uint8_t* rowb, int j, int cols) {
  return (j > 0 && j < cols - 1) ? fabsf(c19_f(rowb[j + 1]) - c19_f(rowb[j - 1])) : 0.f;
}
// s and h of bin j (Utils.cpp:507-512); inv = float(1 / double(maxg)), infinite for a flat sweep (h is NaN then, as in the reference)
static __device__ __forceinline__ void c19_sh(const uint8_t* rowb, int j, int cols, float mean, float inv, float& s, float& h) {
  const float g = c19_grad(rowb, j, cols) * inv;
  s = c19_f(rowb[j]) - mean;
  h = s * (1.f - g);
}
// descending h = descending key; -0 and +0 are one value (the comparison of the reference's sort)
static __device__ __forceinline__ uint32_t c19_ord(float h) {
  const uint32_t u = __float_as_uint(h == 0.f ? 0.f : h);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ float c19_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
// the low key bits of flat index `flat` are flat ^ tie: tie = kC19FlatMask makes them descending in the index, so that among
// equal h the smaller index holds the larger key and comes first; tie = 0 the other way round
static __device__ __forceinline__ uint32_t c19_tie(int tie_rev) { return tie_rev ? 0u : kC19FlatMask; }
// 54 bits: 32 of h, 22 of the flat index (rows * cols <= 2^22)
static __device__ __forceinline__ c19_u64 c19_key(uint32_t ord, uint32_t flat, uint32_t tie) { return ((c19_u64)ord << 22) | (c19_u64)(flat ^ tie); }
static __device__ __forceinline__ uint32_t c19_key_flat(c19_u64 key, uint32_t tie) { return (uint32_t)(key & (c19_u64)kC19FlatMask) ^ tie; }

static __device__ __forceinline__ bool c19_bit(const c19_u64* bits, int j) { return (bits[j >> 6] >> (j & 63)) & 1ull; }

// prevz[w] = the last bin before word w with a clear bit (-1: none), nextz[w] = the first bin from word w on with a clear
// bit (words * 64: none), w = 0 .. words.  Bins >= cols are clear.
static __device__ __forceinline__ void c19_zero_tables(const c19_u64* bits, int words, int* prevz, int* nextz, int lane) {
  for (int w = lane; w <= words; w += 64) {
    int pz = -1, nz = words * 64;
    for (int p = w - 1; p >= 0; p--) {
      const c19_u64 z = ~bits[p];
      if (z) { pz = p * 64 + 63 - __clzll((long long)z); break; }
    }
    for (int p = w; p < words; p++) {
      const c19_u64 z = ~bits[p];
      if (z) { nz = p * 64 + __ffsll((long long)z) - 1; break; }
    }
    prevz[w] = pz;
    nextz[w] = nz;
  }
}
// first bin of the run of set bits that ends at, or contains, bin j (bit j itself is not looked at)
static __device__ __forceinline__ int c19_run_start(const c19_u64* bits, const int* prevz, int j) {
  const int w = j >> 6, b = j & 63;
  const c19_u64 zb = ~bits[w] & ((1ull << b) - 1ull);
  return zb ? w * 64 + 64 - __clzll((long long)zb) : prevz[w] + 1;
}
// last bin of the run of set bits that contains bin j
static __device__ __forceinline__ int c19_run_end(const c19_u64* bits, const int* nextz, int j) {
  const int w = j >> 6, b = j & 63;
  const c19_u64 za = b == 63 ? 0ull : (~bits[w] & ~((2ull << b) - 1ull));
  return (za ? w * 64 + __ffsll((long long)za) - 1 : nextz[w + 1]) - 1;
}
// the highest set bit of bits[] in [u, v], -1 if none
static __device__ __forceinline__ int c19_highest(const c19_u64* bits, int u, int v) {
  for (int w = v >> 6; w >= (u >> 6); w--) {
    c19_u64 m = bits[w];
    if (w == (v >> 6) && (v & 63) != 63) m &= (2ull << (v & 63)) - 1ull;
    if (w == (u >> 6)) m &= ~((1ull << (u & 63)) - 1ull);
    if (m) return w * 64 + 63 - __clzll((long long)m);
  }
  return -1;
}
static __device__ __forceinline__ void c19_set_range(c19_u64* bits, int u, int v) {
  for (int w = u >> 6; w <= (v >> 6); w++) {
    c19_u64 m = ~0ull;
    if (w == (v >> 6) && (v & 63) != 63) m &= (2ull << (v & 63)) - 1ull;
    if (w == (u >> 6)) m &= ~((1ull << (u & 63)) - 1ull);
    atomicOr(&bits[w], m);
  }
}
// the ends of the runs of set bits of word w: a set bit whose successor (in the next word for bit 63; bits[words] is 0) is clear
static __device__ __forceinline__ c19_u64 c19_run_ends(const c19_u64* bits, int w) {
  const c19_u64 word = bits[w];
  return word & ~((word >> 1) | ((bits[w + 1] & 1ull) << 63));
}

// runtop[v], for every run [u, v] of neg: the bin of the best candidate TOUCHING it under the tie order `tie` -- its own
// candidates, the one right of it, the one left of it if that sits below T -- or kC19None.  key_of(j) is bin j's key in that
// order.  The own candidates by a segmented maximum, a lane per stretch of C bins (C odd: no LDS bank conflicts), carries
// through tail u64 [64] and bound int [64].  neg and cand are visible on entry, runtop is on return.
template <class KeyOf>
static __device__ __forceinline__ void c19_run_tops(const c19_u64* neg, const c19_u64* cand, const int* prevz, c19_u64* tail, int* bound,
                                                    unsigned short* runtop, int cols, int words, int T, uint32_t flat0, uint32_t tie,
                                                    int lane, KeyOf key_of) {
  {
    const int C = ((cols + 63) / 64) | 1;
    const int j_beg = lane * C, j_end = min(cols, j_beg + C);
    c19_u64 cur = 0ull, first_best = 0ull;
    int first_end = -1;
    bool from_start = true, closed = j_beg >= cols;
    for (int j = j_beg; j < j_end; j++) {
      if (c19_bit(neg, j)) {
        if (c19_bit(cand, j)) {
          const c19_u64 k = key_of(j);
          cur = k > cur ? k : cur;
        }
        if (j == cols - 1 || !c19_bit(neg, j + 1)) {           // the run ends here
          if (from_start) { first_end = j; first_best = cur; }
          else runtop[j] = cur ? (unsigned short)(c19_key_flat(cur, tie) - flat0) : (unsigned short)kC19None;
          cur = 0ull;
          closed = true;
          from_start = false;
        }
      } else {
        cur = 0ull;
        closed = true;
        from_start = false;
      }
    }
    tail[lane] = cur;
    bound[lane] = closed;
    c19_wave_sync();
    if (first_end >= 0) {                                      // the run may have begun in the stretches before
      c19_u64 best = first_best;
      for (int p = lane - 1; p >= 0; p--) {
        const c19_u64 t = tail[p];
        best = t > best ? t : best;
        if (bound[p]) break;
      }
      runtop[first_end] = best ? (unsigned short)(c19_key_flat(best, tie) - flat0) : (unsigned short)kC19None;
    }
  }
  c19_wave_sync();
  for (int w = lane; w < words; w += 64) {
    c19_u64 ends = c19_run_ends(neg, w);
    while (ends) {
      const int v = w * 64 + __ffsll((long long)ends) - 1;
      ends &= ends - 1;
      const int u = c19_run_start(neg, prevz, v);
      unsigned top = runtop[v];
      c19_u64 ktop = top != kC19None ? key_of((int)top) : 0ull;
      if (v + 1 < cols && c19_bit(cand, v + 1)) {
        const c19_u64 k = key_of(v + 1);
        if (k > ktop) { ktop = k; top = v + 1; }
      }
      if (u >= 1 && u - 1 < T && c19_bit(cand, u - 1)) {
        const c19_u64 k = key_of(u - 1);
        if (k > ktop) { ktop = k; top = u - 1; }
      }
      runtop[v] = (unsigned short)top;
    }
  }
  c19_wave_sync();
}
#endif  // __HIPCC__
