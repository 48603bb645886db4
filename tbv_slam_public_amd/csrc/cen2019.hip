// cen2019.hip -- Cen and Newman's 2019 radar landmark detector as a batched polar filter on gfx950.
//
// Replaces (coral_alignment_quality/src/alignment_checker/):
//   cen2019features                Utils.cpp:436-594 (findRangeBoundaries, checkAdjacentMarked, getMaxInRegion included)
//   convertTo(CV_32F, 1/255.0)     ScanType.cpp:94
// The reference stops at `targets`: Cen2019Radar's constructor body is commented out (ScanType.cpp:90-101).  The cloud step
// here is Cen2018Radar's (ScanType.cpp:68-88): theta = (row + 1) / rows * 2 pi, r = range_res * bin, intensity = the byte.
//
// The reference sorts every pixel with h > mean_h by descending h and walks the sorted list serially, marking intervals
// until max_points of them were `fresh`.  Neither the sort nor the serial walk is done here (tests/cen2019_cpu.py states
// the equivalence and test_cen2019_cpu.py checks it against the literal loops).  With key = (h descending, flat index
// ascending), T = rows - 1 and a `run` a maximal stretch of bins with s < 0:
//   * a candidate is fresh iff it holds the best key among the candidates touching each run it touches (a run's own
//     candidates, the s >= 0 candidate right of it, and the one left of it if that sits at r < T);
//   * the loop processes exactly the candidates with key >= K, K the key of the max_points-th best fresh candidate;
//   * a run's marks are a prefix [u, M], decided from the processed candidates touching it (cen2019_mark_kernel).
// Every float operation rounds on its own (the library is built -ffp-contract=off).  Kernels, per chunk of sweeps (a chunk's
// sweeps stay in the Infinity Cache, so they come from HBM once and are read on-die three more times):
//   cen2019_range_kernel    a wavefront per row: the row's largest |f[r+1] - f[r-1]| and its fp64 sum of f (exact in any order
//                           while rows * cols <= 2^22)
//   cen2019_image_kernel    a workgroup per sweep: maxg, mean; in a second launch mean_h from the rows' fp64 sums of h
//   cen2019_hsum_kernel     a wavefront per row: the fp64 sum of h, in an order that depends on the row's width alone
//   cen2019_fresh_kernel    a wavefront per row: the s < 0 and candidate bitmaps by ballot, the best own
//                           candidate of every run by a segmented maximum (a lane per stretch of bins, carries through LDS),
//                           the fresh flags, and the fresh keys compacted into the row's piece of the selection buffer
//   cen2019_hist / _pick    radix select (11 bits a pass, 5 passes) of the max_points-th largest fresh key of every sweep
//   cen2019_mark_kernel     a wavefront per row: the processed candidates and the marks R as LDS bitmaps -> global bitmaps
//   cen2019_emit_kernel     a wavefront per row: R of the row and of its two neighbours (wrapping), the runs an unmarked bin
//                           ends, their adjacency test and getMaxInRegion's bin -> target bitmap
//   cen2019_cloud_kernel    compaction in (row, bin) order without atomics, as cen2018_cloud_kernel; also the sweep's counts
// The limits, C19Args, the device helpers and the launchers c19_launch_* live in cen2019_dev.hpp: cen2019_audit.hip runs this
// chain twice (C19Args::tie_rev = 1 reverses the order among equal h; the filter always passes 0) and the select on key sets of its own.
// Rows are read with 16-byte loads only where all 16 bytes lie inside the row, and byte by byte elsewhere (ragged widths,
// odd strides, rows narrower than a piece): nothing is read beyond a row's own `cols` bytes.
#include <cmath>

#include "cen2019_dev.hpp"

namespace {

typedef c19_u64 u64;

// ---- the row's largest gradient and its sum of f ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cen2019_range_kernel(const C19Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;                                   // no workgroup barrier below
  const int b = blockIdx.y, cols = a.cols;
  uint8_t* rowb = smem + (size_t)wave * a.per_wave;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  float mg = 0.f;
  double sum = 0.0;
  for (int j = lane; j < cols; j += 64) {
    mg = fmaxf(mg, c19_grad(rowb, j, cols));
    sum += (double)c19_f(rowb[j]);
  }
  mg = c19_wave_max_f32(mg);
  sum = wave_sum_f64(sum);
  if (lane == 0) {
    a.row_maxg[(long long)b * a.rows + r] = mg;
    a.row_sum[(long long)b * a.rows + r] = sum;
  }
}

// stage 0: maxg, mean = float(sum f / N), float(1 / double(maxg)) (Utils.cpp:505-510); stage 1: mean_h (Utils.cpp:513)
__global__ __launch_bounds__(256) void cen2019_image_kernel(const C19Args a, int stage) {
  __shared__ double sh_sum[256];
  __shared__ float sh_max[256];
  const int b = blockIdx.x, t = threadIdx.x;
  double sum = 0.0;
  float mg = 0.f;
  for (int r = t; r < a.rows; r += 256) {
    sum += a.row_sum[(long long)b * a.rows + r];
    if (stage == 0) mg = fmaxf(mg, a.row_maxg[(long long)b * a.rows + r]);
  }
  sh_sum[t] = sum;
  sh_max[t] = mg;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if (t < o) {
      sh_sum[t] += sh_sum[t + o];
      sh_max[t] = fmaxf(sh_max[t], sh_max[t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const double n = (double)((long long)a.rows * a.cols);
    if (stage == 0) {
      a.img[b * 4] = (float)(sh_sum[0] / n);
      a.img[b * 4 + 1] = (float)(1.0 / (double)sh_max[0]);   // g /= maxg (UNPINNED against OpenCV: DESIGN.md)
      a.img[b * 4 + 3] = sh_max[0];
    } else {
      a.img[b * 4 + 2] = a.img[b * 4 + 3] == 0.f ? __builtin_nanf("") : (float)(sh_sum[0] / n);
    }
  }
}

__global__ __launch_bounds__(256) void cen2019_hsum_kernel(const C19Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;
  const int b = blockIdx.y, cols = a.cols;
  uint8_t* rowb = smem + (size_t)wave * a.per_wave;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  const float mean = a.img[b * 4], inv = a.img[b * 4 + 1];
  double sum = 0.0;
  for (int j = lane; j < cols; j += 64) {
    float s, h;
    c19_sh(rowb, j, cols, mean, inv, s, h);
    sum += (double)h;
  }
  sum = wave_sum_f64(sum);
  if (lane == 0) a.row_sum[(long long)b * a.rows + r] = sum;
}

// LDS of a wavefront: c19_fresh_lds (cen2019_dev.hpp)
__global__ __launch_bounds__(256) void cen2019_fresh_kernel(const C19Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;
  const int b = blockIdx.y, cols = a.cols, words = a.words, T = a.rows - 1;
  uint8_t* rowb = smem + (size_t)wave * a.per_wave;
  u64* neg = (u64*)(rowb + a.rowb_bytes);
  u64* cand = neg + words + 1;
  u64* tail = cand + words;
  int* prevz = (int*)(tail + 64);
  int* nextz = prevz + words + 1;
  int* bound = nextz + words + 1;
  unsigned short* runtop = (unsigned short*)(bound + 64);
  const long long row = (long long)b * a.rows + r;
  const uint32_t flat0 = (uint32_t)r * (uint32_t)cols;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  const float mean = a.img[b * 4], inv = a.img[b * 4 + 1], mean_h = a.img[b * 4 + 2];
  const uint32_t tie = c19_tie(a.tie_rev);
  const auto key_of = [&](int j) {
    float s, h;
    c19_sh(rowb, j, cols, mean, inv, s, h);
    return c19_key(c19_ord(h), flat0 + j, tie);
  };

  // ---- the s < 0 and candidate bitmaps (Utils.cpp:517-523) -------------------------------------------------------------
  int n_cand = 0;
  for (int j0 = 0; j0 < words * 64; j0 += 64) {
    const int j = j0 + lane;
    bool ng = false, cd = false;
    if (j < cols) {
      float s, h;
      c19_sh(rowb, j, cols, mean, inv, s, h);
      ng = s < 0.f;
      cd = h > mean_h;
    }
    const u64 bn = __ballot(ng), bc = __ballot(cd);
    if (lane == 0) { neg[j0 >> 6] = bn; cand[j0 >> 6] = bc; }
    n_cand += __popcll(bc);
  }
  if (lane == 0) neg[words] = 0ull;
  c19_wave_sync();
  c19_zero_tables(neg, words, prevz, nextz, lane);

  // ---- the best candidate TOUCHING every run: its own, the one right of it, the one left of it if that sits below T --------------
  c19_run_tops(neg, cand, prevz, tail, bound, runtop, cols, words, T, flat0, tie, lane, key_of);

  // ---- fresh candidates: the best key in each run they touch; their keys, compacted --------------------------------------------
  u64* seg = a.keys + row * cols;
  int n_fresh = 0;
  for (int j0 = 0; j0 < words * 64; j0 += 64) {
    const int j = j0 + lane;
    bool fresh = false;
    if (j < cols && c19_bit(cand, j)) {
      if (c19_bit(neg, j)) {
        fresh = runtop[c19_run_end(neg, nextz, j)] == j;
      } else {
        fresh = true;
        if (j >= 1 && c19_bit(neg, j - 1)) fresh = runtop[j - 1] == j;
        if (fresh && j < T && j + 1 < cols && c19_bit(neg, j + 1)) fresh = runtop[c19_run_end(neg, nextz, j + 1)] == j;
      }
    }
    const u64 bf = __ballot(fresh);
    if (fresh) seg[n_fresh + __popcll(bf & ((1ull << lane) - 1ull))] = key_of(j);
    n_fresh += __popcll(bf);
  }
  if (lane == 0) {
    a.row_cnt[row * 4] = n_cand;
    a.row_cnt[row * 4 + 1] = n_fresh;
  }
}

// K = the key of the max_points-th best fresh candidate (Utils.cpp:531: the loop ends when l == max_points); 0 when fewer
// are fresh (every candidate is processed), all ones for max_points == 0 (none is).  Radix select over the 54 key bits, 11 a
// pass: cen2019_hist_kernel counts the keys that match the digits chosen so far by their next digit (several workgroups a
// sweep, LDS histograms flushed with atomics: a count does not depend on the order), cen2019_pick_kernel chooses the digit.
__global__ __launch_bounds__(256) void cen2019_select_init_kernel(const C19Args a, C19Select* sel, int* ghist) {
  __shared__ int sh_tot[4];
  const int b = blockIdx.x, t = threadIdx.x;
  int tot = 0;
  for (int r = t; r < a.rows; r += 256) tot += a.row_cnt[((long long)b * a.rows + r) * 4 + 1];
  tot = wave_sum_i32(tot);
  if ((t & 63) == 0) sh_tot[t >> 6] = tot;
  for (int i = t; i < kC19Bins; i += 256) ghist[(long long)b * kC19Bins + i] = 0;
  __syncthreads();
  if (t == 0) {
    tot = sh_tot[0] + sh_tot[1] + sh_tot[2] + sh_tot[3];
    const bool binding = a.max_points > 0 && tot >= a.max_points;
    sel[b].prefix = 0ull;
    sel[b].rank = a.max_points;
    sel[b].active = binding;
    if (!binding) a.cut[b] = a.max_points <= 0 ? ~0ull : 0ull;
  }
}

__global__ __launch_bounds__(256) void cen2019_hist_kernel(const C19Args a, const C19Select* sel, int* ghist, int shift) {
  __shared__ int hist[kC19Bins];
  const int b = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (!sel[b].active) return;                                  // uniform over the workgroup
  for (int i = t; i < kC19Bins; i += 256) hist[i] = 0;
  __syncthreads();
  const u64 prefix = sel[b].prefix;
  const u64 mask = ~((1ull << (shift + kC19Digit)) - 1ull);     // shift + 11 <= 55
  for (int r = blockIdx.y * 4 + wave; r < a.rows; r += gridDim.y * 4) {
    const long long row = (long long)b * a.rows + r;
    const int n = a.row_cnt[row * 4 + 1];
    const u64* seg = a.keys + row * a.cols;
    for (int i = lane; i < n; i += 64) {
      const u64 k = seg[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(int)((k >> shift) & (u64)(kC19Bins - 1))], 1);
    }
  }
  __syncthreads();
  for (int i = t; i < kC19Bins; i += 256)
    if (hist[i]) atomicAdd(&ghist[(long long)b * kC19Bins + i], hist[i]);
}

__global__ __launch_bounds__(256) void cen2019_pick_kernel(const C19Args a, C19Select* sel, int* ghist, int shift) {
  __shared__ int hist[kC19Bins];
  __shared__ int chunk[256];
  const int b = blockIdx.x, t = threadIdx.x;
  if (!sel[b].active) return;
  int sum = 0;
  for (int i = 0; i < kC19Bins / 256; i++) {                    // thread t holds bins [8 t, 8 t + 8)
    const int v = ghist[(long long)b * kC19Bins + t * (kC19Bins / 256) + i];
    hist[t * (kC19Bins / 256) + i] = v;
    sum += v;
    ghist[(long long)b * kC19Bins + t * (kC19Bins / 256) + i] = 0;   // for the next pass
  }
  chunk[t] = sum;
  __syncthreads();
  if (t == 0) {
    int rank = sel[b].rank, c = 255;
    for (; c > 0; c--) {
      if (rank <= chunk[c]) break;
      rank -= chunk[c];
    }
    int d = c * (kC19Bins / 256) + kC19Bins / 256 - 1;
    for (; d > c * (kC19Bins / 256); d--) {
      if (rank <= hist[d]) break;
      rank -= hist[d];
    }
    const u64 prefix = sel[b].prefix | ((u64)d << shift);
    sel[b].prefix = prefix;
    sel[b].rank = rank;
    if (shift == 0) a.cut[b] = prefix;
  }
}

// LDS of a wavefront of the mark kernel: rowb | neg u64 [words + 1] | proc, marks u64 [words] each | prevz, nextz int [words + 1] | straddle int [4]
__host__ __device__ inline int c19_mark_lds(int words, int rowb_bytes) { return rowb_bytes + (3 * words + 1) * 8 + (2 * (words + 1) + 4) * 4 + 8; }

__global__ __launch_bounds__(256) void cen2019_mark_kernel(const C19Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;
  const int b = blockIdx.y, cols = a.cols, words = a.words, T = a.rows - 1;
  uint8_t* rowb = smem + (size_t)wave * a.per_wave;
  u64* neg = (u64*)(rowb + a.rowb_bytes);
  u64* proc = neg + words + 1;
  u64* marks = proc + words;
  int* prevz = (int*)(marks + words);
  int* nextz = prevz + words + 1;
  int* straddle = nextz + words + 1;                           // u, v of the run whose best processed candidate decides
  const long long row = (long long)b * a.rows + r;
  const uint32_t flat0 = (uint32_t)r * (uint32_t)cols;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  const float mean = a.img[b * 4], inv = a.img[b * 4 + 1], mean_h = a.img[b * 4 + 2];
  const u64 K = a.cut[b];
  const uint32_t tie = c19_tie(a.tie_rev);

  // ---- the processed candidates (key >= K); R starts as those with s >= 0: their own bins ----------------------------------------
  int n_proc = 0;
  u64 kmin = ~0ull;
  for (int j0 = 0; j0 < words * 64; j0 += 64) {
    const int j = j0 + lane;
    bool ng = false, pr = false, hp = false;
    if (j < cols) {
      float s, h;
      c19_sh(rowb, j, cols, mean, inv, s, h);
      ng = s < 0.f;
      hp = h > 0.f;
      if (h > mean_h) {
        const u64 k = c19_key(c19_ord(h), flat0 + j, tie);
        pr = k >= K;
        if (pr) kmin = k < kmin ? k : kmin;
      }
    }
    const u64 bn = __ballot(ng), bp = __ballot(pr), bh = __ballot(hp);
    if (lane == 0) {
      neg[j0 >> 6] = bn;
      proc[j0 >> 6] = bp;
      marks[j0 >> 6] = bp & ~bn;
      a.hpos_bits[row * words + (j0 >> 6)] = bh;
    }
    n_proc += __popcll(bp);
  }
  if (lane == 0) { neg[words] = 0ull; straddle[0] = -1; straddle[1] = -1; }
  c19_wave_sync();
  c19_zero_tables(neg, words, prevz, nextz, lane);
  c19_wave_sync();

  // ---- the marks of every run [u, v]: a prefix [u, M] ------------------------------------------------------------------------------
  for (int w = lane; w < words; w += 64) {
    const u64 word = neg[w];
    u64 ends = word & ~((word >> 1) | ((neg[w + 1] & 1ull) << 63));
    while (ends) {
      const int v = w * 64 + __ffsll((long long)ends) - 1;
      ends &= ends - 1;
      const int u = c19_run_start(neg, prevz, v);
      int M = -1;
      if ((v + 1 < cols && c19_bit(proc, v + 1)) || (u >= 1 && u - 1 < T && c19_bit(proc, u - 1))) {
        M = v;                                                 // a processed s >= 0 neighbour extends over the whole run
      } else {
        const int top = c19_highest(proc, u, v);               // the furthest own processed candidate
        if (top >= 0) {
          if (top < T) M = v;                                  // every own processed candidate extends right (r < T)
          else if (u >= T) M = top;                            // none does
          else { straddle[0] = u; straddle[1] = v; }           // the run straddles column T: the best of them decides
        }
      }
      if (M >= 0) c19_set_range(marks, u, M);
    }
  }
  c19_wave_sync();
  if (straddle[1] >= 0) {                                      // wave-uniform; at most one run of a row contains columns T - 1 and T
    const int u = straddle[0], v = straddle[1];
    u64 best = 0ull;
    for (int j = u + lane; j <= v; j += 64)
      if (c19_bit(proc, j)) {
        float s, h;
        c19_sh(rowb, j, cols, mean, inv, s, h);
        const u64 k = c19_key(c19_ord(h), flat0 + j, tie);
        best = k > best ? k : best;
      }
    best = c19_wave_max_u64(best);
    const int bin = (int)(c19_key_flat(best, tie) - flat0);
    // the best at r < T marks the whole run, and every later one finds its bin marked; the best at r >= T marks [u, r], the
    // others at r' >= T extend that to r', and those at r < T find their bin marked and are skipped
    if (lane == 0) c19_set_range(marks, u, bin < T ? v : c19_highest(proc, u, v));
  }
  c19_wave_sync();
  for (int w = lane; w < words; w += 64) a.mark_bits[row * words + w] = marks[w];
  if (a.region_mask) {
    uint8_t* mrow = a.region_mask + row * cols;
    for (int j = lane; j < cols; j += 64) mrow[j] = (uint8_t)c19_bit(marks, j);
  }
  kmin = ~c19_wave_max_u64(~kmin);
  if (lane == 0) {
    a.row_cnt[row * 4 + 2] = n_proc;
    a.row_minkey[row] = kmin;
  }
}

// Utils.cpp:553-578.  LDS of a wavefront: own (bins below min_range cleared), below, above, hpos, tbits: u64 [words + 1] each
__global__ __launch_bounds__(256) void cen2019_emit_kernel(const C19Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;
  const int b = blockIdx.y, cols = a.cols, words = a.words;
  u64* own = (u64*)(smem + (size_t)wave * a.per_wave);
  u64* adj = own + words + 1;                                  // below | above
  u64* hpos = adj + words + 1;
  u64* tbits = hpos + words + 1;
  const long long img_row0 = (long long)b * a.rows, row = img_row0 + r;
  const int below = r - 1 < 0 ? a.rows - 1 : r - 1, above = r + 1 >= a.rows ? 0 : r + 1;
  for (int w = lane; w <= words; w += 64) {
    u64 o = 0ull, ad = 0ull, hp = 0ull;
    if (w < words) {
      o = a.mark_bits[row * words + w];
      ad = a.mark_bits[(img_row0 + below) * words + w] | a.mark_bits[(img_row0 + above) * words + w];
      hp = a.hpos_bits[row * words + w];
      const int lo = a.min_range_bins - w * 64;                // bins below min_range are not looked at (Utils.cpp:559)
      if (lo >= 64) o = 0ull;
      else if (lo > 0) o &= ~((1ull << lo) - 1ull);
    }
    own[w] = o; adj[w] = ad; hpos[w] = hp; tbits[w] = 0ull;
  }
  c19_wave_sync();
  int n_tgt = 0;
  for (int w = lane; w < words; w += 64) {
    const u64 word = own[w];
    u64 ends = word & ~((word >> 1) | ((own[w + 1] & 1ull) << 63));
    if (w == ((cols - 1) >> 6)) ends &= ~(1ull << ((cols - 1) & 63));   // only an unmarked bin ends a run: none follows the last column
    while (ends) {
      const int e = __ffsll((long long)ends) - 1;
      ends &= ends - 1;
      const u64 zeros_below = ~word & ((1ull << e) - 1ull);
      int start = 0;
      if (zeros_below) {
        start = w * 64 + 64 - __clzll((long long)zeros_below);
      } else {
        for (int pw = w - 1; pw >= 0; pw--) {
          const u64 z = ~own[pw];
          if (z) { start = pw * 64 + 64 - __clzll((long long)z); break; }
        }
      }
      const int end = w * 64 + e;
      if (c19_highest(adj, start, end) < 0) continue;          // checkAdjacentMarked
      // getMaxInRegion: `int max = -1000; if (h > max) { max = h; max_r = r; }` -- |h| < 1, so max becomes 0 at the run's
      // first bin and stays 0: the first bin, then every later bin with h > 0, is taken; the last taken stands
      const int hi = c19_highest(hpos, start, end);
      const int tgt = hi >= 0 ? hi : start;
      atomicOr(&tbits[tgt >> 6], 1ull << (tgt & 63));
      n_tgt++;
    }
  }
  n_tgt = wave_sum_i32(n_tgt);
  c19_wave_sync();
  for (int w = lane; w < words; w += 64) a.tgt_bits[row * words + w] = tbits[w];
  if (lane == 0) a.row_cnt[row * 4 + 3] = n_tgt;
}

// Compaction in (row, bin) order, as cen2018_cloud_kernel: grid = (image, row slices); every workgroup scans all row counts
// and emits the rows of its slice, one wavefront per row.  Slice 0 also leaves the sweep's counts and image_stats.
__global__ __launch_bounds__(256) void cen2019_cloud_kernel(const C19Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int32_t* row_off = (int32_t*)smem;
  __shared__ int32_t wave_tot[4];
  __shared__ int32_t run_base;
  __shared__ int32_t sh_cnt[3][256];
  __shared__ u64 sh_min[256];
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) run_base = 0;
  __syncthreads();
  int cnt[3] = {0, 0, 0};
  u64 kmin = ~0ull;
  for (int r0 = 0; r0 < a.rows; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const long long row = (long long)b * a.rows + r;
    const int v = r < a.rows ? a.row_cnt[row * 4 + 3] : 0;
    if (r < a.rows) {
      for (int c = 0; c < 3; c++) cnt[c] += a.row_cnt[row * 4 + c];
      const u64 k = a.row_minkey[row];
      kmin = k < kmin ? k : kmin;
    }
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
  if (blockIdx.y == 0) {
    for (int c = 0; c < 3; c++) sh_cnt[c][threadIdx.x] = cnt[c];
    sh_min[threadIdx.x] = kmin;
    __syncthreads();
    for (int o = 128; o; o >>= 1) {
      if ((int)threadIdx.x < o) {
        for (int c = 0; c < 3; c++) sh_cnt[c][threadIdx.x] += sh_cnt[c][threadIdx.x + o];
        const u64 k = sh_min[threadIdx.x + o];
        if (k < sh_min[threadIdx.x]) sh_min[threadIdx.x] = k;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      a.n_points[b] = run_base;
      if (a.counts)
        for (int c = 0; c < 3; c++) a.counts[b * 3 + c] = sh_cnt[c][0];
      if (a.image_stats) {
        a.image_stats[b * 4] = a.img[b * 4];
        a.image_stats[b * 4 + 1] = a.img[b * 4 + 3];
        a.image_stats[b * 4 + 2] = a.img[b * 4 + 2];
        a.image_stats[b * 4 + 3] = sh_cnt[2][0] ? c19_unord((uint32_t)(sh_min[0] >> 22)) : 0.f;   // h of the last processed candidate
      }
    }
  }
  const uint8_t* img = a.polar + (long long)b * a.batch_stride;
  const int rows_per = (a.rows + (int)gridDim.y - 1) / (int)gridDim.y;
  const int rbeg = blockIdx.y * rows_per, rend = min(a.rows, rbeg + rows_per);
  unsigned short* dlist = (unsigned short*)(row_off + a.rows + 1) + (size_t)wave * 64 * 64;   // [64 words x 64 bits]
  for (int r = rbeg + wave; r < rend; r += 4) {
    const double cos_t = a.cos_t[r], sin_t = a.sin_t[r];
    int base = row_off[r];
    for (int w0 = 0; w0 < a.words; w0 += 64) {
      const int wd = w0 + lane;
      u64 bits = wd < a.words ? a.tgt_bits[((long long)b * a.rows + r) * a.words + wd] : 0ull;
      const int pc = __popcll(bits);
      const int incl = wave_incl_scan_i32(pc);
      const int n = __builtin_amdgcn_readlane(incl, 63);
      int off = incl - pc;
      while (bits) {
        dlist[off++] = (unsigned short)(wd * 64 + __ffsll((long long)bits) - 1);
        bits &= bits - 1;
      }
      c19_wave_sync();
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
      c19_wave_sync();
      base += n;
    }
  }
}

// a row kernel over the chunk: a wavefront per row, the sweep on gridDim.y
void c19_rows_launch(cfear_ctx* ctx, const C19Args& c, void (*fn)(const C19Args), int per_wave, const char* name) {
  ProfScope ps(ctx, name);
  C19Args k = c;
  k.per_wave = per_wave;
  const int waves = c19_waves(per_wave);
  hipLaunchKernelGGL(fn, dim3((c.rows + waves - 1) / waves, c.batch), dim3(64 * waves), (size_t)per_wave * waves, ctx->stream, k);
}

}  // namespace

int c19_check_input(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc, const cfear_cen2019_params* par) {
  if (!polar || !desc || !par) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: null argument");
  if (desc->rows <= 0 || desc->cols <= 0 || desc->stride < desc->cols || desc->batch <= 0 ||
      (desc->batch > 1 && desc->batch_stride < (int64_t)desc->rows * desc->stride))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: bad polar descriptor");
  if (desc->cols < 2 || desc->cols > kC19MaxCols)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: cols must be in [2, %d]", kC19MaxCols);
  if ((long long)desc->rows * desc->cols > kC19MaxPixels)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: rows * cols > 2^22 unsupported (the fp64 sum of the sweep must be exact)");
  if (desc->rows > kC19MaxRows) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: rows > %d unsupported", kC19MaxRows);
  if (par->max_points < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: max_points < 0");
  if (par->min_range_bins < 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: min_range_bins < 0");
  if (!std::isfinite(par->range_res)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: range_res must be finite");
  return CFEAR_OK;
}

int c19_launch_stats(cfear_ctx* ctx, const C19Args& c) {
  c19_rows_launch(ctx, c, cen2019_range_kernel, c.rowb_bytes, "cen2019_range");
  {
    ProfScope ps(ctx, "cen2019_image");
    hipLaunchKernelGGL(cen2019_image_kernel, dim3(c.batch), dim3(256), 0, ctx->stream, c, 0);
  }
  c19_rows_launch(ctx, c, cen2019_hsum_kernel, c.rowb_bytes, "cen2019_hsum");
  {
    ProfScope ps(ctx, "cen2019_image");
    hipLaunchKernelGGL(cen2019_image_kernel, dim3(c.batch), dim3(256), 0, ctx->stream, c, 1);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

void c19_launch_select(cfear_ctx* ctx, const C19Args& c, C19Select* d_sel, int* d_hist) {
  ProfScope ps(ctx, "cen2019_select");
  const int slices = std::max(1, std::min((c.rows + 3) / 4, 2048 / c.batch));
  hipLaunchKernelGGL(cen2019_select_init_kernel, dim3(c.batch), dim3(256), 0, ctx->stream, c, d_sel, d_hist);
  for (int pass = kC19Passes - 1; pass >= 0; pass--) {
    hipLaunchKernelGGL(cen2019_hist_kernel, dim3(c.batch, slices), dim3(256), 0, ctx->stream, c, d_sel, d_hist, pass * kC19Digit);
    hipLaunchKernelGGL(cen2019_pick_kernel, dim3(c.batch), dim3(256), 0, ctx->stream, c, d_sel, d_hist, pass * kC19Digit);
  }
}

int c19_launch_detect(cfear_ctx* ctx, const C19Args& c, C19Select* d_sel, int* d_hist) {
  const int lds_fresh = (c19_fresh_lds(c.cols, c.words, c.rowb_bytes) + 15) & ~15;
  const int lds_mark = (c19_mark_lds(c.words, c.rowb_bytes) + 15) & ~15;
  const int lds_emit = (c.words + 1) * 4 * 8;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)cen2019_fresh_kernel, (size_t)lds_fresh * c19_waves(lds_fresh)));
  c19_rows_launch(ctx, c, cen2019_fresh_kernel, lds_fresh, "cen2019_fresh");
  CFEAR_HIP_CHECK(ctx, hipGetLastError());                   // the kernels below trust what the fresh kernel leaves in the scratch
  c19_launch_select(ctx, c, d_sel, d_hist);
  c19_rows_launch(ctx, c, cen2019_mark_kernel, lds_mark, "cen2019_mark");
  c19_rows_launch(ctx, c, cen2019_emit_kernel, lds_emit, "cen2019_emit");
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

extern "C" void cfear_cen2019_params_default(cfear_cen2019_params* par) {
  if (!par) return;
  par->max_points = 1000;         // Utils.h:46
  par->min_range_bins = 0;
  par->range_res = 0.04328;       // ScanType.h:62
}

extern "C" int cfear_filter_cen2019(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                    const cfear_cen2019_params* par, float* xyzi, int32_t* n_points, int32_t cap_points,
                                    int32_t* targets, uint8_t* region_mask, float* image_stats, int32_t* counts) {
  if (!polar || !desc || !par || !xyzi || !n_points || cap_points <= 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: null argument");
  CFEAR_CHECK(c19_check_input(ctx, polar, desc, par));
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, cols = desc->cols, batch = desc->batch;
  const int words = (cols + 63) / 64;
  const size_t img_bytes = (size_t)rows * desc->stride, pixels = (size_t)rows * cols;
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(batch, kC19MaxGridY),
                                                             std::min(kC19ChunkBytes / img_bytes, kC19KeyBytes / (pixels * 8))));

  HostStage st(ctx, kWsFilter);
  C19Args a{};
  const cfear_polar_desc dd = st.images(a.polar, polar, *desc);
  int32_t* d_np;
  st.out(a.xyzi, xyzi, (size_t)batch * cap_points * 16);
  st.out(d_np, n_points, (size_t)batch * 4);
  if (targets) st.out(a.targets, targets, (size_t)batch * cap_points * 8);
  if (region_mask) st.out(a.region_mask, region_mask, (size_t)batch * pixels);
  if (image_stats) st.out(a.image_stats, image_stats, (size_t)batch * 16);
  if (counts) st.out(a.counts, counts, (size_t)batch * 12);
  st.piece(a.row_maxg, (size_t)chunk * rows * 4);
  st.piece(a.row_sum, (size_t)chunk * rows * 8);
  st.piece(a.img, (size_t)chunk * 16);
  st.piece(a.keys, (size_t)chunk * pixels * 8);
  st.piece(a.row_cnt, (size_t)chunk * rows * 16);
  st.piece(a.row_minkey, (size_t)chunk * rows * 8);
  st.piece(a.cut, (size_t)chunk * 8);
  C19Select* d_sel;
  int* d_hist;
  st.piece(d_sel, (size_t)chunk * sizeof(C19Select));
  st.piece(d_hist, (size_t)chunk * kC19Bins * 4);
  st.piece(a.mark_bits, (size_t)chunk * rows * words * 8);
  st.piece(a.hpos_bits, (size_t)chunk * rows * words * 8);
  st.piece(a.tgt_bits, (size_t)chunk * rows * words * 8);
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: the image and the outputs must be all host or all device");
  CFEAR_CHECK(st.carve());
  double *d_cos = nullptr, *d_sin = nullptr;
  CFEAR_CHECK(cfear_trig_tables(ctx, rows, &d_cos, &d_sin));

  a.rows = rows; a.cols = cols; a.stride = dd.stride;
  a.batch_stride = batch > 1 ? dd.batch_stride : (long long)img_bytes;
  a.max_points = par->max_points; a.min_range_bins = par->min_range_bins;
  a.words = words; a.rowb_bytes = (cols + 15) & ~15;
  a.cos_t = d_cos; a.sin_t = d_sin; a.range_res = par->range_res; a.cap_points = cap_points;
  const size_t cloud_lds = (size_t)(rows + 1) * 4 + kC19CloudLists;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)cen2019_cloud_kernel, cloud_lds));

  const C19Args base = a;
  for (int b0 = 0; b0 < batch; b0 += chunk) {
    C19Args c = base;
    c.batch = std::min(chunk, batch - b0);
    c.polar = base.polar + (long long)b0 * base.batch_stride;
    c.xyzi = base.xyzi + (size_t)b0 * cap_points * 4;
    c.n_points = d_np + b0;
    if (base.targets) c.targets = base.targets + (size_t)b0 * cap_points * 2;
    if (base.region_mask) c.region_mask = base.region_mask + (size_t)b0 * pixels;
    if (base.image_stats) c.image_stats = base.image_stats + (size_t)b0 * 4;
    if (base.counts) c.counts = base.counts + (size_t)b0 * 3;
    CFEAR_CHECK(c19_launch_stats(ctx, c));
    CFEAR_CHECK(c19_launch_detect(ctx, c, d_sel, d_hist));
    {
      ProfScope ps(ctx, "cen2019_cloud");
      hipLaunchKernelGGL(cen2019_cloud_kernel, dim3(c.batch, kC19CloudSplit), dim3(256), cloud_lds, ctx->stream, c);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  std::vector<int32_t> n_host((size_t)batch);
  st.fetch(n_host.data(), d_np, (size_t)batch * 4);
  CFEAR_CHECK(st.finish());
  for (int b = 0; b < batch; b++)
    if (n_host[b] > cap_points)
      return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "cen2019: image %d: %d targets > cap_points %d", b, n_host[b], cap_points);
  return CFEAR_OK;
}
