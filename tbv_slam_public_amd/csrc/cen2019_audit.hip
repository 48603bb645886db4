// cen2019_audit.hip -- which Cen2019 landmarks of a sweep hang on the order among equal h in cen2019features' unstable
// std::sort (Utils.cpp:524; DESIGN.md sections 3 and 4.20).  tests/cen2019_audit_cpu.py is the definition.
//
// The order-free form of the detector (cen2019.hip) uses keys through comparisons only, so it holds for every total order
// that refines "descending h".  With T = rows - 1, a `run` a maximal stretch of bins with s < 0 and the TOUCHERS of a run
// [u, v] its own candidates, the candidate at v + 1 and the one at u - 1 if u - 1 < T:
//   sure(c)       in every run c touches, c alone attains the largest h among the touchers
//   possible(c)   in every run c touches, h(c) is the largest h among the touchers
//   sure <= fresh(order) <= possible, so every order's cut K has h_lo <= h(K) <= h_hi: the h of the max_points-th largest
//   sure candidate and of the max_points-th largest possible one.  P_in = {h > h_hi} is processed under every order and
//   P_out = {h >= h_lo} holds every order's processed set; the marking rule is monotone in the processed set, which gives
//   R_in <= R(order) <= R_out.  A target of R_in whose run is the same maximal run in R_out is emitted under every order.
// Kernels, per chunk of sweeps, after cen2019.hip's own chain has run twice (ties ascending: this library's result; ties
// descending: the witness):
//   cen2019_audit_fresh_kernel   a wavefront per row: the segmented maximum of cen2019_fresh_kernel under BOTH tie directions
//                                (two runtop tables: the winners differ iff the largest h is attained twice), the sure and
//                                possible flags, and the two key sets compacted into the two halves of the selection buffer
//   cen2019_select (cen2019.hip) once per key set: h_hi and h_lo are the h bits of the two results
//   cen2019_audit_band_kernel    a wavefront per row: the candidates with h_lo <= h <= h_hi
//   cen2019_audit_level_kernel   a workgroup per sweep: the band's size, the single-candidate rule, the two thresholds
//   cen2019_audit_mark_kernel    a wavefront per row, once for R_in and once for R_out: cen2019_mark_kernel's rule on an h
//                                level, with the two straddle rules
//   cen2019_audit_certify_kernel a wavefront per row: the runs of R_in an unmarked bin ends, adjacency in R_in, the run's ends
//                                in R_out -> certain-target bitmap; the row's popcounts and the optional marks bytes
//   cen2019_audit_out_kernel     a workgroup per sweep: the record, and targets / certain in (row, bin) order
#include <cmath>

#include "cen2019_dev.hpp"

namespace {

typedef c19_u64 u64;

// the per-row counters of q.arow (kRowCols apart), and behind them the sums the out kernel takes from the other row tables
enum { kRowBand = 0, kRowStraddle, kRowMarksIn, kRowMarks, kRowMarksOut, kRowCertain, kRowTargetsRev, kRowTargetsChanged,
       kRowMarksChanged, kRowUsed, kSumSure = kRowUsed, kSumPossible, kSumCandidates, kSumFresh, kSums, kRowCols = 12 };

struct C19Level {
  u64 in_from, out_from;             // a candidate is in P_in / P_out iff its c19_ord(h) >= this (2^32: none, 0: all)
  float h_hi, h_lo;
  int n_band, pad;
};

struct C19Audit {
  u64* keys_sure;                    // [batch][rows][cols]: the second half of the selection buffer (the possible keys: a.keys)
  int32_t* cnt_possible;             // [batch][rows][4]: [1] = the row's possible candidates (the layout the select reads)
  int32_t* cnt_sure;
  u64* cut_possible;                 // [batch]: the select's results
  u64* cut_sure;
  C19Level* level;                   // [batch]
  int32_t* arow;                     // [batch][rows][kRowCols]
  int32_t* row_off;                  // [batch][rows]: the row's first target in the sweep's list
  const int32_t* fwd_cnt;            // [batch][rows][4], [batch][rows][words]: the detector's scratch of the two orders
  const u64 *fwd_marks, *rev_marks, *fwd_tgt, *rev_tgt, *hpos;
  u64 *in_bits, *out_bits, *cert_bits;   // [batch][rows][words]
  cfear_cen2019_order_record* records;   // outputs
  int32_t* n_targets;                // [batch]
  int32_t* targets;
  uint8_t* certain;
  uint8_t* marks;
  int cap_points;
};

// the cut of a select as a threshold on c19_ord(h): ~0 -> max_points == 0, nothing is processed; 0 -> fewer than max_points
// keys, everything is (no candidate has ord 0: that is a NaN)
__device__ __forceinline__ u64 c19a_from(u64 cut) { return cut == ~0ull ? (1ull << 32) : (cut >> 22); }
__device__ __forceinline__ float c19a_level(u64 cut) {
  return cut == ~0ull ? __builtin_inff() : cut == 0ull ? -__builtin_inff() : c19_unord((uint32_t)(cut >> 22));
}

// LDS of a wavefront: as cen2019_fresh_kernel's, with a second runtop table
__host__ __device__ inline int c19a_fresh_lds(int cols, int words, int rowb_bytes) {
  return c19_fresh_lds(cols, words, rowb_bytes) + ((cols * 2 + 15) & ~15);
}

__global__ __launch_bounds__(256) void cen2019_audit_fresh_kernel(const C19Args a, const C19Audit q) {
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
  unsigned short* top_f = (unsigned short*)(bound + 64);      // the best toucher of the run that ends at v, ties ascending
  unsigned short* top_r = top_f + (((cols * 2 + 15) & ~15) >> 1);   // ... ties descending
  const long long row = (long long)b * a.rows + r;
  const uint32_t flat0 = (uint32_t)r * (uint32_t)cols;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  const float mean = a.img[b * 4], inv = a.img[b * 4 + 1], mean_h = a.img[b * 4 + 2];
  const auto ord_of = [&](int j) {
    float s, h;
    c19_sh(rowb, j, cols, mean, inv, s, h);
    return c19_ord(h);
  };
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
  }
  if (lane == 0) neg[words] = 0ull;
  c19_wave_sync();
  c19_zero_tables(neg, words, prevz, nextz, lane);
  c19_run_tops(neg, cand, prevz, tail, bound, top_f, cols, words, T, flat0, kC19FlatMask, lane,
               [&](int j) { return c19_key(ord_of(j), flat0 + j, kC19FlatMask); });
  c19_run_tops(neg, cand, prevz, tail, bound, top_r, cols, words, T, flat0, 0u, lane,
               [&](int j) { return c19_key(ord_of(j), flat0 + j, 0u); });

  u64* seg_p = a.keys + row * cols;
  u64* seg_s = q.keys_sure + row * cols;
  int n_poss = 0, n_sure = 0;
  for (int j0 = 0; j0 < words * 64; j0 += 64) {
    const int j = j0 + lane;
    bool poss = false, sure = false;
    uint32_t ord = 0;
    if (j < cols && c19_bit(cand, j)) {
      ord = ord_of(j);
      poss = sure = true;
      const auto touch = [&](int v) {                          // the run that ends at v: j is one of its touchers
        const int tf = top_f[v];
        poss = poss && ord_of(tf) == ord;                      // h(j) is the largest h among them
        sure = sure && tf == j && top_r[v] == j;               // and whichever way ties go, j wins: nobody else attains it
      };
      if (c19_bit(neg, j)) {
        touch(c19_run_end(neg, nextz, j));
      } else {
        if (j >= 1 && c19_bit(neg, j - 1)) touch(j - 1);
        if (j < T && j + 1 < cols && c19_bit(neg, j + 1)) touch(c19_run_end(neg, nextz, j + 1));
      }
    }
    const u64 bp = __ballot(poss), bs = __ballot(sure);
    const u64 below = (1ull << lane) - 1ull;
    const u64 key = c19_key(ord, flat0 + j, kC19FlatMask);
    if (poss) seg_p[n_poss + __popcll(bp & below)] = key;
    if (sure) seg_s[n_sure + __popcll(bs & below)] = key;
    n_poss += __popcll(bp);
    n_sure += __popcll(bs);
  }
  if (lane == 0) {
    q.cnt_possible[row * 4 + 1] = n_poss;
    q.cnt_sure[row * 4 + 1] = n_sure;
  }
}

// the candidates whose processing the order decides: h_lo <= h <= h_hi (none when h_hi is -inf or +inf)
__global__ __launch_bounds__(256) void cen2019_audit_band_kernel(const C19Args a, const C19Audit q) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;
  const int b = blockIdx.y, cols = a.cols;
  uint8_t* rowb = smem + (size_t)wave * a.per_wave;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  const float mean = a.img[b * 4], inv = a.img[b * 4 + 1], mean_h = a.img[b * 4 + 2];
  const u64 cut_p = q.cut_possible[b];
  const bool binding = cut_p != ~0ull && cut_p != 0ull;
  const u64 upto = cut_p >> 22, from = c19a_from(q.cut_sure[b]);
  int n = 0;
  for (int j = lane; j < cols; j += 64) {
    float s, h;
    c19_sh(rowb, j, cols, mean, inv, s, h);
    const u64 o = c19_ord(h);
    n += binding && h > mean_h && o >= from && o <= upto;
  }
  n = wave_sum_i32(n);
  if (lane == 0) q.arow[((long long)b * a.rows + r) * kRowCols + kRowBand] = n;
}

__global__ __launch_bounds__(256) void cen2019_audit_level_kernel(const C19Args a, const C19Audit q) {
  __shared__ int sh[4];
  const int b = blockIdx.x, t = threadIdx.x;
  int n = 0;
  for (int r = t; r < a.rows; r += 256) n += q.arow[((long long)b * a.rows + r) * kRowCols + kRowBand];
  n = wave_sum_i32(n);
  if ((t & 63) == 0) sh[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    n = sh[0] + sh[1] + sh[2] + sh[3];
    const u64 cut_p = q.cut_possible[b], cut_s = q.cut_sure[b];
    const bool binding = cut_p != ~0ull && cut_p != 0ull;
    const bool flat = a.img[b * 4 + 3] == 0.f;
    C19Level lv;
    lv.out_from = c19a_from(cut_s);
    // h > h_hi; a band of one candidate is every order's K and is processed under each: h >= h_hi
    lv.in_from = !binding ? c19a_from(cut_p) : (cut_p >> 22) + (n == 1 ? 0ull : 1ull);
    lv.n_band = n == 1 ? 0 : n;
    lv.h_hi = flat ? __builtin_nanf("") : c19a_level(cut_p);
    lv.h_lo = flat ? __builtin_nanf("") : c19a_level(cut_s);
    lv.pad = 0;
    q.level[b] = lv;
  }
}

// cen2019_mark_kernel's rule on the h level of P_in (outer == 0) or P_out (outer == 1).  A run's own rule: "an own candidate is
// processed and a top-h own candidate sits at r < T" (R_out), "... and none at r >= T" (R_in); the processed set is an h level,
// so the top-h own candidates are processed as soon as one own candidate is.  Only the run that straddles column T can have
// them on both sides.  LDS of a wavefront: c19a_mark_lds.
__host__ __device__ inline int c19a_mark_lds(int words, int rowb_bytes) { return rowb_bytes + (3 * words + 1) * 8 + 2 * (words + 1) * 4 + 8; }

__global__ __launch_bounds__(256) void cen2019_audit_mark_kernel(const C19Args a, const C19Audit q, int outer) {
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
  const long long row = (long long)b * a.rows + r;
  const uint32_t flat0 = (uint32_t)r * (uint32_t)cols;
  c19_stage_row(a.polar + (long long)b * a.batch_stride + (long long)r * a.stride, cols, rowb, lane);
  c19_wave_sync();
  const float mean = a.img[b * 4], inv = a.img[b * 4 + 1], mean_h = a.img[b * 4 + 2];
  const u64 from = outer ? q.level[b].out_from : q.level[b].in_from;
  for (int j0 = 0; j0 < words * 64; j0 += 64) {
    const int j = j0 + lane;
    bool ng = false, pr = false;
    if (j < cols) {
      float s, h;
      c19_sh(rowb, j, cols, mean, inv, s, h);
      ng = s < 0.f;
      pr = h > mean_h && (u64)c19_ord(h) >= from;
    }
    const u64 bn = __ballot(ng), bp = __ballot(pr);
    if (lane == 0) {
      neg[j0 >> 6] = bn;
      proc[j0 >> 6] = bp;
      marks[j0 >> 6] = bp & ~bn;
    }
  }
  if (lane == 0) neg[words] = 0ull;
  c19_wave_sync();
  c19_zero_tables(neg, words, prevz, nextz, lane);
  c19_wave_sync();

  // ---- the run that holds columns T - 1 and T (wave-uniform): on which sides of T its top-h processed own candidates sit ---------
  int su = -1;
  bool s_lo = false, s_hi = false;
  if (T >= 1 && T < cols && c19_bit(neg, T - 1) && c19_bit(neg, T)) {
    su = c19_run_start(neg, prevz, T);
    const int sv = c19_run_end(neg, nextz, T);
    u64 best_f = 0ull, best_r = 0ull;                           // the first and the last bin that attain the largest h
    for (int j = su + lane; j <= sv; j += 64)
      if (c19_bit(proc, j)) {
        float s, h;
        c19_sh(rowb, j, cols, mean, inv, s, h);
        const uint32_t o = c19_ord(h);
        const u64 kf = c19_key(o, flat0 + j, kC19FlatMask), kr = c19_key(o, flat0 + j, 0u);
        best_f = kf > best_f ? kf : best_f;
        best_r = kr > best_r ? kr : best_r;
      }
    best_f = c19_wave_max_u64(best_f);
    best_r = c19_wave_max_u64(best_r);
    if (best_f) {
      s_lo = (int)(c19_key_flat(best_f, kC19FlatMask) - flat0) < T;
      s_hi = (int)(c19_key_flat(best_r, 0u) - flat0) >= T;
    }
  }

  for (int w = lane; w < words; w += 64) {
    u64 ends = c19_run_ends(neg, w);
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
          const bool lo = u == su ? s_lo : v < T, hi = u == su ? s_hi : u >= T;
          M = (outer ? lo : (lo && !hi)) ? v : top;
        }
      }
      if (M >= 0) c19_set_range(marks, u, M);
    }
  }
  c19_wave_sync();
  u64* dst = (outer ? q.out_bits : q.in_bits) + row * words;
  int n = 0;
  for (int w = lane; w < words; w += 64) {
    dst[w] = marks[w];
    n += __popcll(marks[w]);
  }
  n = wave_sum_i32(n);
  if (lane == 0) {
    q.arow[row * kRowCols + (outer ? kRowMarksOut : kRowMarksIn)] = n;
    if (outer) q.arow[row * kRowCols + kRowStraddle] = s_lo && s_hi;
  }
}

// As cen2019_emit_kernel on R_in, with the row's R_out for the run's ends.  LDS of a wavefront: own (R_in, bins below min_range
// cleared), adj (R_in of the two neighbour rows), outb (R_out), hpos, cbits: u64 [words + 1] each
__global__ __launch_bounds__(256) void cen2019_audit_certify_kernel(const C19Args a, const C19Audit q) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * (blockDim.x >> 6) + wave;
  if (r >= a.rows) return;
  const int b = blockIdx.y, cols = a.cols, words = a.words;
  u64* own = (u64*)(smem + (size_t)wave * a.per_wave);
  u64* adj = own + words + 1;
  u64* outb = adj + words + 1;
  u64* hpos = outb + words + 1;
  u64* cbits = hpos + words + 1;
  const long long img_row0 = (long long)b * a.rows, row = img_row0 + r;
  const int below = r - 1 < 0 ? a.rows - 1 : r - 1, above = r + 1 >= a.rows ? 0 : r + 1;
  int cnt[4] = {0, 0, 0, 0};                                   // marks, marks changed, targets reversed, targets changed
  for (int w = lane; w <= words; w += 64) {
    u64 o = 0ull, ad = 0ull, ob = 0ull, hp = 0ull;
    if (w < words) {
      o = q.in_bits[row * words + w];
      ad = q.in_bits[(img_row0 + below) * words + w] | q.in_bits[(img_row0 + above) * words + w];
      ob = q.out_bits[row * words + w];
      hp = q.hpos[row * words + w];
      const int lo = a.min_range_bins - w * 64;                // bins below min_range are not looked at (Utils.cpp:559)
      if (lo >= 64) o = 0ull;
      else if (lo > 0) o &= ~((1ull << lo) - 1ull);
      const u64 mf = q.fwd_marks[row * words + w], mr = q.rev_marks[row * words + w];
      const u64 tf = q.fwd_tgt[row * words + w], tr = q.rev_tgt[row * words + w];
      cnt[0] += __popcll(mf);
      cnt[1] += __popcll(mf ^ mr);
      cnt[2] += __popcll(tr);
      cnt[3] += __popcll(tf ^ tr);
    }
    own[w] = o; adj[w] = ad; outb[w] = ob; hpos[w] = hp; cbits[w] = 0ull;
  }
  c19_wave_sync();
  for (int w = lane; w < words; w += 64) {
    const u64 word = own[w];
    u64 ends = c19_run_ends(own, w);
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
      const int end = w * 64 + e;                              // end + 1 < cols
      if (c19_highest(adj, start, end) < 0) continue;          // checkAdjacentMarked: it holds in every order, R_in is the least
      if (c19_bit(outb, end + 1)) continue;                    // some order may run on beyond end ...
      if (start > a.min_range_bins && c19_bit(outb, start - 1)) continue;   // ... or begin before start
      const int hi = c19_highest(hpos, start, end);            // getMaxInRegion depends on h > 0 alone
      const int tgt = hi >= 0 ? hi : start;
      atomicOr(&cbits[tgt >> 6], 1ull << (tgt & 63));
    }
  }
  c19_wave_sync();
  int n_cert = 0;
  for (int w = lane; w < words; w += 64) {
    q.cert_bits[row * words + w] = cbits[w];
    n_cert += __popcll(cbits[w]);
  }
  n_cert = wave_sum_i32(n_cert);
  for (int c = 0; c < 4; c++) cnt[c] = wave_sum_i32(cnt[c]);
  if (lane == 0) {
    int32_t* ar = q.arow + row * kRowCols;
    ar[kRowMarks] = cnt[0];
    ar[kRowMarksChanged] = cnt[1];
    ar[kRowTargetsRev] = cnt[2];
    ar[kRowTargetsChanged] = cnt[3];
    ar[kRowCertain] = n_cert;
  }
  if (q.marks) {
    uint8_t* mrow = q.marks + row * cols;
    const u64 *in = q.in_bits + row * words, *mf = q.fwd_marks + row * words, *mr = q.rev_marks + row * words;
    for (int j = lane; j < cols; j += 64)
      mrow[j] = (uint8_t)((int)c19_bit(in, j) | ((int)c19_bit(mf, j) << 1) | ((int)c19_bit(outb, j) << 2) | ((int)c19_bit(mr, j) << 3));
  }
}

// the sweep's record; its targets in (row, bin) order, as cen2019_cloud_kernel leaves them, and which of them are certain
__global__ __launch_bounds__(256) void cen2019_audit_out_kernel(const C19Args a, const C19Audit q) {
  __shared__ int32_t wave_tot[4];
  __shared__ int32_t run_base;
  __shared__ int32_t sh[kSums][4];
  const int b = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t* row_off = q.row_off + (long long)b * a.rows;
  if (threadIdx.x == 0) run_base = 0;
  __syncthreads();
  int sum[kSums];
  for (int c = 0; c < kSums; c++) sum[c] = 0;
  for (int r0 = 0; r0 < a.rows; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const long long row = (long long)b * a.rows + r;
    const int v = r < a.rows ? q.fwd_cnt[row * 4 + 3] : 0;
    if (r < a.rows) {
      for (int c = 0; c < kRowUsed; c++) sum[c] += q.arow[row * kRowCols + c];
      sum[kSumSure] += q.cnt_sure[row * 4 + 1];
      sum[kSumPossible] += q.cnt_possible[row * 4 + 1];
      sum[kSumCandidates] += q.fwd_cnt[row * 4];
      sum[kSumFresh] += q.fwd_cnt[row * 4 + 1];
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
  for (int c = 0; c < kSums; c++) {
    const int s = wave_sum_i32(sum[c]);
    if (lane == 0) sh[c][wave] = s;
  }
  __syncthreads();                                             // also: row_off is visible to the workgroup
  if (threadIdx.x == 0) {
    const auto tot = [&](int c) { return sh[c][0] + sh[c][1] + sh[c][2] + sh[c][3]; };
    const C19Level lv = q.level[b];
    cfear_cen2019_order_record rec;
    rec.n_candidates = tot(kSumCandidates);
    rec.n_fresh = tot(kSumFresh);
    rec.n_sure_fresh = tot(kSumSure);
    rec.n_possibly_fresh = tot(kSumPossible);
    rec.n_band = lv.n_band;
    rec.n_rows_straddle_tied = tot(kRowStraddle);
    rec.n_marks_in = tot(kRowMarksIn);
    rec.n_marks = tot(kRowMarks);
    rec.n_marks_out = tot(kRowMarksOut);
    rec.n_targets = run_base;
    rec.n_targets_certain = tot(kRowCertain);
    rec.n_targets_reversed = tot(kRowTargetsRev);
    rec.n_targets_changed_reversed = tot(kRowTargetsChanged);
    rec.n_marks_changed_reversed = tot(kRowMarksChanged);
    rec.h_hi = lv.h_hi;
    rec.h_lo = lv.h_lo;
    q.records[b] = rec;
    q.n_targets[b] = run_base;
  }
  if (!q.targets && !q.certain) return;
  for (int r = wave; r < a.rows; r += 4) {
    const long long row = (long long)b * a.rows + r;
    int base = row_off[r];
    for (int w0 = 0; w0 < a.words; w0 += 64) {
      const int wd = w0 + lane;
      u64 bits = wd < a.words ? q.fwd_tgt[row * a.words + wd] : 0ull;
      const u64 cert = wd < a.words ? q.cert_bits[row * a.words + wd] : 0ull;
      const int pc = __popcll(bits);
      const int incl = wave_incl_scan_i32(pc);
      const int n = __builtin_amdgcn_readlane(incl, 63);
      long long idx = base + incl - pc;
      while (bits) {
        const int e = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        if (idx < q.cap_points) {
          if (q.targets) {
            q.targets[((long long)b * q.cap_points + idx) * 2] = r;
            q.targets[((long long)b * q.cap_points + idx) * 2 + 1] = wd * 64 + e;
          }
          if (q.certain) q.certain[(long long)b * q.cap_points + idx] = (uint8_t)((cert >> e) & 1ull);
        }
        idx++;
      }
      base += n;
    }
  }
}

void c19a_rows_launch(cfear_ctx* ctx, const C19Args& c, const C19Audit& q, void (*fn)(const C19Args, const C19Audit), int per_wave,
                      const char* name) {
  ProfScope ps(ctx, name);
  C19Args k = c;
  k.per_wave = per_wave;
  const int waves = c19_waves(per_wave);
  hipLaunchKernelGGL(fn, dim3((c.rows + waves - 1) / waves, c.batch), dim3(64 * waves), (size_t)per_wave * waves, ctx->stream, k, q);
}

}  // namespace

extern "C" int cfear_cen2019_order_audit(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                         const cfear_cen2019_params* par, cfear_cen2019_order_record* records, int32_t* targets,
                                         uint8_t* certain, int32_t cap_points, uint8_t* marks) {
  static_assert(sizeof(cfear_cen2019_order_record) == 64, "cfear_cen2019_order_record is 64 bytes");
  if (!polar || !desc || !par || !records || cap_points < 0 || ((targets || certain) && cap_points <= 0))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: null argument");
  CFEAR_CHECK(c19_check_input(ctx, polar, desc, par));
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, cols = desc->cols, batch = desc->batch;
  const int words = (cols + 63) / 64;
  const size_t img_bytes = (size_t)rows * desc->stride, pixels = (size_t)rows * cols;
  // the selection buffer holds two key sets here
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min(batch, kC19MaxGridY),
                                                             std::min(kC19ChunkBytes / img_bytes, kC19KeyBytes / (pixels * 16))));

  HostStage st(ctx, kWsFilter);
  C19Args a{};
  C19Audit q{};
  const cfear_polar_desc dd = st.images(a.polar, polar, *desc);
  st.out(q.records, records, (size_t)batch * sizeof(cfear_cen2019_order_record));
  if (targets) st.out(q.targets, targets, (size_t)batch * cap_points * 8);
  if (certain) st.out(q.certain, certain, (size_t)batch * cap_points);
  if (marks) st.out(q.marks, marks, (size_t)batch * pixels);
  int32_t* d_nt;
  st.piece(d_nt, (size_t)batch * 4);
  const size_t bitmap = (size_t)chunk * rows * words * 8, cnt4 = (size_t)chunk * rows * 16;
  u64 *fwd_marks, *rev_marks, *fwd_tgt, *rev_tgt, *rev_cut;
  int32_t *fwd_cnt, *rev_cnt;
  st.piece(a.row_maxg, (size_t)chunk * rows * 4);
  st.piece(a.row_sum, (size_t)chunk * rows * 8);
  st.piece(a.img, (size_t)chunk * 16);
  st.piece(a.keys, (size_t)chunk * pixels * 8);
  st.piece(q.keys_sure, (size_t)chunk * pixels * 8);
  st.piece(fwd_cnt, cnt4);
  st.piece(rev_cnt, cnt4);
  st.piece(q.cnt_possible, cnt4);
  st.piece(q.cnt_sure, cnt4);
  st.piece(a.row_minkey, (size_t)chunk * rows * 8);
  st.piece(a.cut, (size_t)chunk * 8);
  st.piece(rev_cut, (size_t)chunk * 8);
  st.piece(q.cut_possible, (size_t)chunk * 8);
  st.piece(q.cut_sure, (size_t)chunk * 8);
  C19Select* d_sel;
  int* d_hist;
  st.piece(d_sel, (size_t)chunk * sizeof(C19Select));
  st.piece(d_hist, (size_t)chunk * kC19Bins * 4);
  st.piece(fwd_marks, bitmap);
  st.piece(rev_marks, bitmap);
  st.piece(a.hpos_bits, bitmap);
  st.piece(fwd_tgt, bitmap);
  st.piece(rev_tgt, bitmap);
  st.piece(q.in_bits, bitmap);
  st.piece(q.out_bits, bitmap);
  st.piece(q.cert_bits, bitmap);
  st.piece(q.level, (size_t)chunk * sizeof(C19Level));
  st.piece(q.arow, (size_t)chunk * rows * kRowCols * 4);
  st.piece(q.row_off, (size_t)chunk * rows * 4);
  if (st.mixed()) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cen2019: the image and the outputs must be all host or all device");
  CFEAR_CHECK(st.carve());

  a.rows = rows; a.cols = cols; a.stride = dd.stride;
  a.batch_stride = batch > 1 ? dd.batch_stride : (long long)img_bytes;
  a.max_points = par->max_points; a.min_range_bins = par->min_range_bins;
  a.words = words; a.rowb_bytes = (cols + 15) & ~15;
  q.cap_points = cap_points;
  q.fwd_cnt = fwd_cnt;
  q.fwd_marks = fwd_marks; q.rev_marks = rev_marks; q.fwd_tgt = fwd_tgt; q.rev_tgt = rev_tgt; q.hpos = a.hpos_bits;
  const int lds_fresh = (c19a_fresh_lds(cols, words, a.rowb_bytes) + 15) & ~15;
  const int lds_mark = (c19a_mark_lds(words, a.rowb_bytes) + 15) & ~15;
  const int lds_cert = (words + 1) * 5 * 8;
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)cen2019_audit_fresh_kernel, (size_t)lds_fresh * c19_waves(lds_fresh)));
  CFEAR_CHECK(cfear_allow_lds(ctx, (const void*)cen2019_audit_mark_kernel, (size_t)lds_mark * c19_waves(lds_mark)));

  for (int b0 = 0; b0 < batch; b0 += chunk) {
    C19Args c = a;
    c.batch = std::min(chunk, batch - b0);
    c.polar = a.polar + (long long)b0 * a.batch_stride;
    C19Audit k = q;
    k.records = q.records + b0;
    k.n_targets = d_nt + b0;
    if (q.targets) k.targets = q.targets + (size_t)b0 * cap_points * 2;
    if (q.certain) k.certain = q.certain + (size_t)b0 * cap_points;
    if (q.marks) k.marks = q.marks + (size_t)b0 * pixels;
    CFEAR_CHECK(c19_launch_stats(ctx, c));
    C19Args fwd = c, rev = c;                                  // this library's order, then the witness; the keys are the select's only
    fwd.row_cnt = fwd_cnt; fwd.mark_bits = fwd_marks; fwd.tgt_bits = fwd_tgt;
    rev.row_cnt = rev_cnt; rev.mark_bits = rev_marks; rev.tgt_bits = rev_tgt; rev.cut = rev_cut; rev.tie_rev = 1;
    CFEAR_CHECK(c19_launch_detect(ctx, fwd, d_sel, d_hist));
    CFEAR_CHECK(c19_launch_detect(ctx, rev, d_sel, d_hist));
    c19a_rows_launch(ctx, c, k, cen2019_audit_fresh_kernel, lds_fresh, "cen2019_audit_fresh");
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    C19Args sp = c, ss = c;                                    // the two cut levels
    sp.row_cnt = q.cnt_possible; sp.cut = q.cut_possible;
    ss.row_cnt = q.cnt_sure; ss.cut = q.cut_sure; ss.keys = q.keys_sure;
    c19_launch_select(ctx, sp, d_sel, d_hist);
    c19_launch_select(ctx, ss, d_sel, d_hist);
    c19a_rows_launch(ctx, c, k, cen2019_audit_band_kernel, c.rowb_bytes, "cen2019_audit_band");
    {
      ProfScope ps(ctx, "cen2019_audit_level");
      hipLaunchKernelGGL(cen2019_audit_level_kernel, dim3(c.batch), dim3(256), 0, ctx->stream, c, k);
    }
    for (int outer = 0; outer < 2; outer++) {
      ProfScope ps(ctx, "cen2019_audit_mark");
      C19Args m = c;
      m.per_wave = lds_mark;
      const int waves = c19_waves(lds_mark);
      hipLaunchKernelGGL(cen2019_audit_mark_kernel, dim3((rows + waves - 1) / waves, c.batch), dim3(64 * waves), (size_t)lds_mark * waves,
                         ctx->stream, m, k, outer);
    }
    c19a_rows_launch(ctx, c, k, cen2019_audit_certify_kernel, lds_cert, "cen2019_audit_certify");
    {
      ProfScope ps(ctx, "cen2019_audit_out");
      hipLaunchKernelGGL(cen2019_audit_out_kernel, dim3(c.batch), dim3(256), 0, ctx->stream, c, k);
    }
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  std::vector<int32_t> n_host((size_t)batch);
  st.fetch(n_host.data(), d_nt, (size_t)batch * 4);
  CFEAR_CHECK(st.finish());
  if (targets || certain)
    for (int b = 0; b < batch; b++)
      if (n_host[b] > cap_points)
        return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "cen2019: image %d: %d targets > cap_points %d (the records are complete)", b,
                               n_host[b], cap_points);
  return CFEAR_OK;
}
