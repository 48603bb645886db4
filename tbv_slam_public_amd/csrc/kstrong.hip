// kstrong.hip -- the k-strongest filter of the polar radar image (stage F of the CFEAR hot path): StructuredKStrongest::
// FilterKstrongest, AxialNonMaxSupress and getPeaksFilteredPointCloud (cfear_radarodometry/src/cfear_radarodometry/
// radar_filters.cpp:209-337).  The row sweep (kstrong_row, kstrongest_rows_kernel), the decode family for
// [range bins][azimuths] sources (kstrong_extract / _select / _image_kernel, kstrongest_cols_kernel), the cloud
// kernel, one selection per family (kstrong_select, kstrong_cols_select) with the device entries that launch from it, and the
// entry points cfear_kstrong_plan, cfear_filter_kstrongest and cfear_filter_kstrongest_rowkeys.
#include <cmath>

#include "polar_common.hpp"

namespace {

struct KStrongArgs {
  const uint8_t* polar;
  int rows, cols, stride, batch;
  long long batch_stride;
  int k, u_zmin, want_peaks, batch0;
  int32_t* sel_range;
  uint8_t* sel_intensity;
  int32_t* sel_count;
  uint8_t* is_peak;
  int32_t* row_valid;      // [batch][rows][2]: kept bins beyond min_range_bin (all, peaks) -> cloud offsets
  int min_range_bin;
  int dense_halo;          // 1: the image is a padded copy of a DENSE cv::Mat (the pipeline's rotated buffer): bins read
                           // past a row end are the first bins of the next row, not the padding
  // Fused cloud output (the batched odometry pipeline, k <= 64): the kept bins beyond min_range_bin of row r as packed
  // keys (intensity << 24 | range bin) at row_keys[(b * rows + r) * k + j], j < row_valid[..][0], in the reference's
  // order (ascending (intensity, range), radar_filters.cpp:309-337): 4 bytes per point instead of a PointXYZI; the
  // surface-point kernel compacts the rows and converts to Cartesian (surface.hip).
  uint32_t* row_keys;
  const long long* image_offsets;   // optional [batch]: byte offset of image b from `polar` instead of b * batch_stride
};

// bit 7 of every byte of the result is set iff that byte of x is >= t (0 <= t <= 255).
// Per byte (0x80 + low7) - (t & 0x7f) stays in [1, 0xff]: no borrow crosses a byte boundary.
__device__ __forceinline__ uint32_t swar_ge(uint32_t x, uint32_t tl4, bool thi) {
  const uint32_t g = ((x & 0x7f7f7f7fu) | 0x80808080u) - tl4;
  const uint32_t xh = x & 0x80808080u;
  return thi ? (xh & g) : ((g & 0x80808080u) | xh);
}

// Reads the row into registers: lane L of chunk c owns bytes [(c*64+L)*16, +16).  Lanes whose chunk
// lies entirely past the row end hold zeros and issue no loads.
// tail_safe: the 16 bytes of the row's LAST, partial piece may be read whole (they end inside the image:
// cfear_piece_inside_image, row_pieces.hpp) -- the bytes beyond the row are then cleared in registers.  Without it the piece is gathered byte by byte:
// sixteen dependent predicated loads on one lane that the whole wavefront waits for (Oxford's native 3768 bins end 8 bytes into
// a piece: 0.220 instead of 0.159 ms per 512 sweeps until round 6).
template <int NCHUNK, bool VEC>
__device__ __forceinline__ void load_row(const uint8_t* rowp, int cols, int lane, uint32_t (&w)[NCHUNK * 4], const bool tail_safe = false) {
#pragma unroll
  for (int c = 0; c < NCHUNK; c++) {
    const int pos = (c * 64 + lane) * 16;
    w[c * 4 + 0] = w[c * 4 + 1] = w[c * 4 + 2] = w[c * 4 + 3] = 0u;
    if (VEC && (pos + 16 <= cols || (tail_safe && pos < cols))) {
      const u32x4 v = __builtin_nontemporal_load((const u32x4*)(rowp + pos));
      w[c * 4 + 0] = v.x; w[c * 4 + 1] = v.y; w[c * 4 + 2] = v.z; w[c * 4 + 3] = v.w;
      if (pos + 16 > cols) {                       // the ragged tail: keep the row's own bytes only
#pragma unroll
        for (int d = 0; d < 4; d++) {
          const int rem = cols - (pos + 4 * d);
          w[c * 4 + d] &= rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
        }
      }
    } else if (pos < cols) {                       // unaligned image or the partial tail chunk of an image's last row
#pragma unroll
      for (int d = 0; d < 4; d++) {
        uint32_t word = 0;
#pragma unroll
        for (int by = 0; by < 4; by++) {
          const int p = pos + d * 4 + by;
          if (p < cols) word |= (uint32_t)rowp[p] << (8 * by);
        }
        w[c * 4 + d] = word;
      }
    }
  }
}

// Candidate bitmaps.  For each 16-byte chunk c of this lane, bit (8*by + 4 + d) of bm[c] is set iff
// byte `by` of word d is >= t.  The SWAR compare leaves its verdict in bit 7 of every byte; a
// v_bfi per word shifts the running bitmap down one bit and inserts the new verdicts, so the
// bitmap costs nothing over the masks themselves (5 VALU per 4 bins).
template <int NCHUNK, bool MASK, bool THI>
__device__ __forceinline__ void candidate_bitmaps(const uint32_t (&w)[NCHUNK * 4], uint32_t tl4, int cols, int lane,
                                                  uint32_t (&bm)[NCHUNK]) {
  constexpr uint32_t M = 0x80808080u;
#pragma unroll
  for (int c = 0; c < NCHUNK; c++) {
    uint32_t acc = 0;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t x = w[c * 4 + d];
      const uint32_t g = ((x & 0x7f7f7f7fu) | M) - tl4;   // per byte in [1, 0xff]: no borrow crosses bytes
      uint32_t raw = THI ? (g & x) : (g | x);              // bit 7 of each byte: byte >= t
      if (MASK) {                                          // byte validity (row tail / z_min == 0)
        const int rem = cols - ((c * 64 + lane) * 16 + d * 4);
        raw &= rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
      }
      acc = (raw & M) | ((acc >> 1) & ~M);
    }
    bm[c] = acc;
  }
}

// Calls f(pos) for every candidate bin of this lane.  Two chunks share one loop (their bitmaps
// occupy disjoint nibbles), so a row of <= 2048 bins costs one divergent loop, 4096 bins two.
template <int NCHUNK, typename F>
__device__ __forceinline__ void for_each_candidate(const uint32_t (&bm)[NCHUNK], int lane, F&& f) {
#pragma unroll
  for (int c = 0; c < NCHUNK; c += 2) {
    uint32_t mm = (bm[c] >> 4) | (c + 1 < NCHUNK ? bm[c + 1] : 0u);
    const int base = c * 1024 + lane * 16;
    while (mm) {
      const int t = __ffs(mm) - 1;
      mm &= mm - 1;
      f(base + ((t & 4) << 8) + ((t & 3) << 2) + (t >> 3));
    }
  }
}

// One azimuth row on one wavefront.  STAGED = false: the row is read from `rowp` (global memory) and staged in `rowbuf`;
// STAGED = true: the caller has already placed the row's bytes in `rowbuf` (LDS, 16-byte aligned, readable up to the next
// multiple of 16 bins; kstrongest_cols_kernel transposes them there) -- no peaks in that mode (no halo bytes).
// hist: [kScratch / 4] dwords of scratch, list: [kpad] packed keys; nothing below crosses a workgroup barrier.
template <int NCHUNK, bool VEC, bool MASK, bool STAGED>
__device__ __forceinline__ void kstrong_row(const KStrongArgs& a, const int r, const int b, const uint8_t* img, uint8_t* rowbuf,
                                            uint32_t* hist, uint32_t* list, const int lane) {
  const long long row_lin = (long long)r * a.stride;
  const uint8_t* rowp = img + row_lin;
  const int k = a.k;
  constexpr int NP = (NCHUNK + 1) / 2;             // bitmap words per lane (two chunks per word)

  // Peaks only: the six bytes before and after the row (AxialNonMaxSupress reads them through unchecked cv::Mat::at,
  // radar_filters.cpp:238-298).  Their loads are issued here, together with the row's, so that they cost no extra
  // memory round trip later.
  const bool do_peaks = !STAGED && a.want_peaks && a.is_peak;
  uint8_t halo = 0;
  int halo_pos = 0;                                // rowbuf offset this lane's halo byte belongs to (0 = none)
  if (do_peaks && (lane < 6 || (lane >= 8 && lane < 14))) {
    const long long total = (long long)a.rows * a.stride;
    long long lin;
    if (lane < 6) {
      halo_pos = -6 + lane;
      lin = row_lin - 6 + lane;
      if (a.dense_halo) lin = r > 0 ? row_lin - a.stride + a.cols - 6 + lane : -1;       // last bins of the previous row
    } else {
      halo_pos = a.cols + (lane - 8);
      lin = row_lin + halo_pos;
      if (a.dense_halo) lin = r + 1 < a.rows ? row_lin + a.stride + (lane - 8) : total;   // first bins of the next row
    }
    if (lin >= 0 && lin < total) halo = img[lin];
  }
  const int cols16 = (a.cols + 15) & ~15;          // STAGED: the bytes of rowbuf that may be read
  uint32_t w[NCHUNK * 4];
  if (STAGED) {
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if ((c * 64 + lane) * 16 < cols16) v = *(const uint4*)(rowbuf + (c * 64 + lane) * 16);
      w[c * 4] = v.x; w[c * 4 + 1] = v.y; w[c * 4 + 2] = v.z; w[c * 4 + 3] = v.w;
    }
  } else {
    load_row<NCHUNK, VEC>(rowp, a.cols, lane, w, cfear_piece_inside_image(r, a.cols & ~15, a.rows, a.stride));
#pragma unroll
    for (int c = 0; c < NCHUNK; c++)                 // stage the row: candidate bytes are fetched by position
      *(uint4*)(rowbuf + (c * 64 + lane) * 16) = make_uint4(w[c * 4], w[c * 4 + 1], w[c * 4 + 2], w[c * 4 + 3]);
  }

  // The row lives on in LDS: the (rare) later passes over it re-read it from there instead of keeping 4 NCHUNK
  // registers alive across the whole kernel (occupancy: 8 wavefronts per SIMD need <= 64 VGPRs).
  // Each re-read stands behind a compiler barrier: the row does not change, so without one the compiler lifts the reads
  // -- and the masked copies of every word that the byte compares start from -- out of the loop that re-tests the row,
  // and holds the whole unrolled compaction's words at once: 48 registers more than 7 wavefronts per SIMD leave, which went
  // to scratch memory (and a kernel that declares any is dispatched with a private segment on every wavefront).
  auto reload_chunk = [&](const int c, uint32_t (&x)[4]) {
    asm volatile("" ::: "memory");
    uint4 v = make_uint4(0, 0, 0, 0);
    if (!STAGED || (c * 64 + lane) * 16 < cols16) v = *(const uint4*)(rowbuf + (c * 64 + lane) * 16);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  };
  auto reload_row = [&](uint32_t (&x)[NCHUNK * 4]) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (!STAGED || (c * 64 + lane) * 16 < cols16) v = *(const uint4*)(rowbuf + (c * 64 + lane) * 16);
      x[c * 4] = v.x; x[c * 4 + 1] = v.y; x[c * 4 + 2] = v.z; x[c * 4 + 3] = v.w;
    }
  };
  // ---- candidates: bins with intensity >= uchar(z_min) (radar_filters.cpp:217) ---------------------
  uint32_t bm[NCHUNK];
  {
    const uint32_t tz4 = (uint32_t)(a.u_zmin & 0x7f) * 0x01010101u;
    if (a.u_zmin & 0x80) candidate_bitmaps<NCHUNK, MASK, true>(w, tz4, a.cols, lane, bm);
    else candidate_bitmaps<NCHUNK, MASK, false>(w, tz4, a.cols, lane, bm);
  }
  int c_lane = 0;
#pragma unroll
  for (int c = 0; c < NCHUNK; c++) c_lane += __popc(bm[c]);
  const int c_incl = wave_incl_scan_i32(c_lane);
  const int n_ge = __builtin_amdgcn_readlane(c_incl, 63);
  int n_sel;                                       // survivors = min(candidates, k)
  int n_all;                                       // keys placed in list[] (== n_sel unless the cut is made by rank)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // One candidate per lane and round, however the candidates cluster (a wall return fills adjacent bins of ONE
  // lane).  Candidates are numbered lane-major ("slots"); owner lanes mark the first slot of their run, a max-scan
  // spreads the owner id over the run, and in round rd lane j takes slot 64 rd + j: it selects bit (slot - first
  // slot) of its owner's bitmap by popcount bisection.  n <= 256 candidates -> at most 4 rounds, no divergent loop.
  uint8_t* marker = (uint8_t*)hist;                // [256] owner lane of the slot that starts a run, else 0
  uint32_t* sexcl = hist + 64;                     // [64] first slot of each lane's run
  uint32_t* spw = hist + 128;                      // [NP][64] bitmaps
  auto scatter_prepare = [&](const uint32_t (&bmx)[NCHUNK], int cnt_lane, int cnt_incl) {
    uint32_t pw[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) pw[p] = (bmx[2 * p] >> 4) | (2 * p + 1 < NCHUNK ? bmx[2 * p + 1] : 0u);
    const int excl = cnt_incl - cnt_lane;
    ((uint32_t*)marker)[lane] = 0;
    sexcl[lane] = excl;
#pragma unroll
    for (int p = 0; p < NP; p++) spw[p * 64 + lane] = pw[p];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (cnt_lane && excl < 256) marker[excl] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  int scatter_carry = 0;                           // owner of the last slot of the previous round
  auto scatter_round = [&](int rd, int n, bool& valid) -> uint32_t {
    const int slot = rd * 64 + lane;
    const int own = max(scatter_carry, wave_incl_scan_max_i32((int)marker[slot]));
    scatter_carry = __builtin_amdgcn_readlane(own, 63);
    valid = slot < n;
    uint32_t key = 0;
    if (valid) {
      int q = slot - (int)sexcl[own];
      uint32_t word = spw[own];
      int p = 0;
#pragma unroll
      for (int pp = 1; pp < NP; pp++) {
        const int c = __popc(word);
        const uint32_t nxt = spw[pp * 64 + own];
        if (p == pp - 1 && q >= c) { q -= c; word = nxt; p = pp; }
      }
      int t = 0;
      { const int c = __popc(word & 0xFFFFu); if (q >= c) { q -= c; t = 16; word >>= 16; } }
      { const int c = __popc(word & 0xFFu);   if (q >= c) { q -= c; t += 8; word >>= 8; } }
      { const int c = __popc(word & 0xFu);    if (q >= c) { q -= c; t += 4; word >>= 4; } }
      { const int c = __popc(word & 0x3u);    if (q >= c) { q -= c; t += 2; word >>= 2; } }
      if (q >= (int)(word & 1u)) t += 1;
      const int pos = p * 2048 + own * 16 + ((t & 4) << 8) + ((t & 3) << 2) + (t >> 3);
      key = ((uint32_t)rowbuf[pos] << 24) | (uint32_t)pos;
    }
    return key;
  };
  auto scatter_to_lanes = [&](const uint32_t (&bmx)[NCHUNK], int cnt_lane, int cnt_incl, int n) {   // n <= 64
    scatter_prepare(bmx, cnt_lane, cnt_incl);
    scatter_carry = 0;
    bool valid;
    const uint32_t key = scatter_round(0, n, valid);
    if (valid) list[lane] = key;
  };
  // The cut intensity T of the k largest among the histogrammed keys: lane L owns intensities 4 (63 - L) + {0..3},
  // an inclusive scan over lanes counts from 255 downward.
  auto cut_from_hist = [&](int& T, int& n_gt, int& n_eq) {
    const uint4 h = *(const uint4*)(hist + (63 - lane) * 4);
    const int s_lane = (int)(h.x + h.y + h.z + h.w);
    const int s_incl = wave_incl_scan_i32(s_lane);
    const unsigned long long reach = __ballot(s_incl >= k);
    const int lc = __ffsll((long long)reach) - 1;                  // first lane whose cumulative count reaches k
    int Tl = 0, gl = 0, el = 0;
    {
      int cum = s_incl - s_lane;
      const int hv[4] = {(int)h.w, (int)h.z, (int)h.y, (int)h.x};  // descending intensity
      bool found = false;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!found && cum + hv[j] >= k) { Tl = 4 * (63 - lane) + 3 - j; gl = cum; el = hv[j]; found = true; }
        cum += hv[j];
      }
    }
    T = __builtin_amdgcn_readlane(Tl, lc);
    n_gt = __builtin_amdgcn_readlane(gl, lc);
    n_eq = __builtin_amdgcn_readlane(el, lc);
  };

  if (__builtin_expect(n_ge <= k || n_ge <= 64, 1)) {
    // ---- at most k candidates, or at most 64: all of them become keys (any order); the ranking below
    //      restores the reference's ascending (intensity, range) order and, when there are more than k,
    //      keeps the k largest keys -- the lexicographic (intensity, range) cut of the reference, ties at
    //      the cut intensity resolved toward the larger range, without building the histogram --------------
    n_sel = min(n_ge, k);
    n_all = n_ge;
    if (__builtin_expect(n_ge <= 64, 1)) {
      scatter_to_lanes(bm, c_lane, c_incl, n_ge);
    } else {
      int slot = c_incl - c_lane;
      for_each_candidate<NCHUNK>(bm, lane, [&](int pos) { list[slot++] = ((uint32_t)rowbuf[pos] << 24) | (uint32_t)pos; });
    }
  } else {
    // ---- more than k and more than 64 candidates: the cut intensity T -------------------------------------------
    n_sel = k;
    n_all = k;
    int T = 0, n_gt = 0, n_eq = 0;
    bool have_list = false;                        // list[] already holds every bin >= T (n_all of them, <= 64)
    // (a) very dense rows (> 256 candidates): raise the candidate threshold until between k and 256 bins pass it --
    //     each trial is one SWAR pass over the register-resident row (5 VALU per 4 bins); the first trial assumes
    //     a flat intensity distribution above the threshold, later ones bisect.  If two neighbouring thresholds
    //     bracket k the cut is known exactly (a plateau) and goes to the tie scan below.
    //     Invariant: c_lo = #(>= lo) >= k > c_hi = #(>= hi), so on exit without a trial in [k, 256] the cut is T = lo with
    //     c_lo >= k > c_hi.  A trial is tested for "< k" FIRST: k may exceed 256 (kMaxK = 1024), and a count in (256, k) is
    //     below the cut, not above it (every row with k > 256 ends here, exactly).
    // The bitmaps of the trial that lands in [k, 256] go straight into the scatter tables in LDS (scatter_prepare): kept in
    // registers until the loop's end they were part of what went to scratch memory.
    int n_c = n_ge;
    bool exact = false, prepared = false;
    if (n_ge > 256) {
      int lo = a.u_zmin, c_lo = n_ge, hi = 256, c_hi = 0;
      bool first = true;
      while (hi - lo > 1) {
        int mid = first ? 256 - max(1, ((256 - lo) * 128) / c_lo) : (lo + hi) >> 1;
        mid = min(max(mid, lo + 1), hi - 1);
        first = false;
        const uint32_t tm4 = (uint32_t)(mid & 0x7f) * 0x01010101u;
        uint32_t bx[NCHUNK];
        {
          uint32_t wx[NCHUNK * 4];
          reload_row(wx);
          if (mid & 0x80) candidate_bitmaps<NCHUNK, false, true>(wx, tm4, a.cols, lane, bx);
          else candidate_bitmaps<NCHUNK, false, false>(wx, tm4, a.cols, lane, bx);
          // mid > z_min: a bin that passes the trial passes z_min too, so the candidates' bitmap carries the byte validity
          // (one AND per chunk; the sixteen validity masks, hoisted out of this loop, were the MASK forms' scratch memory)
          if (MASK) {
#pragma unroll
            for (int c = 0; c < NCHUNK; c++) bx[c] &= bm[c];
          }
        }
        int x_lane = 0;
#pragma unroll
        for (int c = 0; c < NCHUNK; c++) x_lane += __popc(bx[c]);
        const int x_incl = wave_incl_scan_i32(x_lane);
        const int cnt = __builtin_amdgcn_readlane(x_incl, 63);
        if (cnt < k) { hi = mid; c_hi = cnt; }
        else if (cnt > 256) { lo = mid; c_lo = cnt; }
        else {
          scatter_prepare(bx, x_lane, x_incl);
          n_c = cnt; prepared = true;
          break;
        }
      }
      if (n_c > 256) { exact = true; T = lo; n_gt = c_hi; n_eq = c_lo - c_hi; }
    }
    if (!exact) {
      // (b) 64 < n_c <= 256 candidates: one key per lane and round (registers), an LDS histogram of the keys'
      //     intensities -> T; the keys >= T (the survivors plus the ties at the cut, <= 64 unless a plateau is
      //     wider) are packed into list[] by ballot and cut by rank below -- the reference's tie rule.
      if (!prepared) scatter_prepare(bm, c_lane, c_incl);
      scatter_carry = 0;
      uint32_t kr[4];
      bool kv[4];
      const int rounds = (n_c + 63) >> 6;
#pragma unroll
      for (int rd = 0; rd < 4; rd++) { kr[rd] = 0; kv[rd] = false; if (rd < rounds) kr[rd] = scatter_round(rd, n_c, kv[rd]); }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      *(uint4*)(hist + lane * 4) = make_uint4(0, 0, 0, 0);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int rd = 0; rd < 4; rd++) if (kv[rd]) atomicAdd(&hist[kr[rd] >> 24], 1u);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      cut_from_hist(T, n_gt, n_eq);
      if (n_gt + n_eq <= 64) {
        int base = 0;
#pragma unroll
        for (int rd = 0; rd < 4; rd++) {
          const bool sel = kv[rd] && (int)(kr[rd] >> 24) >= T;
          const unsigned long long bal = __ballot(sel);
          if (sel) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = kr[rd];
          base += __popcll(bal);
        }
        n_all = n_gt + n_eq;
        have_list = true;
      }
    }
    if (!have_list) {
    const int skip_eq = n_eq - (k - n_gt);         // drop the lowest-range ties: lexicographic (intensity, range)
    // ---- ordered compaction: all (> T) plus the (== T) bins of rank >= skip_eq in position order -----
    // (T >= z_min, so ">= T" implies candidacy; only the MASK variant needs the validity bits)
    const int thr_gt = T + 1;
    const uint32_t tg4 = (uint32_t)(thr_gt & 0x7f) * 0x01010101u;
    const bool tghi = (thr_gt & 0x80) != 0;
    const uint32_t te4 = (uint32_t)(T & 0x7f) * 0x01010101u;
    const bool tehi = (T & 0x80) != 0;
    int g_base = 0, e_base = 0;                    // survivors > T / bins == T before the current chunk
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) {
      uint32_t wt[4];                              // one chunk of the row at a time
      reload_chunk(c, wt);
      uint32_t mg[4], me[4];
      int cg = 0, ce = 0;
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const uint32_t valid = MASK ? ((bm[c] << (3 - d)) & 0x80808080u) : 0x80808080u;
        mg[d] = thr_gt > 255 ? 0u : (swar_ge(wt[d], tg4, tghi) & valid);
        me[d] = swar_ge(wt[d], te4, tehi) & valid & ~mg[d];
        cg += __popc(mg[d]);
        ce += __popc(me[d]);
      }
      const int packed = (ce << 16) | cg;          // one scan carries both prefixes (totals < 65536)
      const int incl = wave_incl_scan_i32(packed);
      const int tot = __builtin_amdgcn_readlane(incl, 63);
      const int excl = incl - packed;
      int g_run = g_base + (excl & 0xFFFF);
      int e_run = e_base + (excl >> 16);
      if (cg + ce) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
          uint32_t mm = mg[d] | me[d];
          while (mm) {
            const int bit = __ffs(mm) - 1;         // bit 7 of byte (bit >> 3)
            mm &= mm - 1;
            const int by = bit >> 3;
            const bool is_eq = (me[d] >> bit) & 1u;
            const bool selected = !is_eq || e_run >= skip_eq;
            const int e_sel_before = e_run > skip_eq ? e_run - skip_eq : 0;
            if (selected) {
              const int pos = (c * 64 + lane) * 16 + d * 4 + by;
              list[g_run + e_sel_before] = (((wt[d] >> (8 * by)) & 0xffu) << 24) | (uint32_t)pos;
            }
            if (is_eq) e_run++; else g_run++;
          }
        }
      }
      g_base += tot & 0xFFFF;
      e_base += tot >> 16;
    }
    }
  }
  const int nq = (n_all + 3) & ~3;
  for (int j = n_all + lane; j < nq; j += 64) list[j] = 0xFFFFFFFFu;      // pad for the b128 reads
  if (a.row_keys && lane < 2) hist[2 + lane] = 0;                       // ranks of the kept bins beyond min_range_bin
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int drop = n_all - n_sel;                  // keys below the cut (only when n_all <= 64)

  // ---- peaks (AxialNonMaxSupress, radar_filters.cpp:238-298): score[r] = sum of raw[r-3..r+3]
  //      exists for r within 3 bins of a kept bin m with 3 <= m < cols - 3; a kept bin is a peak iff its
  //      score is not exceeded by the three scores either side (missing scores are 0).  The reference reads
  //      raw[] through unchecked cv::Mat::at, i.e. up to 6 bytes before / after the row in image memory:
  //      those halo bytes are staged next to the row so that every tap is one LDS read. --------------------
  auto note_kept = [&](int m) {                    // kept VALID bins among the first / last 16 bins of the row
    if (m >= 3 && m < a.cols - 3) {
      if (m < 16) atomicOr(&hist[0], 1u << m);
      if (m >= a.cols - 16) atomicOr(&hist[1], 1u << (m - (a.cols - 16)));
    }
  };
  if (__builtin_expect(do_peaks, 0)) {
    if (halo_pos != 0) rowbuf[halo_pos] = halo;    // after the row staging: the tail chunk's zero padding lies there
    if (lane < 2) hist[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (drop == 0) {                               // every key survives: the kept set is known before ranking
      for (int j = lane; j < n_all; j += 64) note_kept((int)(list[j] & 0xFFFFFFu));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  // ---- rank the keys: ascending (intensity, range) == ascending packed key; survivors have rank >= drop ----
  const long long obase = ((long long)b * a.rows + r) * k;
  int nvalid = 0, nvalid_pk = 0;                   // wave-uniform (ballot popcounts)
  for (int j0 = 0; j0 < n_all; j0 += 64) {         // one pass unless k > 64
    const int j = j0 + lane;
    bool beyond = false, beyond_pk = false;
    uint32_t key = 0;
    int rank = -1;
    if (j < n_all) {
      key = list[j];
      rank = 0;
      for (int i = 0; i < nq; i += 4) {
        const uint4 q = *(const uint4*)(list + i);  // same address in every lane: LDS broadcast
        rank += (q.x < key) + (q.y < key) + (q.z < key) + (q.w < key);
      }
      rank -= drop;                                 // < 0: below the cut
    }
    const int range = (int)(key & 0xFFFFFFu);
    if (do_peaks && drop != 0) {                    // n_all <= 64: single pass, the kept set follows from the ranks
      if (rank >= 0) note_kept(range);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (rank >= 0) {
      if (a.sel_range) a.sel_range[obase + rank] = range;
      if (a.sel_intensity) a.sel_intensity[obase + rank] = (uint8_t)(key >> 24);
      beyond = range > a.min_range_bin;                             // radar_filters.cpp:327
      if (do_peaks) {
        int v[13];                                  // raw[range - 6 .. range + 6]
#pragma unroll
        for (int i = 0; i < 13; i++) v[i] = rowbuf[range - 6 + i];
        int sc[7];                                  // score[range - 3 .. range + 3]
        sc[0] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + v[6]);
#pragma unroll
        for (int i = 1; i < 7; i++) sc[i] = sc[i - 1] - v[i - 1] + v[i + 6];
        if (!(range >= 3 && range < a.cols - 3)) {
          // border bin: it created no scores itself; score[r] exists only if another kept valid bin lies
          // within 3 bins of r (all such bins are among the first / last 16 of the row)
          const uint32_t klo = hist[0], khi = hist[1];
          const int base = a.cols - 16;
#pragma unroll
          for (int i = 0; i < 7; i++) {
            const int rr = range - 3 + i;
            bool covered = false;
            {                                       // kept valid bins in [rr - 3, rr + 3] among bins 0..15
              const int lo = max(rr - 3, 0), hi = min(rr + 3, 15);
              if (hi >= lo) covered = ((klo >> lo) & ((2u << (hi - lo)) - 1u)) != 0u;
            }
            {                                       // ... among bins cols - 16 .. cols - 1
              const int lo = max(rr - 3 - base, 0), hi = min(rr + 3 - base, 15);
              if (hi >= lo) covered = covered || ((khi >> lo) & ((2u << (hi - lo)) - 1u)) != 0u;
            }
            if (!covered) sc[i] = 0;
          }
        }
        bool pk = true;
#pragma unroll
        for (int i = 1; i <= 3; i++)
          if (sc[3 - i] > sc[3] || sc[3] < sc[3 + i]) pk = false;
        a.is_peak[obase + rank] = pk ? 1 : 0;
        beyond_pk = beyond && pk;
      }
    }
    if (__builtin_expect(a.row_keys != nullptr, 1)) {
      // fused getPeaksFilteredPointCloud(cloud, false) (radar_filters.cpp:309-337): the row's kept bins in rank order;
      // a bin's slot = number of kept bins beyond min_range_bin with a lower rank (k <= 64: one pass)
      if (beyond) atomicOr(&hist[2 + (rank >> 5)], 1u << (rank & 31));
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (beyond) {
        const uint32_t m0 = hist[2], m1 = hist[3];
        const int idx = rank < 32 ? __popc(m0 & ((1u << rank) - 1u)) : __popc(m0) + __popc(m1 & ((1u << (rank - 32)) - 1u));
        a.row_keys[obase + idx] = key;
      }
    }
    nvalid += __popcll(__ballot(beyond));
    nvalid_pk += __popcll(__ballot(beyond_pk));
  }
  for (int j = n_sel + lane; j < k; j += 64) {     // unused slots
    if (a.sel_range) a.sel_range[obase + j] = -1;
    if (a.sel_intensity) a.sel_intensity[obase + j] = 0;
    if (do_peaks) a.is_peak[obase + j] = 0;
  }
  if (lane == 0) {
    if (a.row_valid) {
      a.row_valid[((long long)b * a.rows + r) * 2] = nvalid;
      a.row_valid[((long long)b * a.rows + r) * 2 + 1] = nvalid_pk;
    }
    if (a.sel_count) a.sel_count[(long long)b * a.rows + r] = n_sel;
  }
}

// per-wavefront LDS of a row: [raw row + 16-byte halos] (not STAGED) | scratch | list
__host__ __device__ constexpr int kstrong_scratch_bytes(int nchunk) { return ((nchunk + 1) / 2 + 2) * 256 > 1024 ? ((nchunk + 1) / 2 + 2) * 256 : 1024; }

// The sweep is issue-bound and feels where its code lands: CFEAR_KSTRONG_HEAD_PAD bytes (0 / 16 / 32 / 48) of s_nop at the kernel
// head move it through the four placements.  A change to kstrong_row is measured at all four (EXPERIMENTS.md) and the best
// one becomes the default here.
#ifndef CFEAR_KSTRONG_HEAD_PAD
#define CFEAR_KSTRONG_HEAD_PAD 0
#endif

template <int NCHUNK, bool VEC, bool MASK>
__global__ __launch_bounds__(256, 7) void kstrongest_rows_kernel(const KStrongArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if CFEAR_KSTRONG_HEAD_PAD > 0
  asm volatile(".rept %0\n\ts_nop 0\n\t.endr" ::"n"(CFEAR_KSTRONG_HEAD_PAD / 4));
#endif
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * kRowsPerBlock + wave;          // grid = (row quads, images): no division
  if (r >= a.rows) return;                                  // no workgroup barrier below
  const int b = a.batch0 + blockIdx.y;
  const uint8_t* img = a.polar + (a.image_offsets ? a.image_offsets[b] : (long long)b * a.batch_stride);
  const int kpad = max((a.k + 3) & ~3, 64);        // list capacity: k survivors, or up to 64 candidates to rank
  constexpr int kScratch = kstrong_scratch_bytes(NCHUNK);   // marker u8[256] | sexcl[64] | spw[NP][64], or hist[256]
  const int per_wave = NCHUNK * 1024 + 32 + kScratch + kpad * 4;
  uint8_t* rowbuf = smem + wave * per_wave + 16;                                  // the raw row, 16-byte halo either side
  uint32_t* hist = (uint32_t*)(smem + wave * per_wave + NCHUNK * 1024 + 32);      // [256] histogram / scatter scratch
  uint32_t* list = (uint32_t*)(smem + wave * per_wave + NCHUNK * 1024 + 32 + kScratch);   // [kpad] survivors (packed keys)
  kstrong_row<NCHUNK, VEC, MASK, false>(a, r, b, img, rowbuf, hist, list, lane);
}

// ---- two rows per wavefront ---------------------------------------------------------------------------------
// A radar azimuth holds two dozen bins >= z_min, so everything kstrong_row does after the byte compares -- the scan, the
// scatter, the ranking, the emission -- runs on a wavefront with a third of its lanes live, once per row.  Here wavefront w of
// a 128-thread workgroup owns rows 4 blockIdx.x + 2 w and + 1 from the load on: when the two rows hold at most 64 candidates
// TOGETHER (so each is on kstrong_row's "n_ge <= 64" branch) one scatter round, one ranking loop and one emission serve
// both.  (The rows are counted by a scan each, not by one packed scan: a first row beyond 64 alone ends the joint attempt before
// the second row's compares, which is what keeps dense scenes at the single-row kernel's time.)  Slots are numbered row 0 first; the owner id of a slot is (row << 6 | lane), which still grows with the
// slot, so the max-scan spreads it as before.  Row 0's keys go to list[0 ..), row 1's to list[kpad ..), and a lane ranks its
// key against its own row's segment: two addresses per LDS read instead of one.  Any other pair -- and the last row of an odd
// image -- takes kstrong_row<STAGED> on each row in turn (row 1 waits in its sixteen registers), so the results are the
// single-row kernel's bit for bit.
// Both rows stay in registers until their candidates' bytes have been fetched, and ONE row buffer in LDS holds them in turn
// (row 0, then row 1): a wavefront with two rows then needs no more LDS than one of the single-row kernel's, and as many
// wavefronts are resident as the registers allow -- with two buffers it was 3.5 per SIMD, and the sweep, which needs the other
// wavefronts' instructions to cover a wavefront's loads, ran 10 % SLOWER than one row per wavefront (EXPERIMENTS.md).
// Seven wavefronts per SIMD without scratch memory (six for the MASK forms): the Makefile binds the <4, ...> forms to that.
// VEC only, no peaks (no halo bytes are kept), NCHUNK <= 4: cfear_kstrong_device routes the rest to the table of 16.
// per-wavefront scratch: marker u8[256] | sexcl[2][64] | spw[2][NP][64] (never below what kstrong_row carves from it)
__host__ __device__ constexpr int kstrong_pair_scratch_bytes(int nchunk) { return (3 + 2 * ((nchunk + 1) / 2)) * 256; }
// per-wavefront LDS: one row, to the next multiple of 16 bins | scratch | two key lists
__host__ __device__ constexpr int kstrong_pair_wave_bytes(int nchunk, int cols, int kpad) {
  return ((cols + 15) & ~15) + kstrong_pair_scratch_bytes(nchunk) + 2 * kpad * 4;
}
constexpr int kPairRows = 2;                       // rows per wavefront; kRowsPerBlock / kPairRows wavefronts per workgroup

template <int NCHUNK, bool MASK>
__global__ __launch_bounds__(64 * kRowsPerBlock / kPairRows, MASK ? 6 : 7) void kstrongest_rowpairs_kernel(const KStrongArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if CFEAR_KSTRONG_HEAD_PAD > 0
  asm volatile(".rept %0\n\ts_nop 0\n\t.endr" ::"n"(CFEAR_KSTRONG_HEAD_PAD / 4));
#endif
  static_assert(kstrong_pair_scratch_bytes(NCHUNK) >= kstrong_scratch_bytes(NCHUNK), "kstrong_row's scratch fits the pair's");
  constexpr int NP = (NCHUNK + 1) / 2;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * kRowsPerBlock + kPairRows * wave;
  if (r0 >= a.rows) return;                                 // no workgroup barrier below
  const bool has1 = r0 + 1 < a.rows;                        // odd row counts: the last wavefront owns one row
  const int b = a.batch0 + blockIdx.y;
  const uint8_t* img = a.polar + (a.image_offsets ? a.image_offsets[b] : (long long)b * a.batch_stride);
  const int k = a.k;
  const int kpad = max((k + 3) & ~3, 64);
  const int cols16 = (a.cols + 15) & ~15;
  uint8_t* rowbuf = smem + wave * kstrong_pair_wave_bytes(NCHUNK, a.cols, kpad);           // [cols16]: row 0, later row 1
  uint32_t* hist = (uint32_t*)(rowbuf + cols16);
  uint32_t* list = (uint32_t*)(rowbuf + cols16 + kstrong_pair_scratch_bytes(NCHUNK));      // [2][kpad]

  // ---- load both rows before the first use (8 loads in flight at NCHUNK = 4), compare -----------------------------------
  uint32_t w0[NCHUNK * 4], w1[NCHUNK * 4];
  auto stage = [&](const uint32_t (&w)[NCHUNK * 4]) {       // the pieces kstrong_row<STAGED> and the byte fetch may read
#pragma unroll
    for (int c = 0; c < NCHUNK; c++)
      if ((c * 64 + lane) * 16 < cols16) *(uint4*)(rowbuf + (c * 64 + lane) * 16) = make_uint4(w[c * 4], w[c * 4 + 1], w[c * 4 + 2], w[c * 4 + 3]);
  };
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  uint32_t bm0[NCHUNK], bm1[NCHUNK];
  {
    const int r1 = has1 ? r0 + 1 : r0;                      // an absent row reads row 0 again and is not used
    load_row<NCHUNK, true>(img + (long long)r0 * a.stride, a.cols, lane, w0, cfear_piece_inside_image(r0, a.cols & ~15, a.rows, a.stride));
    load_row<NCHUNK, true>(img + (long long)r1 * a.stride, a.cols, lane, w1, cfear_piece_inside_image(r1, a.cols & ~15, a.rows, a.stride));
  }
  const uint32_t tz4 = (uint32_t)(a.u_zmin & 0x7f) * 0x01010101u;
  if (a.u_zmin & 0x80) candidate_bitmaps<NCHUNK, MASK, true>(w0, tz4, a.cols, lane, bm0);
  else candidate_bitmaps<NCHUNK, MASK, false>(w0, tz4, a.cols, lane, bm0);
  stage(w0);
  int c0 = 0, c1 = 0;
#pragma unroll
  for (int c = 0; c < NCHUNK; c++) c0 += __popc(bm0[c]);
  const int incl0 = wave_incl_scan_i32(c0);
  const int n0 = __builtin_amdgcn_readlane(incl0, 63);
  int n1 = 65, incl1 = 0;
  if (has1 && n0 <= 64) {                                   // a first row beyond 64 alone: the second row's compares are kstrong_row's
    if (a.u_zmin & 0x80) candidate_bitmaps<NCHUNK, MASK, true>(w1, tz4, a.cols, lane, bm1);
    else candidate_bitmaps<NCHUNK, MASK, false>(w1, tz4, a.cols, lane, bm1);
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) c1 += __popc(bm1[c]);
    incl1 = wave_incl_scan_i32(c1);
    n1 = __builtin_amdgcn_readlane(incl1, 63);
  } else {
#pragma unroll
    for (int c = 0; c < NCHUNK; c++) bm1[c] = 0;
  }
  const int e0 = incl0 - c0, e1 = n0 + incl1 - c1;

  if (__builtin_expect(!has1 || n0 + n1 > 64, 0)) {
    // ---- the rows one after the other, each from the row buffer: every path of kstrong_row, none of it written twice.
    //      (Two calls, not a loop of two turns: in a loop the compiler computes what kstrong_row derives from the lane id and
    //      the geometry before the loop and holds it across -- in scratch memory.)
    wave_sync();                                            // row 0 is staged
    kstrong_row<NCHUNK, true, MASK, true>(a, r0, b, img, rowbuf, hist, list, lane);
    if (!has1) return;
    wave_sync();                                            // the buffer, the scratch and the list are free again
    stage(w1);
    wave_sync();
    kstrong_row<NCHUNK, true, MASK, true>(a, r0 + 1, b, img, rowbuf, hist, list, lane);
    return;
  }

  // ---- slots: row 0's candidates lane-major, then row 1's; one candidate per lane ------------------------------------------
  uint8_t* marker = (uint8_t*)hist;                         // [256] (row << 6 | lane) of the slot that starts a run, else 0
  uint32_t* sexcl = hist + 64;                              // [2][64] first slot of each lane's run, by owner id
  uint32_t* spw = hist + 192;                               // [2][NP][64] bitmaps
  const int n = n0 + n1;
  {
    ((uint32_t*)marker)[lane] = 0;
    sexcl[lane] = e0;
    sexcl[64 + lane] = e1;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      spw[p * 64 + lane] = (bm0[2 * p] >> 4) | (2 * p + 1 < NCHUNK ? bm0[2 * p + 1] : 0u);
      spw[(NP + p) * 64 + lane] = (bm1[2 * p] >> 4) | (2 * p + 1 < NCHUNK ? bm1[2 * p + 1] : 0u);
    }
    list[lane] = 0xFFFFFFFFu;                               // the padding ranks above every key: both segments, up to the
    list[kpad + lane] = 0xFFFFFFFFu;                        // longer one's end (the ranking loop reads both that far)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (c0) marker[e0] = (uint8_t)lane;                     // e0 < n0, e1 < n <= 64
    if (c1) marker[e1] = (uint8_t)(64 + lane);
    wave_sync();
  }
  const bool valid = lane < n;
  const int row1 = lane >= n0 ? 1 : 0;                      // the row of this lane's slot
  uint32_t* seg = list + (row1 ? kpad : 0);                 // its row's keys
  uint32_t key = 0;
  {
    const int own = wave_incl_scan_max_i32((int)marker[lane]);
    int pos = 0;
    if (valid) {
      const int ol = own & 63;
      const uint32_t* sp = spw + (own >> 6) * (NP * 64) + ol;
      int q = lane - (int)sexcl[own];
      uint32_t word = sp[0];
      int p = 0;
#pragma unroll
      for (int pp = 1; pp < NP; pp++) {
        const int c = __popc(word);
        const uint32_t nxt = sp[pp * 64];
        if (p == pp - 1 && q >= c) { q -= c; word = nxt; p = pp; }
      }
      int t = 0;
      { const int c = __popc(word & 0xFFFFu); if (q >= c) { q -= c; t = 16; word >>= 16; } }
      { const int c = __popc(word & 0xFFu);   if (q >= c) { q -= c; t += 8; word >>= 8; } }
      { const int c = __popc(word & 0xFu);    if (q >= c) { q -= c; t += 4; word >>= 4; } }
      { const int c = __popc(word & 0x3u);    if (q >= c) { q -= c; t += 2; word >>= 2; } }
      if (q >= (int)(word & 1u)) t += 1;
      pos = p * 2048 + ol * 16 + ((t & 4) << 8) + ((t & 3) << 2) + (t >> 3);
    }
    // the candidates' bytes: row 0's from the buffer as it stands, then row 1 takes its place
    uint32_t byte = 0;
    if (valid && !row1) byte = rowbuf[pos];
    wave_sync();
    stage(w1);
    wave_sync();
    if (valid && row1) byte = rowbuf[pos];
    if (valid) {
      key = (byte << 24) | (uint32_t)pos;
      seg[lane - (row1 ? n0 : 0)] = key;
    }
  }
  wave_sync();                                              // the scatter tables have been read: their first words become
  if (a.row_keys && lane < 4) hist[lane] = 0;               // the rows' bitmaps of kept bins beyond min_range_bin
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- rank: ascending packed key within the lane's own row; survivors have rank >= drop ---------------------------------
  const int n_all = row1 ? n1 : n0;
  const int n_sel = min(n_all, k);
  const int nq = (max(n0, n1) + 3) & ~3;                    // wave-uniform, <= 64 <= kpad
  int rank = -1;
  if (valid) {
    rank = 0;
    for (int i = 0; i < nq; i += 4) {
      const uint4 q = *(const uint4*)(seg + i);             // two addresses per instruction
      rank += (q.x < key) + (q.y < key) + (q.z < key) + (q.w < key);
    }
    rank -= n_all - n_sel;                                  // < 0: below the cut
  }
  // ---- emit ----------------------------------------------------------------------------------------------------------------
  const long long obase = ((long long)b * a.rows + r0 + row1) * k;
  const int range = (int)(key & 0xFFFFFFu);
  bool beyond = false;
  if (rank >= 0) {
    if (a.sel_range) a.sel_range[obase + rank] = range;
    if (a.sel_intensity) a.sel_intensity[obase + rank] = (uint8_t)(key >> 24);
    beyond = range > a.min_range_bin;                       // radar_filters.cpp:327
  }
  if (__builtin_expect(a.row_keys != nullptr, 1)) {         // k <= 64: the ranks fit one pair of words per row
    uint32_t* bits = hist + 2 * row1;
    if (beyond) atomicOr(&bits[rank >> 5], 1u << (rank & 31));
    wave_sync();
    if (beyond) {
      const uint32_t m0 = bits[0], m1 = bits[1];
      const int idx = rank < 32 ? __popc(m0 & ((1u << rank) - 1u)) : __popc(m0) + __popc(m1 & ((1u << (rank - 32)) - 1u));
      a.row_keys[obase + idx] = key;
    }
  }
  const unsigned long long bal = __ballot(beyond);
  const unsigned long long lanes1 = n0 >= 64 ? 0ull : ~0ull << n0;      // the lanes that hold row 1's slots
  if (a.sel_range || a.sel_intensity) {                     // unused slots, both rows
#pragma nounroll
    for (int h = 0; h < kPairRows; h++) {
      const long long ob = ((long long)b * a.rows + r0 + h) * k;
      for (int j = min(h ? n1 : n0, k) + lane; j < k; j += 64) {
        if (a.sel_range) a.sel_range[ob + j] = -1;
        if (a.sel_intensity) a.sel_intensity[ob + j] = 0;
      }
    }
  }
  if (lane < kPairRows) {                                   // lane h reports row h
    const long long ro = (long long)b * a.rows + r0 + lane;
    if (a.row_valid) {
      a.row_valid[ro * 2] = __popcll(bal & (lane ? lanes1 : ~lanes1));
      a.row_valid[ro * 2 + 1] = 0;
    }
    if (a.sel_count) a.sel_count[ro] = min(lane ? n1 : n0, k);
  }
}

// ---- [range bins][azimuths] sources: the driver's decode fused into the sweep ---------------------------------------
// radarDriver::Callback (radar_driver.cpp:74-90) rotates such a sweep 90 degrees counter-clockwise before Process();
// rotate_ccw_rows_kernel + kstrongest_rows_kernel move the image through HBM three times (read, write, read).  The fused
// route reads it ONCE, along its own rows, and never builds the rotated image:
//   1. extraction   the source is streamed in 16-byte pieces (16 azimuths of one bin); a SWAR compare finds the bytes >=
//      uchar(z_min) -- the only bins FilterKstrongest can keep (radar_filters.cpp:217) -- and each is appended as a key
//      (intensity << 24 | bin) to the list of ITS azimuth (a radar sweep holds a few dozen per azimuth).
//   2. selection    one wavefront per azimuth (two when both lists are short): the k largest keys of the list ARE the
//      reference's selection (lexicographic (intensity, range) cut, ties toward the larger range), ranked into its order.
//      Batches that fill the chip run 1 + 2 in ONE kernel, a workgroup per image with the lists in LDS
//      (kstrong_image_kernel); smaller ones spread an image over many workgroups and keep the lists in global memory
//      (kstrong_extract_kernel: one returning atomic per candidate; kstrong_select_kernel).
//   3. kstrongest_cols_kernel   azimuths with more than kCandCap candidates (dense returns; z_min = 0) need the raw row:
//      pass 2 puts their 16-column tile on a work list, and this kernel transposes those tiles into LDS (v_perm_b32 on
//      4 x 4 byte blocks) and runs the complete row algorithm on them.  Without a list it takes every tile.
// a.rows / a.cols are the ROTATED image's (azimuths, bins); a.stride / a.batch_stride are the SOURCE's (bytes per bin
// row, per image).  Output row r holds source column a.rows - 1 - r (cv::ROTATE_90_COUNTERCLOCKWISE).
constexpr int kColsTile = 16;
constexpr int kColsWaves = 8;
constexpr int kCandCap = 256;                 // candidate keys kept per azimuth (1 KiB)
constexpr int kExtractPieces = 8;             // 16-byte pieces in flight per thread and step

// The candidates among kExtractPieces 16-byte pieces held in registers (w[u] = piece p0 + step * u of the image, pieces
// numbered along the source rows: piece p = bin p / segs, source columns 16 (p % segs) ..): emit(r, key) once per byte
// >= uchar(z_min), r = the azimuth row of the ROTATED image.  One candidate per lane and turn, whichever piece it sits in
// (a wall fills adjacent azimuths of ONE piece): a wavefront takes as many turns as its busiest lane holds candidates.
template <typename Emit>
__device__ __forceinline__ void extract_candidates(const KStrongArgs& a, const uint32_t (&w)[kExtractPieces][4], const uint32_t p0,
                                                   const uint32_t step, const uint32_t n_pieces, const uint32_t seg_magic,
                                                   const int segs, Emit&& emit) {
  const uint32_t tz4 = (uint32_t)(a.u_zmin & 0x7f) * 0x01010101u;
  const bool thi = (a.u_zmin & 0x80) != 0;
  uint32_t cm[kExtractPieces / 2];                           // bit 16 (u & 1) + 4 d + byte of word u / 2
#pragma unroll
  for (int h = 0; h < kExtractPieces / 2; h++) cm[h] = 0;
#pragma unroll
  for (int u = 0; u < kExtractPieces; u++) {
    // the SWAR verdicts sit in bit 7 of every byte; v_dot4_u32_u8 with the weights 1, 2, 4, .., 128 sums them into
    // 128 * (one bit per byte) -- two dwords per accumulator
    const uint32_t lo = __builtin_amdgcn_udot4(swar_ge(w[u][1], tz4, thi), 0x80402010u,
                                               __builtin_amdgcn_udot4(swar_ge(w[u][0], tz4, thi), 0x08040201u, 0u, false), false);
    const uint32_t hi = __builtin_amdgcn_udot4(swar_ge(w[u][3], tz4, thi), 0x80402010u,
                                               __builtin_amdgcn_udot4(swar_ge(w[u][2], tz4, thi), 0x08040201u, 0u, false), false);
    uint32_t pm = (lo >> 7) | ((hi >> 7) << 8);
    if (p0 + step * u >= n_pieces) pm = 0;
    cm[u >> 1] |= pm << (16 * (u & 1));
  }
  for (;;) {
    int t = -1;
#pragma unroll
    for (int h = kExtractPieces / 2 - 1; h >= 0; h--)
      if (cm[h]) t = 32 * h + __ffs(cm[h]) - 1;
    if (t < 0) break;
#pragma unroll
    for (int h = 0; h < kExtractPieces / 2; h++)
      if ((t >> 5) == h) cm[h] &= cm[h] - 1;
    const int u = t >> 4, e = t & 15;
    // w[u][e >> 2]: registers cannot be indexed by a lane -- the piece by a chain of selects, then the dword
    uint32_t x0 = 0, x1 = 0, x2 = 0, x3 = 0;
#pragma unroll
    for (int uu = 0; uu < kExtractPieces; uu++) {
      const bool is = u == uu;
      x0 = is ? w[uu][0] : x0; x1 = is ? w[uu][1] : x1; x2 = is ? w[uu][2] : x2; x3 = is ? w[uu][3] : x3;
    }
    const uint32_t word = (e & 8) ? ((e & 4) ? x3 : x2) : ((e & 4) ? x1 : x0);
    const uint32_t p = p0 + step * (uint32_t)u;
    const uint32_t j = segs == 1 ? p : __umulhi(p, seg_magic), sg = p - j * (uint32_t)segs;
    emit(a.rows - 1 - (int)(16u * sg + e), (((word >> (8 * (e & 3))) & 0xffu) << 24) | j);
  }
}

__device__ __forceinline__ void load_pieces(const KStrongArgs& a, const uint8_t* img, const uint32_t p0, const uint32_t step,
                                            const uint32_t n_pieces, const uint32_t seg_magic, const int segs,
                                            uint32_t (&w)[kExtractPieces][4]) {
  if (a.stride == 16 * segs) {                               // no row pitch: piece p is bytes 16 p .. of the image
#pragma unroll
    for (int u = 0; u < kExtractPieces; u++) {
      const uint32_t p = min(p0 + step * u, n_pieces - 1u);
      const u32x4 v = __builtin_nontemporal_load((const u32x4*)(img + (size_t)p * 16u));
      w[u][0] = v.x; w[u][1] = v.y; w[u][2] = v.z; w[u][3] = v.w;
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < kExtractPieces; u++) {
    const uint32_t p = min(p0 + step * u, n_pieces - 1u);
    const uint32_t j = segs == 1 ? p : __umulhi(p, seg_magic), sg = p - j * (uint32_t)segs;
    const u32x4 v = __builtin_nontemporal_load((const u32x4*)(img + (size_t)j * a.stride + 16u * sg));
    w[u][0] = v.x; w[u][1] = v.y; w[u][2] = v.z; w[u][3] = v.w;
  }
}

// The k strongest of one azimuth's n <= kCandCap candidate keys (fetch(j), j < n, any order) -> row_keys / row_valid.
// list: [kCandCap + 8] dwords of this wavefront's LDS.  Survivors = the min(n, k) largest keys -- the lexicographic
// (intensity, range) cut of FilterKstrongest (radar_filters.cpp:214-229), ties toward the larger range; the slot of a
// survivor = its rank among the survivors beyond min_range_bin (getPeaksFilteredPointCloud(cloud, false), :309-337).
template <typename Fetch>
__device__ __forceinline__ void select_row(const KStrongArgs& a, const long long row, const int n, uint32_t* list, const int lane,
                                           Fetch&& fetch) {
  uint32_t* bits = list + kCandCap + 4;
  constexpr int NR = kCandCap / 64;
  uint32_t key[NR];
#pragma unroll
  for (int i = 0; i < NR; i++) {
    const int j = i * 64 + lane;
    key[i] = 0xFFFFFFFFu;                                    // the padding ranks above every key
    if (i * 64 < n) {
      if (j < n) key[i] = fetch(j);
      list[j] = key[i];
    }
  }
  if (lane < 2) bits[lane] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int k = a.k, drop = n - min(n, k), nq = (n + 3) & ~3;
  int rank[NR];
  bool beyond[NR];
#pragma unroll
  for (int i = 0; i < NR; i++) {
    rank[i] = -1;
    beyond[i] = false;
    if (i * 64 < n) {                                        // wave-uniform
      if (i * 64 + lane < n) {
        int c = 0;
        for (int q = 0; q < nq; q += 4) {
          const uint4 x = *(const uint4*)(list + q);         // same address in every lane: LDS broadcast
          c += (x.x < key[i]) + (x.y < key[i]) + (x.z < key[i]) + (x.w < key[i]);
        }
        rank[i] = c - drop;
      }
      beyond[i] = rank[i] >= 0 && (int)(key[i] & 0xFFFFFFu) > a.min_range_bin;
      if (beyond[i]) atomicOr(&bits[rank[i] >> 5], 1u << (rank[i] & 31));      // (the survivors' ranks are < k <= 64)
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint32_t m0 = bits[0], m1 = bits[1];
#pragma unroll
  for (int i = 0; i < NR; i++) {
    if (beyond[i]) {
      const int rk = rank[i];
      const int idx = rk < 32 ? __popc(m0 & ((1u << rk) - 1u)) : __popc(m0) + __popc(m1 & ((1u << (rk - 32)) - 1u));
      a.row_keys[row * k + idx] = key[i];
    }
  }
  if (lane == 0) {
    a.row_valid[row * 2] = __popc(m0) + __popc(m1);
    a.row_valid[row * 2 + 1] = 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the list is reused by the wavefront's next row
  __builtin_amdgcn_wave_barrier();
}

// Two azimuths with at most 32 candidates each on one wavefront: lanes 0-31 take row[0], lanes 32-63 row[1] (the typical
// radar azimuth holds two or three dozen bins >= z_min, so select_row leaves half of its lanes idle).  fetch(h, j) = key j
// of the half's row; list: [64] keys + [2] bitmap words.
template <typename Fetch>
__device__ __forceinline__ void select_pair(const KStrongArgs& a, const long long row0, const long long row1, const int n0,
                                            const int n1, uint32_t* list, const int lane, Fetch&& fetch) {
  const int half = lane >> 5, h = lane & 31;
  const int n = half ? n1 : n0;
  const long long row = half ? row1 : row0;
  uint32_t* bits = list + 64;
  const uint32_t key = h < n ? fetch(half, h) : 0xFFFFFFFFu;
  list[lane] = key;
  if (h == 0) bits[half] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int k = a.k, drop = n - min(n, k);
  const int nq = (max(n0, n1) + 3) & ~3;                     // wave-uniform
  const uint32_t* mine = list + 32 * half;
  int c = 0;
  for (int q = 0; q < nq; q += 4) {
    const uint4 x = *(const uint4*)(mine + q);               // two addresses per instruction
    c += (x.x < key) + (x.y < key) + (x.z < key) + (x.w < key);
  }
  const int rank = h < n ? c - drop : -1;
  const bool beyond = rank >= 0 && (int)(key & 0xFFFFFFu) > a.min_range_bin;
  if (beyond) atomicOr(&bits[half], 1u << rank);             // (survivors' ranks are < min(n, k) <= 32)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint32_t m = bits[half];
  if (beyond) a.row_keys[row * k + __popc(m & ((1u << rank) - 1u))] = key;
  if (h == 0) {
    a.row_valid[row * 2] = __popc(m);
    a.row_valid[row * 2 + 1] = 0;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// a row whose list overflowed: its 16-column tile goes to kstrongest_cols_kernel (once)
__device__ __forceinline__ void flag_tile(const KStrongArgs& a, const int b, const int r, const int tiles, uint32_t* tile_flag,
                                          int32_t* work_n, uint32_t* work) {
  const uint32_t id = (uint32_t)b * (uint32_t)tiles + (uint32_t)((a.rows - 1 - r) / kColsTile);
  if (atomicExch(&tile_flag[id], 1u) == 0u) work[atomicAdd(work_n, 1)] = id;
}

// ---- small batches: many workgroups per image, the lists in global memory (one atomic per candidate) ---------------
__global__ __launch_bounds__(256) void kstrong_extract_kernel(const KStrongArgs a, const uint32_t seg_magic, const int segs,
                                                              int32_t* __restrict__ cand_cnt, uint32_t* __restrict__ cand) {
  const int b = a.batch0 + blockIdx.y;
  const uint8_t* img = a.polar + (long long)b * a.batch_stride;
  const uint32_t n_pieces = (uint32_t)a.cols * (uint32_t)segs;
  const uint32_t p0 = blockIdx.x * (256u * kExtractPieces) + threadIdx.x;
  uint32_t w[kExtractPieces][4];
  load_pieces(a, img, p0, 256u, n_pieces, seg_magic, segs, w);
  extract_candidates(a, w, p0, 256u, n_pieces, seg_magic, segs, [&](const int r, const uint32_t key) {
    const long long row = (long long)b * a.rows + r;
    const int slot = atomicAdd(&cand_cnt[row], 1);
    if (slot < kCandCap) cand[row * kCandCap + slot] = key;
  });
}

__global__ __launch_bounds__(256) void kstrong_select_kernel(const KStrongArgs a, const int tiles, const int32_t* __restrict__ cand_cnt,
                                                             const uint32_t* __restrict__ cand, uint32_t* tile_flag,
                                                             int32_t* work_n, uint32_t* work, uint32_t* stats) {
  __shared__ __attribute__((aligned(16))) uint32_t lists[kRowsPerBlock][kCandCap + 8];   // keys | 2 bitmap words
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r = blockIdx.x * kRowsPerBlock + wave;
  if (r >= a.rows) return;                                   // no workgroup barrier below
  const int b = a.batch0 + blockIdx.y;
  const long long row = (long long)b * a.rows + r;
  const int n = __builtin_amdgcn_readfirstlane(cand_cnt[row]);
  // how dense the batch is: every 16th azimuth reports, for 16 (an atomic per azimuth on 64 counters took longer than the
  // selection itself: 0.48 ms for 255 sweeps)
  if (stats && lane == 0 && (r & 15) == 0) atomicAdd(&stats[(blockIdx.x + blockIdx.y) & 63], 16u * (uint32_t)n);
  if (n > kCandCap) {                                        // the list is incomplete: the row needs its raw bytes
    if (lane == 0) flag_tile(a, b, r, tiles, tile_flag, work_n, work);
    return;
  }
  select_row(a, row, n, lists[wave], lane, [&](const int j) { return cand[row * kCandCap + j]; });
}

// ---- large batches: ONE workgroup streams a whole image; the lists of all its azimuths sit in LDS (the first lds_cap
// keys of each; the rest, up to kCandCap, in global memory), so a candidate costs an LDS atomic, and the same workgroup
// then picks the k strongest of every list: one kernel, nothing but the keys written.  Two workgroups per CU: one streams
// while the other selects.
constexpr int kImgWaves = 8;

__global__ __launch_bounds__(64 * kImgWaves, 4) void kstrong_image_kernel(const KStrongArgs a, const uint32_t seg_magic, const int segs,
                                                                           const int tiles, const int lds_cap,
                                                                           uint32_t* __restrict__ cand, uint32_t* tile_flag,
                                                                           int32_t* work_n, uint32_t* work, uint32_t* stats) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int rows4 = (a.rows + 3) & ~3;
  uint32_t* cnt = (uint32_t*)smem;                           // [rows]
  uint32_t* lists = cnt + rows4;                             // [rows][lds_cap]
  uint32_t* mine = lists + (size_t)a.rows * lds_cap + wave * (kCandCap + 8);
  const uint32_t n_pieces = (uint32_t)a.cols * (uint32_t)segs;
  constexpr uint32_t kThreads = 64 * kImgWaves;
  for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
    const uint8_t* img = a.polar + (long long)b * a.batch_stride;
    for (int i = threadIdx.x; i < a.rows; i += kThreads) cnt[i] = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_pieces; base += kThreads * kExtractPieces) {
      uint32_t w[kExtractPieces][4];
      load_pieces(a, img, base + threadIdx.x, kThreads, n_pieces, seg_magic, segs, w);
      extract_candidates(a, w, base + threadIdx.x, kThreads, n_pieces, seg_magic, segs, [&](const int r, const uint32_t key) {
        const int slot = (int)atomicAdd(&cnt[r], 1u);
        if (slot < lds_cap) lists[r * lds_cap + slot] = key;
        else if (slot < kCandCap) cand[((long long)b * a.rows + r) * kCandCap + slot] = key;
      });
    }
    __syncthreads();                                         // (also orders the overflow stores before the loads below)
    if (stats) {                                             // how dense the batch is: the image's candidates, 64 counters (no hot address)
      int local = 0;
      for (int i = threadIdx.x; i < a.rows; i += kThreads) local += (int)cnt[i];
      const int incl = wave_incl_scan_i32(local);
      if (lane == 63) atomicAdd(&stats[(b * kImgWaves + wave) & 63], (uint32_t)incl);
    }
    const int pair_cap = min(32, lds_cap);                   // (a pair's keys all come from LDS)
    for (int r = wave; r < a.rows; r += 2 * kImgWaves) {
      const int r1 = r + kImgWaves;
      const int n0 = (int)cnt[r], n1 = r1 < a.rows ? (int)cnt[r1] : 0;
      if (r1 < a.rows && n0 <= pair_cap && n1 <= pair_cap) {
        select_pair(a, (long long)b * a.rows + r, (long long)b * a.rows + r1, n0, n1, mine, lane,
                    [&](const int half, const int j) { return lists[(half ? r1 : r) * lds_cap + j]; });
        continue;
      }
      for (int i = 0; i < 2; i++) {
        const int rr = i ? r1 : r, n = i ? n1 : n0;
        if (rr >= a.rows) break;
        const long long row = (long long)b * a.rows + rr;
        if (n > kCandCap) {
          if (lane == 0) flag_tile(a, b, rr, tiles, tile_flag, work_n, work);
          continue;
        }
        select_row(a, row, n, mine, lane, [&](const int j) { return j < lds_cap ? lists[rr * lds_cap + j] : cand[row * kCandCap + j]; });
      }
    }
    __syncthreads();                                         // the counters are cleared for the next image
  }
}

// Persistent workgroups, two per CU.  With a work list: tile ids (image * tiles + tile), taken round robin.  Without:
// every tile of every image -- workgroup n lives on XCD n % 8 and is that XCD's slot n / 8; XCD x takes the images
// b = x (mod 8), tile after tile, its slots striding through that sequence together, so the (up to) eight tiles that
// share a 128-byte line are read by neighbouring slots of one XCD at about the same time.  While a workgroup runs the
// row algorithm on the tile in LDS, the 16-byte pieces of its NEXT tile are already in flight into registers.
template <int NCHUNK, bool MASK>
__global__ __launch_bounds__(64 * kColsWaves, 4) void kstrongest_cols_kernel(const KStrongArgs a, const int tiles,
                                                                              const uint32_t* __restrict__ work,
                                                                              const int32_t* __restrict__ work_n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int xcd = blockIdx.x % kXcds, slot = blockIdx.x / kXcds, slots = gridDim.x / kXcds;
  const int nq = work ? *work_n : ((a.batch - xcd + kXcds - 1) / kXcds) * tiles;       // items of this workgroup's sequence
  const int q0 = work ? (int)blockIdx.x : slot, dq = work ? (int)gridDim.x : slots;
  auto locate = [&](const int q, int& b, int& tile) {
    if (work) { const uint32_t id = work[q]; b = (int)(id / (uint32_t)tiles); tile = (int)(id - (uint32_t)b * (uint32_t)tiles); }
    else { const int im = q / tiles; b = im * kXcds + xcd; tile = q - im * tiles; }
  };
  const int bins = a.cols, cols16 = (bins + 15) & ~15;
  const int kpad = max((a.k + 3) & ~3, 64);
  constexpr int kScratch = kstrong_scratch_bytes(NCHUNK);
  uint8_t* tbase = smem;                                     // [kColsTile][cols16]: row lr = source column c0 + 15 - lr
  uint32_t* hist = (uint32_t*)(smem + kColsTile * cols16 + wave * (kScratch + kpad * 4));
  uint32_t* list = hist + kScratch / 4;
  constexpr int GP = (NCHUNK * 256 + 64 * kColsWaves - 1) / (64 * kColsWaves);   // groups of 4 bins per thread
  uint32_t rw[GP][4][4];
  // one 32-bit byte offset per group and thread (groups past the last bin re-read the last one; their tile bytes are
  // zeroed below), the bin row i and the tile folded into the wave-uniform base: SGPR base + VGPR offset addressing
  uint32_t goff[GP];
#pragma unroll
  for (int p = 0; p < GP; p++)
    goff[p] = (uint32_t)min((int)threadIdx.x + p * 64 * kColsWaves, (bins >> 2) - 1) * 4u * (uint32_t)a.stride;
  auto issue = [&](const int q) {                            // the pieces of item q: bins 4 g .. 4 g + 3, 16 source columns
    int b, tile;
    locate(q, b, tile);
    const uint8_t* src = a.polar + (long long)b * a.batch_stride + tile * kColsTile;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint8_t* bi = src + (long long)i * a.stride;
#pragma unroll
      for (int p = 0; p < GP; p++) {
        const u32x4 v = *(const u32x4*)(bi + (size_t)goff[p]);
        rw[p][i][0] = v.x; rw[p][i][1] = v.y; rw[p][i][2] = v.z; rw[p][i][3] = v.w;
      }
    }
  };
  int q = q0;
  if (q < nq) issue(q);
  while (q < nq) {
#pragma unroll
    for (int p = 0; p < GP; p++) {
      const int g = threadIdx.x + p * 64 * kColsWaves;
      if (4 * g < cols16) {
#pragma unroll
        for (int d = 0; d < 4; d++) {                        // source columns c0 + 4 d .. + 3 of bins 4 g .. 4 g + 3
          uint32_t colw[4];                                  // colw[e] = column c0 + 4 d + e as {bin 4g, +1, +2, +3}
          transpose4x4_bytes(rw[p][0][d], rw[p][1][d], rw[p][2][d], rw[p][3][d], colw);
#pragma unroll
          for (int e = 0; e < 4; e++)
            *(uint32_t*)(tbase + (kColsTile - 1 - (4 * d + e)) * cols16 + 4 * g) = 4 * g < bins ? colw[e] : 0u;
        }
      }
    }
    __syncthreads();
    int b, tile;
    locate(q, b, tile);
    const int qn = q + dq;
    if (qn < nq) issue(qn);
    const int r0 = a.rows - kColsTile - tile * kColsTile;    // output row of tile row 0
    for (int lr = wave; lr < kColsTile; lr += kColsWaves)
      kstrong_row<NCHUNK, true, MASK, true>(a, r0 + lr, b, a.polar, tbase + lr * cols16, hist, list, lane);
    __syncthreads();                                         // every row of the tile has been consumed
    q = qn;
  }
}

// ---- cloud compaction: radar_filters.cpp:309-337 -----------------------------------------------------------------------------
struct CloudArgs {
  const int32_t* sel_range;
  const uint8_t* sel_intensity;
  const int32_t* sel_count;
  const uint8_t* is_peak;
  const int32_t* row_valid;  // [batch][rows][2] written by kstrongest_rows_kernel
  const double* cos_t;      // [rows]
  const double* sin_t;
  int rows, k, min_range_bin;
  double range_res;
  float* xyzi;              // [batch][rows*k][4]
  int32_t* n_points;        // [batch]
  float* xyzi_peaks;
  int32_t* n_peaks;
};

constexpr int kCloudSplit = 8;   // workgroups per image: each scans all row counts, writes its row slice

__global__ __launch_bounds__(256) void kstrong_cloud_kernel(const CloudArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int32_t* row_off = (int32_t*)smem;                 // [rows + 1]
  __shared__ int32_t wave_tot[8];
  const int b = blockIdx.x;
  const bool peaks = blockIdx.y == 1;
  float* out = peaks ? a.xyzi_peaks : a.xyzi;
  int32_t* nout = peaks ? a.n_peaks : a.n_points;
  if (!out && !nout) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long ibase = (long long)b * a.rows * a.k;
  // This workgroup writes the rows [rbeg, rend) of the image: it needs the number of points in the rows before
  // its slice (one block reduction over all row counts) and a prefix inside the slice (one wavefront).
  const int rows_per = (a.rows + kCloudSplit - 1) / kCloudSplit;
  const int rbeg = blockIdx.z * rows_per, rend = min(a.rows, rbeg + rows_per);
  const int which = peaks ? 1 : 0;
  int before = 0, total = 0;
  for (int r = threadIdx.x; r < a.rows; r += 256) {
    const int v = a.row_valid[((long long)b * a.rows + r) * 2 + which];
    total += v;
    before += r < rbeg ? v : 0;
  }
  before = wave_sum_i32(before);
  total = wave_sum_i32(total);
  if (lane == 0) { wave_tot[wave] = before; wave_tot[4 + wave] = total; }
  __syncthreads();
  before = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
  total = wave_tot[4] + wave_tot[5] + wave_tot[6] + wave_tot[7];
  if (threadIdx.x == 0 && nout && blockIdx.z == 0) nout[b] = total;
  if (!out) return;
  if (wave == 0) {
    int run = before;
    for (int r0 = rbeg; r0 < rend; r0 += 64) {
      const int r = r0 + lane;
      const int v = r < rend ? a.row_valid[((long long)b * a.rows + r) * 2 + which] : 0;
      const int incl = wave_incl_scan_i32(v);
      if (r < rend) row_off[r] = run + incl - v;
      run += __builtin_amdgcn_readlane(incl, 63);
    }
  }
  __syncthreads();
  // one wavefront per row of this workgroup's slice writes its points in (intensity,range) order
  const double range_res_half = a.range_res / 2.0;
  // Every load of a row's first 64 slots is issued before any of them is used (the slots past the row's count
  // exist and are simply ignored), so a row costs one memory round trip instead of three dependent ones.
  for (int r = rbeg + wave; r < rend; r += 4) {
    const long long rb = ibase + (long long)r * a.k;
    const int cnt = a.sel_count[(long long)b * a.rows + r];
    const double cos_t = a.cos_t[r], sin_t = a.sin_t[r];
    int range0 = 0;
    uint8_t inten0 = 0, pk0 = 1;
    if (lane < a.k) {
      range0 = a.sel_range[rb + lane];
      inten0 = a.sel_intensity[rb + lane];
      if (peaks) pk0 = a.is_peak[rb + lane];
    }
    int base = row_off[r];
    for (int j0 = 0; j0 < cnt; j0 += 64) {
      const int j = j0 + lane;
      bool ok = false;
      int range = 0;
      uint8_t inten = 0;
      if (j < cnt) {
        if (j0 == 0) { range = range0; inten = inten0; ok = range > a.min_range_bin && pk0; }
        else {
          range = a.sel_range[rb + j];
          inten = a.sel_intensity[rb + j];
          ok = range > a.min_range_bin && (!peaks || a.is_peak[rb + j]);
        }
      }
      const unsigned long long bal = __ballot(ok);
      if (ok) {
        const int idx = base + __popcll(bal & ((1ull << lane) - 1ull));
        const double rho = range_res_half + a.range_res * (double)range;
        float4 p;
        p.x = (float)(rho * cos_t);
        p.y = (float)(rho * sin_t);
        p.z = 0.f;
        p.w = (float)inten;
        ((float4*)out)[(long long)b * a.rows * a.k + idx] = p;
      }
      base += __popcll(bal);
    }
  }
}

// ---- the dispatch table of the row sweep: index 4 log2(NCHUNK) + 2 VEC + MASK, as cfear_kstrong_plan documents it ----------
using KStrongFn = void (*)(const KStrongArgs);
constexpr int kKStrongEntries = 16;
#define CFEAR_KSTRONG_ROW4(N) \
  kstrongest_rows_kernel<N, false, false>, kstrongest_rows_kernel<N, false, true>, kstrongest_rows_kernel<N, true, false>, \
  kstrongest_rows_kernel<N, true, true>
const KStrongFn kKStrongTable[kKStrongEntries] = {CFEAR_KSTRONG_ROW4(1), CFEAR_KSTRONG_ROW4(2), CFEAR_KSTRONG_ROW4(4), CFEAR_KSTRONG_ROW4(8)};
#undef CFEAR_KSTRONG_ROW4
// two rows per wavefront (VEC, no peaks, NCHUNK <= 4): index 2 log2(NCHUNK) + MASK
constexpr int kKStrongPairEntries = 6;
const KStrongFn kKStrongPairTable[kKStrongPairEntries] = {
  kstrongest_rowpairs_kernel<1, false>, kstrongest_rowpairs_kernel<1, true>, kstrongest_rowpairs_kernel<2, false>,
  kstrongest_rowpairs_kernel<2, true>,  kstrongest_rowpairs_kernel<4, false>, kstrongest_rowpairs_kernel<4, true>};

// What follows from the filter's parameters alone, for the row sweep and the bins-major route alike: the candidate threshold,
// the bin the cloud starts beyond, and the list capacity (k survivors, or up to 64 candidates to rank).
struct KStrongDerived { int u_zmin, min_range_bin, kpad; };
KStrongDerived kstrong_derive(const cfear_kstrong_params* par) {
  KStrongDerived d;
  const int z_min_i = (int)par->z_min;                         // radar_driver.cpp:58 float -> int
  d.u_zmin = (int)(uint8_t)z_min_i;                            // radar_filters.cpp:212 uchar(z_min_)
  const double range_res_ = (double)par->range_res, min_distance_ = (double)par->min_distance;
  d.min_range_bin = (int)std::ceil(min_distance_ / range_res_);              // radar_filters.cpp:315
  d.kpad = std::max((par->k_strongest + 3) & ~3, 64);
  return d;
}

// The one selection: everything cfear_kstrong_device launches follows from the plan this fills.  No validation here (the entry
// points refuse what cfear_kstrong_plan reports as refused); base = the address of the first image.
void kstrong_select(const cfear_polar_desc* desc, const cfear_kstrong_params* par, uint64_t base, struct cfear_kstrong_plan& p) {
  memset(&p, 0, sizeof(p));
  const KStrongDerived dv = kstrong_derive(par);
  p.u_zmin = dv.u_zmin; p.min_range_bin = dv.min_range_bin; p.kpad = dv.kpad;
  p.thi = p.u_zmin >= 128;
  const int64_t batch_stride = desc->batch > 1 ? desc->batch_stride : (int64_t)desc->rows * desc->stride;
  p.vec = (base % 4 == 0) && (desc->stride % 4 == 0) && (batch_stride % 4 == 0);
  // Byte-validity masks only where a zero byte could pass a test, i.e. z_min == 0: load_row() zero-fills what lies beyond the row
  // (ragged widths: Oxford's native 3768 bins end 8 bytes into a 16-byte piece), every threshold the kernel compares with is
  // >= uchar(z_min), and the peaks' halo bytes are written behind the last re-read of the staged row.  (Until round 6 every
  // width that is not a multiple of 16 took the masked instantiation: 1.84 instead of 1.25 ms per 4096 Oxford-native sweeps.)
  p.mask = p.u_zmin == 0;
  const int need = (desc->cols + 1023) / 1024;
  const int lg = need <= 1 ? 0 : (need <= 2 ? 1 : (need <= 4 ? 2 : 3));
  p.nchunk = 1 << lg;
  p.table_index = 4 * lg + 2 * p.vec + p.mask;
  // per wavefront: the raw row and its two 16-byte halos | scratch | the key list (kstrongest_rows_kernel carves the same)
  p.lds_bytes = (int64_t)kRowsPerBlock * (p.nchunk * 1024 + 32 + kstrong_scratch_bytes(p.nchunk) + p.kpad * 4);
}

}  // namespace

extern "C" int cfear_kstrong_plan(const cfear_polar_desc* desc, const cfear_kstrong_params* par, uint64_t base_address,
                                  struct cfear_kstrong_plan* out) {
  if (!desc || !par || !out) return CFEAR_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  // what cfear_filter_kstrongest refuses, in its order (check_desc, k, range_res)
  const DescFault fault = polar_desc_fault(desc);
  if (fault == DescFault::kGeometry) out->refused = CFEAR_KSTRONG_REFUSED_DESC;
  else if (fault == DescFault::kTooWide) out->refused = CFEAR_KSTRONG_REFUSED_COLS;
  else if (par->k_strongest < 1 || par->k_strongest > kMaxK) out->refused = CFEAR_KSTRONG_REFUSED_K;
  else if (!(par->range_res > 0.f)) out->refused = CFEAR_KSTRONG_REFUSED_RANGE_RES;
  else kstrong_select(desc, par, base_address, *out);
  return CFEAR_OK;
}

// Device-side entry used by cfear_filter_kstrongest and by the odometry pipeline: everything is
// already in device memory; outputs that are nullptr are skipped.
int cfear_kstrong_device(cfear_ctx* ctx, const uint8_t* d_polar, const cfear_polar_desc* desc,
                         const cfear_kstrong_params* par, const cfear_kstrong_out* o, bool dense_halo,
                         const cfear_kstrong_fused* fused) {
  KStrongArgs a;
  a.row_keys = nullptr;
  a.image_offsets = fused ? (const long long*)fused->image_offsets : nullptr;
  if (fused && fused->row_keys) {
    if (par->k_strongest > 64) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "fused row keys need k <= 64");
    a.row_keys = fused->row_keys;
  }
  a.polar = d_polar;
  a.rows = desc->rows; a.cols = desc->cols; a.stride = desc->stride; a.batch = desc->batch;
  a.batch_stride = desc->batch > 1 ? desc->batch_stride : (int64_t)desc->rows * desc->stride;
  a.k = par->k_strongest;
  struct cfear_kstrong_plan plan;                             // the threshold, vec, mask, nchunk and the LDS size: cfear_kstrong_plan's own
  kstrong_select(desc, par, (uint64_t)(uintptr_t)d_polar, plan);
  a.u_zmin = plan.u_zmin;
  a.want_peaks = par->want_peaks && (o->is_peak != nullptr);
  a.sel_range = o->sel_range; a.sel_intensity = o->sel_intensity; a.sel_count = o->sel_count;
  a.is_peak = o->is_peak;
  const bool want_cloud = o->xyzi || o->n_points || o->xyzi_peaks || o->n_peaks;
  a.row_valid = nullptr;
  a.dense_halo = (dense_halo && desc->stride != desc->cols) ? 1 : 0;
  a.min_range_bin = plan.min_range_bin;
  if (fused && fused->row_valid) {
    a.row_valid = fused->row_valid;
  } else if (want_cloud) {
    a.row_valid = (int32_t*)cfear_workspace(ctx, kWsFilterRows, (size_t)desc->batch * desc->rows * 8);
    if (!a.row_valid) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  }
  if (plan.table_index < 0 || plan.table_index >= kKStrongEntries || plan.nchunk * 1024 < a.cols)   // a missing kernel is an error
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k-strongest: no kernel for %d bins", a.cols);
  // Two rows per wavefront wherever the pair kernel exists: 4-byte-aligned images, at most 4096 bins, no peaks (its fallback
  // reads the staged row, which keeps no halo bytes).  The plan keeps describing the single-row instantiation, which is what
  // everything else -- and CFEAR_OPT_KSTRONG_ROW_PAIRS = 0 -- launches.
  const bool pairs = plan.vec && plan.nchunk <= 4 && !a.want_peaks && ctx->kstrong_row_pairs != 0;
  const KStrongFn fn = pairs ? kKStrongPairTable[plan.table_index / 4 * 2 + plan.mask] : kKStrongTable[plan.table_index];
  const unsigned threads = pairs ? 64 * kRowsPerBlock / kPairRows : 64 * kRowsPerBlock;
  const size_t lds = pairs ? (size_t)(kRowsPerBlock / kPairRows) * kstrong_pair_wave_bytes(plan.nchunk, a.cols, plan.kpad) : (size_t)plan.lds_bytes;
  {
    ProfScope ps(ctx, "kstrongest_rows");
    for (int b0 = 0; b0 < a.batch; b0 += 65535) {             // gridDim.y limit
      a.batch0 = b0;
      dim3 grid((unsigned)((a.rows + kRowsPerBlock - 1) / kRowsPerBlock), (unsigned)std::min(65535, a.batch - b0));
      hipLaunchKernelGGL(fn, grid, dim3(threads), lds, ctx->stream, a);
    }
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  if (want_cloud) {
    double *d_cos = nullptr, *d_sin = nullptr;
    int rc = cfear_trig_tables(ctx, a.rows, &d_cos, &d_sin);
    if (rc != CFEAR_OK) return rc;
    CloudArgs c;
    c.sel_range = o->sel_range; c.sel_intensity = o->sel_intensity; c.sel_count = o->sel_count;
    c.is_peak = o->is_peak;
    c.row_valid = a.row_valid;
    c.cos_t = d_cos; c.sin_t = d_sin;
    c.rows = a.rows; c.k = a.k;
    c.min_range_bin = a.min_range_bin;
    c.range_res = (double)par->range_res;
    c.xyzi = o->xyzi; c.n_points = o->n_points;
    const bool pk = a.want_peaks && (o->xyzi_peaks || o->n_peaks);
    c.xyzi_peaks = pk ? o->xyzi_peaks : nullptr;
    c.n_peaks = pk ? o->n_peaks : nullptr;
    ProfScope ps(ctx, "kstrong_cloud");
    hipLaunchKernelGGL(kstrong_cloud_kernel, dim3(a.batch, pk ? 2 : 1, kCloudSplit), dim3(256),
                       (size_t)(a.rows + 1) * 4, ctx->stream, c);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
  }
  return CFEAR_OK;
}

// [range bins][azimuths] sources, fused decode + sweep (kstrongest_cols_kernel): `sd` describes the SOURCE images (rows =
// range bins, cols = azimuths).  Only the batched odometry's key output; whatever this path does not take (peaks, k > 64,
// unaligned or ragged images, more than 4096 bins) goes through cfear_rotate_ccw_device + cfear_kstrong_device.
bool cfear_kstrong_cols_supported(const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_kstrong_params* par) {
  // azimuths (sd->cols) <= 4096: the image route's fixed LDS part and the exact range of the umulhi division by the number of
  // 16-azimuth segments (p * segs < 2^32 with p < bins * segs) both depend on it
  return par->k_strongest <= 64 && sd->rows <= 4096 && sd->cols <= 4096 && sd->rows % 4 == 0 && sd->cols % kColsTile == 0 && sd->stride % 16 == 0 &&
         (uintptr_t)d_src % 16 == 0 && (sd->batch <= 1 || sd->batch_stride % 16 == 0) &&
         (int64_t)sd->rows * sd->stride < ((int64_t)1 << 31);
}

// ... and pays: a handful of sweeps (one radar alone) are done sooner by the rotation kernel + the row sweep (20 us against
// 37 us for one image through the global lists; a workgroup alone streams its image in ~100 us whatever the batch).  From
// 128 images on the image-per-workgroup kernel wins (128: 0.11 ms against ~0.10 for the two kernels in the pipeline and 0.11
// for the global lists; 192: 0.11 / 0.15 / 0.14; tools/decode_bench.py N --image | --lists | --two-pass).
bool cfear_kstrong_cols_preferred(const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_kstrong_params* par) {
  return sd->batch >= 128 && cfear_kstrong_cols_supported(d_src, sd, par);
}

namespace {

// ---- the dispatch table of the tile sweep: index 2 log2(NCHUNK) + MASK ------------------------------------------------------
using KStrongColsFn = void (*)(const KStrongArgs, int, const uint32_t*, const int32_t*);
constexpr int kKStrongColsEntries = 6;
const KStrongColsFn kKStrongColsTable[kKStrongColsEntries] = {
    kstrongest_cols_kernel<1, false>, kstrongest_cols_kernel<1, true>, kstrongest_cols_kernel<2, false>,
    kstrongest_cols_kernel<2, true>,  kstrongest_cols_kernel<4, false>, kstrongest_cols_kernel<4, true>};

// How the candidates reach the selection.  Lists: kstrong_extract_kernel + kstrong_select_kernel, the lists in global memory;
// image: kstrong_image_kernel, a workgroup per image with the lists in LDS; both leave the azimuths whose list overflowed to
// the tile sweep.  Tiles: no lists, kstrongest_cols_kernel takes every tile.
enum KStrongColsRoute { kColsLists, kColsImage, kColsTiles };

struct KStrongColsPlan {
  KStrongDerived dv;
  KStrongColsRoute route;
  int nchunk, mask, table_index, tiles;    // the tile sweep (every route ends with it) ...
  size_t tile_lds; unsigned tile_grid;
  int segs, lds_cap;                       // the lists: 16-azimuth segments of a source row; keys of a list the image route keeps in LDS
  uint32_t magic, n_pieces;                // p / segs = umulhi(p, magic); 16-byte pieces of an image
  size_t o_flag, o_wn, o_work, o_cand, scratch_bytes, img_lds;   // scratch: candidate counts | tile flags | work count | work list | keys
};

// The one selection of the bins-major route: everything cfear_kstrong_cols_device launches follows from the plan this fills.
// sd = the SOURCE images, as cfear_kstrong_cols_supported accepts them; route: 0 = by the azimuth count, 1 = lists in global
// memory, 2 = one workgroup per image, 3 = every tile through the LDS transposition.
void kstrong_cols_select(const cfear_polar_desc* sd, const cfear_kstrong_params* par, int route, int n_cu, KStrongColsPlan& p) {
  const int azimuths = sd->cols, bins = sd->rows;
  p.dv = kstrong_derive(par);
  const int need = (bins + 1023) / 1024;
  const int lg = need <= 1 ? 0 : (need <= 2 ? 1 : (need <= 4 ? 2 : 3));
  p.nchunk = 1 << lg;
  p.mask = (bins % 16 != 0) || p.dv.u_zmin == 0;
  p.table_index = 2 * lg + p.mask;
  p.tiles = azimuths / kColsTile;
  p.tile_lds = (size_t)kColsTile * ((bins + 15) & ~15) + (size_t)kColsWaves * (kstrong_scratch_bytes(p.nchunk) + p.dv.kpad * 4);
  // persistent: two workgroups per CU (LDS), a multiple of the XCD count; fewer when the batch is small
  p.tile_grid = (unsigned)(xcd_grid_slots(p.tiles, sd->batch, n_cu, 2) * kXcds);
  const size_t n_rows = (size_t)sd->batch * azimuths, n_tiles = (size_t)sd->batch * p.tiles;
  p.o_flag = n_rows * 4; p.o_wn = p.o_flag + n_tiles * 4; p.o_work = p.o_wn + 256; p.o_cand = (p.o_work + n_tiles * 4 + 255) / 256 * 256;
  p.scratch_bytes = p.o_cand + n_rows * kCandCap * 4;
  p.segs = azimuths / 16;
  p.magic = (uint32_t)(((uint64_t)1 << 32) / (uint32_t)p.segs) + 1u;   // p / segs = umulhi(p, magic) while p * segs < 2^32; segs = 1 is taken apart in the kernel
  p.n_pieces = (uint32_t)bins * (uint32_t)p.segs;
  // image-per-workgroup route: its LDS holds rows * (1 + lds_cap) dwords
  const size_t img_fixed = (size_t)((azimuths + 3) & ~3) * 4 + (size_t)kImgWaves * (kCandCap + 8) * 4;
  const size_t img_budget = 80 * 1024 - 512;
  p.lds_cap = img_fixed >= img_budget ? 0 : (int)std::min<size_t>(40, (img_budget - img_fixed) / ((size_t)azimuths * 4));
  p.img_lds = img_fixed + (size_t)azimuths * p.lds_cap * 4;
  if (route == 3 || p.dv.u_zmin == 0) p.route = kColsTiles;   // z_min = 0: every bin is a candidate, the lists would only overflow
  else if (route == 2 || (route == 0 && p.lds_cap >= 16)) p.route = kColsImage;   // (the global lists: azimuth counts whose lists do not fit the LDS)
  else p.route = kColsLists;
}

}  // namespace

int cfear_kstrong_cols_device(cfear_ctx* ctx, const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_kstrong_params* par,
                              const cfear_kstrong_fused* fused, int route) {
  if (!fused || !fused->row_keys || !fused->row_valid || !cfear_kstrong_cols_supported(d_src, sd, par))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "fused decode: unsupported image geometry or outputs");
  KStrongColsPlan plan;
  kstrong_cols_select(sd, par, route, ctx->n_cu, plan);
  if (plan.table_index < 0 || plan.table_index >= kKStrongColsEntries || plan.nchunk * 1024 < sd->rows)   // a missing kernel is an error
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k-strongest: no kernel for %d bins", sd->rows);
  if (plan.route == kColsImage && plan.lds_cap < 1)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "fused decode: too many azimuths for the image route");
  KStrongArgs a{};
  a.polar = d_src;
  a.rows = sd->cols; a.cols = sd->rows; a.stride = sd->stride; a.batch = sd->batch;
  a.batch_stride = sd->batch > 1 ? sd->batch_stride : (int64_t)sd->rows * sd->stride;
  a.k = par->k_strongest; a.u_zmin = plan.dv.u_zmin; a.min_range_bin = plan.dv.min_range_bin;
  a.row_keys = fused->row_keys; a.row_valid = fused->row_valid;
  const int tiles = plan.tiles;
  uint32_t* work = nullptr;                                  // no work list: the tile sweep takes every tile
  int32_t* work_n = nullptr;
  if (fused->cand_stats) CFEAR_HIP_CHECK(ctx, hipMemsetAsync(fused->cand_stats, 0, 64 * 4, ctx->stream));
  if (plan.route != kColsTiles) {
    char* ws = (char*)cfear_workspace(ctx, kWsKstrongCand, plan.scratch_bytes);
    if (!ws) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
    int32_t* cand_cnt = (int32_t*)ws;
    uint32_t* tile_flag = (uint32_t*)(ws + plan.o_flag);
    uint32_t* cand = (uint32_t*)(ws + plan.o_cand);
    work_n = (int32_t*)(ws + plan.o_wn);
    work = (uint32_t*)(ws + plan.o_work);
    if (plan.route == kColsImage) {
      CFEAR_HIP_CHECK(ctx, hipMemsetAsync(ws + plan.o_flag, 0, plan.o_work - plan.o_flag, ctx->stream));
      { const int rc_lds = cfear_allow_lds(ctx, (const void*)kstrong_image_kernel, 160 * 1024); if (rc_lds != CFEAR_OK) return rc_lds; }
      ProfScope ps(ctx, "kstrong_image");
      hipLaunchKernelGGL(kstrong_image_kernel, dim3((unsigned)std::min(a.batch, 2 * ctx->n_cu)), dim3(64 * kImgWaves), plan.img_lds,
                         ctx->stream, a, plan.magic, plan.segs, tiles, plan.lds_cap, cand, tile_flag, work_n, work, fused->cand_stats);
      CFEAR_HIP_CHECK(ctx, hipGetLastError());
    } else {
      CFEAR_HIP_CHECK(ctx, hipMemsetAsync(ws, 0, plan.o_work, ctx->stream));
      for (int b0 = 0; b0 < a.batch; b0 += 65535) {             // gridDim.y limit
        a.batch0 = b0;
        const unsigned by = (unsigned)std::min(65535, a.batch - b0);
        {
          ProfScope ps(ctx, "kstrong_extract");
          hipLaunchKernelGGL(kstrong_extract_kernel, dim3((plan.n_pieces + 256 * kExtractPieces - 1) / (256 * kExtractPieces), by),
                             dim3(256), 0, ctx->stream, a, plan.magic, plan.segs, cand_cnt, cand);
        }
        {
          ProfScope ps(ctx, "kstrong_select");
          hipLaunchKernelGGL(kstrong_select_kernel, dim3((a.rows + kRowsPerBlock - 1) / kRowsPerBlock, by), dim3(256), 0, ctx->stream, a,
                             tiles, cand_cnt, cand, tile_flag, work_n, work, fused->cand_stats);
        }
        CFEAR_HIP_CHECK(ctx, hipGetLastError());
      }
      a.batch0 = 0;
    }
  }
  const KStrongColsFn fn = kKStrongColsTable[plan.table_index];
  ProfScope ps(ctx, "kstrongest_cols");
  (void)cfear_allow_lds(ctx, (const void*)fn, 160 * 1024);
  hipLaunchKernelGGL(fn, dim3(plan.tile_grid), dim3(64 * kColsWaves), plan.tile_lds, ctx->stream, a, tiles, (const uint32_t*)work,
                     (const int32_t*)work_n);
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

extern "C" int cfear_filter_kstrongest_rowkeys(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                               const cfear_kstrong_params* par, int32_t flags, uint32_t* row_keys,
                                               int32_t* row_counts) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!polar || !par || !row_keys || !row_counts) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  const bool bins_major = (flags & CFEAR_ROWKEYS_BINS_MAJOR) != 0;
  if (polar_desc_fault(desc, bins_major) != DescFault::kNone)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad polar descriptor");
  if (par->k_strongest < 1 || par->k_strongest > 64)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "row keys need k_strongest in [1,64]");
  if (!(par->range_res > 0.f)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "range_res must be > 0");
  if (!cfear_is_device_ptr(polar) || !cfear_is_device_ptr(row_keys) || !cfear_is_device_ptr(row_counts))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "images and outputs must be device memory");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  cfear_kstrong_params kp = *par;
  kp.want_peaks = 0;
  cfear_kstrong_fused fz;
  fz.row_keys = row_keys;
  fz.row_valid = row_counts;
  cfear_kstrong_out none{};
  if (!bins_major) return cfear_kstrong_device(ctx, polar, desc, &kp, &none, false, &fz);
  const bool routed = (flags & (CFEAR_ROWKEYS_TILE_SWEEP | CFEAR_ROWKEYS_ROUTE_LISTS | CFEAR_ROWKEYS_ROUTE_IMAGE)) != 0;
  if (!(flags & CFEAR_ROWKEYS_TWO_PASS) &&
      (routed ? cfear_kstrong_cols_supported(polar, desc, &kp) : cfear_kstrong_cols_preferred(polar, desc, &kp)))
    return cfear_kstrong_cols_device(ctx, polar, desc, &kp, &fz, (flags & CFEAR_ROWKEYS_TILE_SWEEP) ? 3 : ((flags >> 4) & 3));
  cfear_polar_desc rd{};                                      // the rotated images: rows = azimuths
  rd.rows = desc->cols; rd.cols = desc->rows; rd.stride = (desc->rows + 15) & ~15; rd.batch = desc->batch;
  rd.batch_stride = (int64_t)rd.rows * rd.stride;
  uint8_t* rot = (uint8_t*)cfear_workspace(ctx, kWsImages, (size_t)rd.batch_stride * rd.batch);
  if (!rot) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
  const int rc = cfear_rotate_ccw_device(ctx, polar, desc, rot, rd.stride, rd.batch_stride);
  if (rc != CFEAR_OK) return rc;
  return cfear_kstrong_device(ctx, rot, &rd, &kp, &none, true, &fz);
}

extern "C" int cfear_filter_kstrongest(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                       const cfear_kstrong_params* par, const cfear_kstrong_out* out) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!polar || !par || !out) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_desc(ctx, desc));
  if (par->k_strongest < 1 || par->k_strongest > kMaxK)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "k_strongest must be in [1,%d]", kMaxK);
  if (!(par->range_res > 0.f))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "range_res must be > 0");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, k = par->k_strongest, batch = desc->batch;
  const size_t nsel = (size_t)batch * rows * k;
  const bool want_pk = par->want_peaks && (out->is_peak || out->xyzi_peaks || out->n_peaks);
  HostStage st(ctx, kWsFilter);
  const uint8_t* d_polar;
  const cfear_polar_desc dd = st.images(d_polar, polar, *desc);
  cfear_kstrong_out d{};                                      // the selection (and peak flags) always; the rest if asked for
  st.out(d.sel_range, out->sel_range, nsel * 4);
  st.out(d.sel_intensity, out->sel_intensity, nsel);
  st.out(d.sel_count, out->sel_count, (size_t)batch * rows * 4);
  if (want_pk) st.out(d.is_peak, out->is_peak, nsel);
  if (out->xyzi) st.out(d.xyzi, out->xyzi, nsel * 16);
  if (out->n_points) st.out(d.n_points, out->n_points, (size_t)batch * 4);
  if (want_pk && out->xyzi_peaks) st.out(d.xyzi_peaks, out->xyzi_peaks, nsel * 16);
  if (want_pk && out->n_peaks) st.out(d.n_peaks, out->n_peaks, (size_t)batch * 4);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(cfear_kstrong_device(ctx, d_polar, &dd, par, &d));
  return st.finish();
}
