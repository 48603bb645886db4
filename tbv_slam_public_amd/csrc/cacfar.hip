// cacfar.hip -- the CA-CFAR filter of the polar radar image: AzimuthCACFAR::getFilteredPointCloud / getMean (cfear_radarodometry/
// src/cfear_radarodometry/cfar.cpp:35-83), DESIGN.md 4.2.  cfar_row with cacfar_rows_kernel (a wavefront per azimuth row) and
// cacfar_cols_kernel ([range bins][azimuths] sources, keys only), cacfar_cloud_kernel, the one selection (cfar_derive, cfar_plan)
// with cfear_cacfar_device, which launches from it, and the entry points cfear_cacfar_plan, cfear_filter_cacfar[_rowkeys].
#include <cmath>

#include "polar_common.hpp"

namespace {

constexpr int kCfarCloudSplit = 8;    // CA-CFAR clouds: 25 slices (16 rows per workgroup) measured slower, 0.146 vs 0.137 ms per 512 sweeps: every workgroup re-scans the row counts
struct CfarArgs {
  const uint8_t* polar;
  int rows, cols, stride, batch;
  long long batch_stride;
  long long total_rows;
  int window, guard;
  double scaling, range_res, static_threshold, min_distance, max_distance;
  // bitmap output (standalone filter; cacfar_cloud_kernel compacts it)
  unsigned long long* det_bits;   // [batch][rows][words]  (words = ceil(cols/64))
  int32_t* det_count;             // [batch][rows]
  int words;
  // key output (batched odometry): row r of image b leaves its detections as (intensity << 24 | bin), ascending bins, at
  // row_keys[(b rows + r) kcap ...] and their number in row_cnt[2 (b rows + r)] -- the layout surface_prep_kernel
  // already takes from the k-strongest sweep, so no cloud kernel runs in between
  uint32_t* row_keys;
  int32_t* row_cnt;
  int kcap;
  int list_cap;                   // entries of a wavefront's candidate list (cacfar_cols_kernel: shorter than a chunk)
  int thr_i, bin_lo, bin_hi;      // candidate pre-test in integers: intensity >= thr_i, bin_lo <= bin < bin_hi
  int need_cols;                  // bins a row's arithmetic can touch: min(cols, bin_hi - 1 + guard + window), in 16s
  int colsp;                      // need_cols in whole 1024-bin chunks: the row's length in LDS
  int lut_ok;                     // lut[] decides a candidate with two full windows in integers
  int pre_on;                     // lower-bound pre-filter on (pa*, pb*, kappa_lb valid)
  int pa0, pa1, pb0, pb1;         // quads [2H + pa0, 2H + pa1) / [2H + pb0, 2H + pb1) lie in the trailing / forwarding
                                  // window of EVERY bin of the 8-bin block H
  int pad_lo, pad_hi;             // guard entries of the prefix table below bin 0 / beyond the row
  float kappa_lb;                 // scaling / (2 window), rounded down a little
  uint32_t lut[256];              // see cfar_build_lut
};

// One wavefront per azimuth row, persistent: a wavefront walks rows g, g + W, g + 2 W, ... and requests the NEXT row's
// 16-byte pieces before it works on the current one, so the HBM round trip hides behind its own arithmetic (the version
// before ran one row per wavefront and 12 wavefronts per CU: a third of a row's residence was the wait for its loads).
//
// Per row:
//  A. the row's bytes and the exact uint32 prefix sums of their squares go to LDS: 16 bins are summed inside a lane
//     (v_dot4), ONE wave scan per 1024 bins places the lanes, the table keeps every fourth prefix (P(x) = P4[x / 4] + the
//     squares of up to three bytes of one LDS word).  Only the bins the arithmetic can reach are read at all: with
//     radar_driver.cpp:54's 400 m cap a Kvarntorp row ends at bin 2286 + guard + window.
//  B. candidates.  cfar.cpp:45 lets a bin through when intensity > static_threshold inside the range window; here a bin
//     must ALSO beat a lower bound of its own CFAR threshold: the aligned 4-bin groups that lie inside the trailing /
//     forwarding window of every bin of an 8-bin block (56 of 80 bins for guard 10, window 40) give S_lb <= S_t + S_f from
//     four prefix reads per block, and I^2 > scaling (S_t / n_t + S_f / n_f) / 2 >= scaling S_lb / (2 w) is necessary for
//     a detection (n_t, n_f <= w).  So each block compares its bytes (SWAR) against max(thr_i, floor(sqrt(kappa S_lb)))
//     instead of thr_i alone: a quarter of the candidates survive on the synthetic Kvarntorp rows, and nothing that can
//     fire is lost.  Survivors are listed in LDS in bin order (a wave scan of the popcounts places the lanes).
//  C. the list is evaluated one candidate per lane, 64 at a time, carrying the remainder from chunk to chunk so that
//     every round but the last is full.  With both windows full the decision is an integer compare: with S = S_t + S_f
//     the reference computes  I^2 > scaling ((S_t / w + S_f / w) / 2)  in fp64, which differs from the exact
//     I^2 > S scaling / (2 w) by at most 5 roundings of 2^-53 -- so with B = I^2 2 w / scaling it fires for S <= B - 1e-3
//     and does not for S >= B + 1e-3, and lut[I] = (T << 1 | amb) with T = ceil(B - 1e-3), amb = an integer lies within
//     1e-3 of B:  fires <=> 2 S + 1 < lut[I];  2 S + 1 == lut[I] (practically never) and bins whose windows the row's ends
//     cut take cfar.cpp:45-60 literally in fp64.
//  D. detections leave in list (= bin) order: as keys for surface_prep_kernel (batched odometry) or as a bit per bin.
constexpr int kCfarListSlack = 64 + 64;     // list entries = one chunk's bins + the carried remainder (a 576-entry list with windowed
                                           // appends admits a fifth workgroup per CU and measured 4 % SLOWER: the kernel is
                                           // bound by VALU issue, not by latency)
__host__ __device__ inline size_t cfar_wave_lds(int colsp, int pad_lo, int pad_hi, bool keys, int chunk_bins) {
  // P4 u32[pad_lo + colsp / 4 + 1 + pad_hi] | raw u8[colsp + 16] | det u32[colsp / 32] (bitmap output) | list u16[chunk + slack]
  size_t b = ((size_t)(pad_lo + colsp / 4 + 1 + pad_hi) * 4 + 15) & ~(size_t)15;
  b += (size_t)colsp + 16;
  if (!keys) b += (size_t)colsp / 8;
  b += (size_t)(chunk_bins + kCfarListSlack) * 2;
  return (b + 15) & ~(size_t)15;
}
// D = dwords a lane owns per chunk (4, 6 or 8: a chunk is 256 D bins), NCH = chunks the registers hold.  The per-chunk
// overhead (two wave scans, the list loop, the round bookkeeping) is paid per CHUNK, so the host picks the D that covers
// the reachable bins with the fewest chunks: 2336 bins of a Kvarntorp row are 2 chunks of 1536 (D = 6) instead of 3 of
// 1024, of which the third held 18 busy lanes and cost 18 % of the kernel.
// DL = dwords per lane of the LAST chunk (DL <= D; DL < D only with exactly NCH chunks): 2336 reachable bins are a chunk
// of 1536 (D = 6) and one of 1024 (DL = 4) -- ten dwords per lane and row instead of twelve.
// One row of CA-CFAR on one wavefront (steps A .. D of cacfar_rows_kernel's comment): the row's bytes are in `cur` (lane l
// owns the dwords [j CB + l 4 D_j ..) of chunk j) and -- STAGED -- already in LDS at `raw` (the reachable a.need_cols bytes + 16 zeros).
// grow = the row's index in the OUTPUT (image * rows + azimuth); key_base = grow * kcap.
template <int D, int NCH, int DL, bool KEYS, bool PRE, bool STAGED, typename AfterSwar>
__device__ __forceinline__ void cfar_row(const CfarArgs& a, const int lane, const uint32_t* lut, uint32_t* P4, uint8_t* raw, uint32_t* det32,
                                         unsigned short* list, uint32_t (&cur)[NCH][D], const int nch, const long long grow,
                                         const long long key_base, AfterSwar&& after_swar) {
  constexpr int CB = 256 * D;
  auto DJ = [](int j) { return (DL != D && j == NCH - 1) ? DL : D; };
  const int colsp = a.colsp;
  auto lds_put = [&](void* at, const uint32_t (&v)[D], int dj) {               // the first dj dwords of v
    if (dj % 4 == 0) {
#pragma unroll
      for (int k = 0; k < D / 4; k++) if (4 * k < dj) ((uint4*)at)[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < D / 2; k++) if (2 * k < dj) ((uint2*)at)[k] = make_uint2(v[2 * k], v[2 * k + 1]);
    }
  };
  // LDS hand-over between the lanes of this wavefront.  The fences name the LDS address space only: a plain wavefront
  // fence makes the compiler wait for vmcnt(0) too, i.e. for the NEXT row's loads that were just requested.
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
  };
  auto P = [&](int x) -> uint32_t {                                         // sum_{q < x} I_q^2, 0 <= x <= colsp
    const int q = x >> 2, rr = x & 3;
    // the first rr bytes of the word (none for rr = 0; the word of x = colsp is the 16 bytes of padding): no branch
    const uint32_t wd = *(const uint32_t*)(raw + 4 * q) & ((1u << (8 * rr)) - 1u);
    return __builtin_amdgcn_udot4(wd, wd, P4[q], false);
  };
#ifdef CFEAR_CFAR_TIMING
  long long tq[6] = {0, 0, 0, 0, 0, 0}; int ctot = 0, nrounds = 0;
#define CFAR_T0() long long t_ = __builtin_readcyclecounter()
#define CFAR_T(k) { const long long n_ = __builtin_readcyclecounter(); tq[k] += n_ - t_; t_ = n_; }
#else
#define CFAR_T0()
#define CFAR_T(k)
#endif
  CFAR_T0();
    // ---- A: bytes + prefix sums of squares -> LDS ---------------------------------------------------------------
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      if (j >= nch) break;
      const int dj = DJ(j);
      const int pos = j * CB + lane * 4 * dj;
      if (!STAGED) lds_put(raw + pos, cur[j], dj);                            // (a staged row already sits there)
      uint32_t pre[D];                                                      // sums of squares before each of the lane's quads
      uint32_t acc = 0;
#pragma unroll
      for (int d = 0; d < D; d++) if (d < dj) { pre[d] = acc; acc += __builtin_amdgcn_udot4(cur[j][d], cur[j][d], 0u, false); }
      const int incl = wave_incl_scan_i32((int)acc);
      const uint32_t base = run + (uint32_t)incl - acc;                     // sum before this lane's first bin
#pragma unroll
      for (int d = 0; d < D; d++) if (d < dj) pre[d] += base;
      lds_put(P4 + (pos >> 2), pre, dj);
      run += (uint32_t)__builtin_amdgcn_readlane(incl, 63);
    }
    if (lane == 0) P4[colsp >> 2] = run;                                    // P(colsp)
    for (int i = lane; i < a.pad_hi; i += 64) P4[(colsp >> 2) + 1 + i] = run;
    if (!KEYS) for (int i = lane; i < colsp / 32; i += 64) det32[i] = 0u;
    wave_sync();
    CFAR_T(0);
    // ---- B + C -------------------------------------------------------------------------------------------------
    int C = 0, ndet = 0;
    // W candidates per lane and round (W = 1, 2): candidate k0 + 64 w + lane, w < W.  The decision of one candidate is a chain
    // of dependent LDS reads (list -> byte and four prefixes -> table); with two per lane the two chains interleave, and a
    // row's ~100 survivors take ONE round of 128 instead of a full and a partial round of 64 (the rounds were 38 % of a
    // row's cycles).  Detections still leave in list (= bin) order: the first 64 candidates' keys, then the second 64's.
    auto rounds = [&](auto w_tag, int k0, int cnt) {
      constexpr int W = decltype(w_tag)::value;
      bool act[W], valid[W], full[W], det[W], slow[W], edge[W];
      int bin[W], nt[W], nf[W];
      uint32_t v[W], st[W], sf[W];
#pragma unroll
      for (int w = 0; w < W; w++) {
        act[w] = 64 * w + lane < cnt;
        bin[w] = 0; v[w] = 0;
        if (act[w]) bin[w] = list[k0 + 64 * w + lane];
      }
#pragma unroll
      for (int w = 0; w < W; w++) if (act[w]) v[w] = raw[bin[w]];
#pragma unroll
      for (int w = 0; w < W; w++) {
        const int t1 = bin[w] - a.guard, t0 = t1 - a.window, f0 = bin[w] + a.guard, f1 = f0 + a.window;   // cfar.cpp:48-53
        const int lt0 = max(t0, 0), lf1 = min(f1, a.cols);                   // the windows as the row's ends cut them
        nt[w] = t1 - lt0; nf[w] = lf1 - f0;
        // getMean over an empty window is 0 / 0 = NaN: no detection (a window "ending" before bin 0 compares a size_t index
        // with a negative end in the reference -- undefined there, no detection here)
        valid[w] = act[w] && nt[w] > 0 && nf[w] > 0;
        st[w] = P(max(t1, 0)) - P(lt0); sf[w] = P(lf1) - P(min(f0, colsp));
        full[w] = nt[w] == a.window && nf[w] == a.window;
        det[w] = false; slow[w] = false; edge[w] = false;
      }
      if (PRE) {
        bool any_edge = false;
#pragma unroll
        for (int w = 0; w < W; w++) {
          // both windows full (every bin but the row's ends): the integer decision of step C
          const uint32_t X = 2u * (st[w] + sf[w]) + 1u, L = lut[v[w]];
          det[w] = valid[w] && full[w] && X < L;
          slow[w] = valid[w] && full[w] && X == L;
          edge[w] = valid[w] && !full[w];
          any_edge = any_edge || edge[w];
        }
        if (__ballot(any_edge)) {
#pragma unroll
          for (int w = 0; w < W; w++) {
            // a cut window: I^2 > scaling (S_t / n_t + S_f / n_f) / 2  <=>  I^2 2 n_t n_f > scaling (S_t n_f + S_f n_t) up to
            // six roundings of 2^-53; the integers on both sides are exact in fp64, so unless the two sides agree to 1e-12
            // the comparison is decided without the reference's divisions
            const double lhs = (double)(v[w] * v[w]) * (double)(2 * nt[w] * nf[w]);
            const double rhs = a.scaling * ((double)st[w] * (double)nf[w] + (double)sf[w] * (double)nt[w]);
            const double d = lhs - rhs;
            const bool sure = fabs(d) > fabs(rhs) * 1e-12;
            if (edge[w]) { det[w] = sure && d > 0.0; slow[w] = !sure; }
          }
        }
      } else {
#pragma unroll
        for (int w = 0; w < W; w++) slow[w] = valid[w];
      }
      bool any_slow = false;
#pragma unroll
      for (int w = 0; w < W; w++) any_slow = any_slow || slow[w];
      if (__ballot(any_slow)) {
#pragma unroll
        for (int w = 0; w < W; w++)
          if (slow[w]) {                                                      // cfar.cpp:55-60, literally
            const double trailing_mean = (double)st[w] / (double)nt[w];
            const double forwarding_mean = (double)sf[w] / (double)nf[w];
            const double mean = (trailing_mean + forwarding_mean) / 2.0;      // :56
            const double threshold = a.scaling * mean;                        // :58
            det[w] = (double)(v[w] * v[w]) > threshold;                       // :59-60
          }
      }
#pragma unroll
      for (int w = 0; w < W; w++) {
        if (KEYS) {
          const unsigned long long dm = __ballot(det[w]);
          const int at = ndet + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0u));
          if (det[w] && at < a.kcap) a.row_keys[key_base + at] = (v[w] << 24) | (uint32_t)bin[w];
          ndet += __popcll(dm);
        } else {
          if (det[w]) atomicOr(&det32[bin[w] >> 5], 1u << (bin[w] & 31));
        }
      }
#ifdef CFEAR_CFAR_TIMING
      nrounds++;
#endif
    };
    auto round = [&](int k0, int cnt) { rounds(std::integral_constant<int, 1>{}, k0, cnt); };
    auto round2 = [&](int k0, int cnt) { rounds(std::integral_constant<int, 2>{}, k0, cnt); };
    // candidate test "byte >= t" for four bytes at once: with tl = t & 127 and y = ((x & 0x7f..) | 0x80..) - tl * 0x0101..,
    // bit 7 of a byte of y says (x & 127) >= tl; the verdict is y & x for t >= 128 and y | x below.
    const int cj_lo = a.bin_lo / CB, cj_hi = (a.bin_hi + CB - 1) / CB;      // chunks that hold bins of the range window
    uint32_t cm[NCH];                                                       // candidate bits of the lane, chunk by chunk
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      cm[j] = 0u;
      if (j >= cj_hi) break;
      if (j < cj_lo) continue;
      const int dj = DJ(j), LB = 4 * dj;                                    // bytes (bins) of the lane in this chunk
      const int pos = j * CB + lane * LB;
      uint32_t cmask = 0;                                                   // bit per bin of the lane (LB <= 32)
#pragma unroll
      for (int h = 0; h < D / 2; h++) {
        if (2 * h >= dj) break;
        int t = a.thr_i;
        if (PRE) {
          const uint32_t* pq = P4 + (pos >> 2) + 2 * h;                     // quad 2 H of this 8-bin block
          const uint32_t slb = (pq[a.pa1] - pq[a.pa0]) + (pq[a.pb1] - pq[a.pb0]);
          const float f = __builtin_amdgcn_sqrtf((float)slb * a.kappa_lb);  // <= sqrt(kappa S_lb): kappa_lb carries the slack
          t = max(t, (int)f);
        }
        t = min(t, 255);                                                     // (a threshold above 255 lets 255 through: harmless, the
                                                                             //  list is decided exactly; thr_i = 256 empties the window on the host)
        const uint32_t tl = (uint32_t)(t & 0x7f);
        const uint32_t lo4 = __builtin_amdgcn_perm(tl, tl, 0u);               // the byte in all four places
        const uint32_t nhi = (t & 0x80) ? 0u : 0xffffffffu;
        const uint32_t x0 = cur[j][2 * h], x1 = cur[j][2 * h + 1];
        const uint32_t y0 = (x0 | 0x80808080u) - lo4, y1 = (x1 | 0x80808080u) - lo4;
        const uint32_t ge0 = (y0 & x0) | ((y0 | x0) & nhi);                  // bit 7 of every byte: byte >= t
        const uint32_t ge1 = (y1 & x1) | ((y1 | x1) & nhi);
        // gather the eight verdict bits: byte k of z holds dword 0's verdict at bit 0 and dword 1's at bit 4, and the dot
        // product of z's bytes with (1, 2, 4, 8) is the mask (one full-rate v_dot4 instead of a 32-bit multiply)
        const uint32_t z = ((ge0 >> 7) & 0x01010101u) | ((ge1 >> 3) & 0x10101010u);
        const uint32_t m8 = __builtin_amdgcn_udot4(z, 0x08040201u, 0u, false);
        cmask |= m8 << (8 * h);
      }
      if (a.bin_lo > j * CB || a.bin_hi < j * CB + 64 * LB) {               // range window: bins [bin_lo, bin_hi) of this lane's LB
        const int lo = min(LB, max(0, a.bin_lo - pos)), hi = min(LB, max(0, a.bin_hi - pos));   // (chunks inside the window skip this)
        const uint32_t win = hi > lo ? ((hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u)) : 0u;
        cmask &= win;
      }
      cm[j] = cmask;
    }
    CFAR_T(1);
    after_swar();                                                           // (the rows kernel moves the NEXT row's pieces into `cur` here)
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      if (j >= cj_hi) break;
      if (j < cj_lo) continue;
      const int pos = j * CB + lane * 4 * DJ(j);
      // the chunk's candidates -> list, behind the carried remainder, in bin order (lane, bit).  STAGED (cacfar_cols_kernel): the
      // list is shorter than a chunk + the carry, so that eight wavefronts share a CU's LDS with two 16-row tiles; a chunk whose
      // candidates would not fit goes in two halves of 32 lanes (<= 1024 bins + 127 carried <= kCfarColsList; the pre-filter
      // leaves ~100 candidates per row, so this is the exception)
      uint32_t m = cm[j];
      const int pc = __popc(m);
      const int incl = wave_incl_scan_i32(pc);
      const int tot = __builtin_amdgcn_readlane(incl, 63);
      const int low = STAGED ? __builtin_amdgcn_readlane(incl, 31) : 0;     // candidates of lanes 0 .. 31
      const int halves = (STAGED && C + tot > a.list_cap) ? 2 : 1;
      for (int hh = 0; hh < halves; hh++) {
        {
          const bool mine = halves == 1 || (lane >> 5) == hh;
          int off = C + incl - pc - (hh == 1 ? low : 0);
          if (mine)
            while (m) {
              list[off++] = (unsigned short)(pos + __ffs((int)m) - 1);
              m &= m - 1u;
            }
          C += halves == 1 ? tot : (hh == 0 ? low : tot - low);
        }
        wave_sync();
        CFAR_T(2);
#ifdef CFEAR_CFAR_TIMING
        ctot += C;
#endif
        int k0 = 0;
        for (; k0 + 128 <= C; k0 += 128) round2(k0, 128);
        if (k0 > 0) {                                                       // carry the remainder (< 128) to the front
          const int rem = C - k0;
          wave_sync();
          const unsigned short tmp0 = lane < rem ? list[k0 + lane] : (unsigned short)0;
          const unsigned short tmp1 = lane + 64 < rem ? list[k0 + 64 + lane] : (unsigned short)0;
          wave_sync();
          if (lane < rem) list[lane] = tmp0;
          if (lane + 64 < rem) list[64 + lane] = tmp1;
          C = rem;
          wave_sync();
        }
#ifdef CFEAR_CFAR_TIMING
        ctot -= C;
#endif
        CFAR_T(3);
      }
    }
    if (C > 64) round2(0, C);
    else if (C > 0) round(0, C);
    CFAR_T(3);
    // ---- D ------------------------------------------------------------------------------------------------------
    if (KEYS) {
      if (lane == 0) { a.row_cnt[2 * grow] = ndet; a.row_cnt[2 * grow + 1] = 0; }
    } else {
      wave_sync();
      int total = 0;
      for (int w0 = 0; w0 < a.words; w0 += 64) {
        const int wd = w0 + lane;
        if (wd < a.words) {
          unsigned long long bits = 0ull;
          if (2 * wd < colsp / 32) bits = (unsigned long long)det32[2 * wd];
          if (2 * wd + 1 < colsp / 32) bits |= (unsigned long long)det32[2 * wd + 1] << 32;
          a.det_bits[grow * a.words + wd] = bits;
          total += __popcll(bits);
        }
      }
      total = wave_sum_i32(total);
      if (lane == 0) a.det_count[grow] = total;
    }
    wave_sync();                                                            // the next row's writes stay behind this row's reads
    CFAR_T(4);
#ifdef CFEAR_CFAR_TIMING
    if (lane == 0 && (grow % 20011) == 0)
      printf("cfar row %lld: prefix %lld | thresholds+swar %lld | list %lld | rounds %lld (%d rounds, %d candidates) | write %lld\n", grow,
             tq[0], tq[1], tq[2], tq[3], nrounds, ctot, tq[4]);
#endif
}

template <int D, int NCH, int DL, bool KEYS, bool PRE>
__global__ __launch_bounds__(256) void cacfar_rows_kernel(const CfarArgs a) {
  constexpr int CB = 256 * D;                                                // bins per chunk (all but a shorter last one)
  auto DJ = [](int j) { return (DL != D && j == NCH - 1) ? DL : D; };        // dwords per lane of chunk j (folds after unrolling)
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2), aligned(4)));
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* lut = (uint32_t*)smem;
  lut[threadIdx.x] = a.lut[threadIdx.x];
  __syncthreads();
  const int colsp = a.colsp;
  uint8_t* wbase = smem + 1024 + (size_t)wave * cfar_wave_lds(colsp, a.pad_lo, a.pad_hi, KEYS, CB);   // (the list holds a full chunk)
  uint32_t* P4 = (uint32_t*)wbase + a.pad_lo;                                // P4[i] = sum_{q < 4 i} I_q^2, i in [-pad_lo, colsp / 4 + pad_hi]
  uint8_t* raw = wbase + (((size_t)(a.pad_lo + colsp / 4 + 1 + a.pad_hi) * 4 + 15) & ~(size_t)15);   // the row itself
  uint32_t* det32 = (uint32_t*)(raw + colsp + 16);                           // detections, bit per bin (bitmap output)
  unsigned short* list = (unsigned short*)(raw + colsp + 16 + (KEYS ? 0 : colsp / 8));
  for (int i = lane; i < a.pad_lo; i += 64) P4[-1 - i] = 0u;
  const int nch = DL != D ? NCH : colsp / CB;
  const long long step = (long long)gridDim.x * kRowsPerBlock;
  long long grow = (long long)blockIdx.x * kRowsPerBlock + wave;
  // (image, row) of the current and of the next row walk along with grow: no 64-bit division per row
  const int step_b = (int)(step / a.rows), step_r = (int)(step - (long long)step_b * a.rows);
  int cb = (int)(grow / a.rows), cr = (int)(grow - (long long)cb * a.rows);
  auto row_ptr = [&](int b, int r) -> const uint8_t* { return a.polar + (long long)b * a.batch_stride + (long long)r * a.stride; };
  // Rows are read in 16-byte pieces wherever they start on a 4-byte boundary (global_load_dwordx4 asks for no more).  A row whose
  // length is not a multiple of 16 (Oxford's native 3768 bins) ends inside its last piece: that piece is read whole where it ends
  // inside the image (cfear_cfar_row_direct, row_pieces.hpp: every row but the image's last, and with a stride below 16 bytes not
  // the rows just before it either) and the bytes beyond the row are cleared in registers (mask_tail), as the byte-wise copy
  // below leaves them.  Only rows on odd addresses and those last rows of a ragged image are copied into LDS byte by byte,
  // zero-padded, and take their pieces from there (no prefetch).  (Until round 6 every ragged or 8-byte-aligned row took
  // the byte copy: 1.42 instead of 0.43 ms per 512 sweeps of 3768 bins.)
  const bool ragged = (a.cols & 15) != 0;
  auto is_direct = [&](const uint8_t* p, const int row) -> bool {
    return cfear_cfar_row_direct((unsigned)((uintptr_t)p & 3), row, a.rows, a.stride, a.need_cols);
  };
  // a lane's LB bytes of a chunk: 16-byte pieces where LB is a multiple of 16 (D = 4, 8), 8-byte pieces otherwise (D = 6:
  // 24 lane is only 8-byte aligned, and ds_write_b128 wants 16)
  auto issue = [&](const uint8_t* p, uint32_t (&dst)[NCH][D]) {
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int dj = DJ(j);
      const int pos = j * CB + lane * 4 * dj;
      // (no zeroing here: the registers of the lanes beyond need_cols are zeroed ONCE before the row loop; the masked loads
      //  never write them, and the copies below move zeros)
      if (dj % 4 == 0) {
#pragma unroll
        for (int k = 0; k < D / 4; k++)
          if (4 * k < dj && pos + 16 * k < a.need_cols) {
            const u32x4 v = __builtin_nontemporal_load((const u32x4*)(p + pos + 16 * k));
            dst[j][4 * k] = v.x; dst[j][4 * k + 1] = v.y; dst[j][4 * k + 2] = v.z; dst[j][4 * k + 3] = v.w;
          }
      } else {
#pragma unroll
        for (int k = 0; k < D / 2; k++)
          if (2 * k < dj && pos + 8 * k < a.need_cols) {
            const u32x2 v = __builtin_nontemporal_load((const u32x2*)(p + pos + 8 * k));
            dst[j][2 * k] = v.x; dst[j][2 * k + 1] = v.y;
          }
      }
    }
  };
  auto wave_sync = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
  };
  uint32_t cur[NCH][D], nxt[NCH][D];
#pragma unroll
  for (int j = 0; j < NCH; j++)
#pragma unroll
    for (int d = 0; d < D; d++) { cur[j][d] = 0u; nxt[j][d] = 0u; }
  auto mask_tail = [&](uint32_t (&x)[NCH][D]) {             // ragged rows: nothing but zeros beyond bin cols - 1
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int dj = DJ(j);
      const int pos = j * CB + lane * 4 * dj;
#pragma unroll
      for (int d = 0; d < D; d++)
        if (d < dj) {
          const int rem = a.cols - (pos + 4 * d);
          x[j][d] &= rem >= 4 ? 0xffffffffu : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
        }
    }
  };
  bool direct_cur = grow < a.total_rows && is_direct(row_ptr(cb, cr), cr);
  if (direct_cur) issue(row_ptr(cb, cr), cur);
  // the first row's pieces are waited for HERE, so that inside the loop `cur` only ever comes from register copies: the
  // compiler cannot count conditional loads and would otherwise wait for vmcnt(0) -- the NEXT row's requests -- at the
  // first use of `cur` in every iteration
  __builtin_amdgcn_s_waitcnt(0);
  if (ragged && direct_cur) mask_tail(cur);
  const uint8_t* rowp = row_ptr(cb, cr);
  long long key_base = grow * (long long)a.kcap;
  const long long key_step = step * (long long)a.kcap;
  for (; grow < a.total_rows; grow += step, key_base += key_step) {
    cb += step_b; cr += step_r;
    if (cr >= a.rows) { cr -= a.rows; cb++; }
    if (!direct_cur) {
      for (int pos = lane * 16; pos < colsp; pos += 1024) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int q = pos; q < min(pos + 16, a.cols); q++) w[(q - pos) >> 2] |= (uint32_t)rowp[q] << (8 * (q & 3));
        *(uint4*)(raw + pos) = make_uint4(w[0], w[1], w[2], w[3]);
      }
      wave_sync();
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int dj = DJ(j);
        const int pos = j * CB + lane * 4 * dj;
#pragma unroll
        for (int d = 0; d < D; d++) cur[j][d] = (d < dj && pos < colsp) ? *(const uint32_t*)(raw + pos + 4 * d) : 0u;
      }
    }
    const bool have_next = grow + step < a.total_rows;
    const uint8_t* nextp = have_next ? row_ptr(cb, cr) : rowp;
    const bool next_direct = have_next && is_direct(nextp, cr);
    if (next_direct) issue(nextp, nxt);
    rowp = nextp;                                                           // (this row is in registers / LDS from here on)
    cfar_row<D, NCH, DL, KEYS, PRE, false>(a, lane, lut, P4, raw, det32, list, cur, nch, grow, key_base, [&]() {
      // The row's bytes are dead from here on (the rounds work from LDS): the NEXT row's pieces move into `cur` now, so that
      // the wait for them does not sit behind this row's key stores (vmcnt counts stores too: at the end of the row the copy
      // waited for the stores of the last round every time).
      if (next_direct) {
#pragma unroll
        for (int j = 0; j < NCH; j++)
#pragma unroll
          for (int d = 0; d < D; d++) cur[j][d] = nxt[j][d];
        if (ragged) mask_tail(cur);
      }
    });
    direct_cur = next_direct;
  }
}

// CA-CFAR on [range bins][azimuths] sweeps (the layout the non-Oxford drivers deliver, radar_driver.cpp:74-90): the decode
// (cv::rotate 90 deg counter-clockwise) fused into the filter -- ONE pass over the image instead of rotate (read + write)
// + cacfar_rows (read).  A workgroup takes a tile of 16 azimuths: the 16-byte pieces of the bins the arithmetic can reach
// (a.need_cols source rows) are transposed into LDS with v_perm_b32 on 4 x 4 byte blocks, the next tile's pieces are
// requested, and each wavefront runs cfar_row on four of the tile's rows straight from LDS.  Output row r holds source
// column a.rows - 1 - r.  a.rows / a.cols are the ROTATED image's (azimuths, bins); a.stride / a.batch_stride the SOURCE's.
// Key output only (the batched odometry).  Tiles of one image run on one XCD (blockIdx % 8): the eight tiles that share a
// 128-byte line of a source row meet in that XCD's L2.
constexpr int kCfarTile = 16;
constexpr int kCfarColsWaves = 8;             // 2 workgroups x 8 wavefronts per CU: two rows of a tile per wavefront, four wavefronts per
                                              // SIMD like cacfar_rows_kernel (4 x 4 rows: 0.364 ms per 512 sweeps, 6 x 3|2: 0.338)
constexpr int kCfarColsList = 1152;           // list entries per wavefront (cfar_row's STAGED append)
__host__ __device__ inline int cfar_cols_list_cap(int chunk_bins) { return chunk_bins + kCfarListSlack < kCfarColsList ? chunk_bins + kCfarListSlack : kCfarColsList; }
__host__ __device__ inline size_t cfar_cols_wave_lds(int colsp, int pad_lo, int pad_hi, int chunk_bins) {
  // P4 + list: the row lives in the tile
  return (((size_t)(pad_lo + colsp / 4 + 1 + pad_hi) * 4 + 15) & ~(size_t)15) + (((size_t)cfar_cols_list_cap(chunk_bins) * 2 + 15) & ~(size_t)15);
}
template <int D, int NCH, int DL, bool PRE>
__global__ __launch_bounds__(64 * kCfarColsWaves, 4) void cacfar_cols_kernel(const CfarArgs a, const int tiles) {
  constexpr int CB = 256 * D;
  auto DJ = [](int j) { return (DL != D && j == NCH - 1) ? DL : D; };
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  uint32_t* lut = (uint32_t*)smem;
  if (threadIdx.x < 256) lut[threadIdx.x] = a.lut[threadIdx.x];   // (256 entries: the workgroup has more threads than that)
  const int colsp = a.colsp, tstride = a.need_cols + 16;      // (the arithmetic never reads a row beyond need_cols: cfar_derive)
  uint8_t* tbase = smem + 1024;                               // [kCfarTile][tstride]: row lr = source column c0 + 15 - lr
  uint8_t* wbase = tbase + (((size_t)kCfarTile * tstride + 15) & ~(size_t)15) + (size_t)wave * cfar_cols_wave_lds(colsp, a.pad_lo, a.pad_hi, CB);
  uint32_t* P4 = (uint32_t*)wbase + a.pad_lo;
  unsigned short* list = (unsigned short*)(wbase + (((size_t)(a.pad_lo + colsp / 4 + 1 + a.pad_hi) * 4 + 15) & ~(size_t)15));
  for (int i = lane; i < a.pad_lo; i += 64) P4[-1 - i] = 0u;
  for (int i = threadIdx.x; i < kCfarTile * 4; i += 64 * kCfarColsWaves)     // the 16 bytes of padding behind every tile row
    *(uint32_t*)(tbase + (size_t)(i >> 2) * tstride + a.need_cols + 4 * (i & 3)) = 0u;
  const int nch = DL != D ? NCH : colsp / CB;
  const int xcd = blockIdx.x % kXcds, slot = blockIdx.x / kXcds, slots = gridDim.x / kXcds;
  const int nq = ((a.batch - xcd + kXcds - 1) / kXcds) * tiles;               // (image, tile) items of this workgroup's XCD
  auto locate = [&](const int q, int& b, int& tile) { const int im = q / tiles; b = im * kXcds + xcd; tile = q - im * tiles; };
  constexpr int GP = (NCH * CB / 4 + 64 * kCfarColsWaves - 1) / (64 * kCfarColsWaves);   // groups of 4 bins per thread (upper bound)
  const int need_groups = a.need_cols >> 2;
  uint32_t rw[GP][4][4];
  auto issue = [&](const int q) {                             // the pieces of item q: bins 4 g .. 4 g + 3, 16 source columns
    int b, tile;
    locate(q, b, tile);
    const uint8_t* src = a.polar + (long long)b * a.batch_stride + tile * kCfarTile;
#pragma unroll
    for (int p = 0; p < GP; p++) {
      const int g = (int)threadIdx.x + p * 64 * kCfarColsWaves;
      if (g < need_groups) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const u32x4 v = *(const u32x4*)(src + (size_t)(4 * g + i) * a.stride);
          rw[p][i][0] = v.x; rw[p][i][1] = v.y; rw[p][i][2] = v.z; rw[p][i][3] = v.w;
        }
      }
    }
  };
#pragma unroll
  for (int p = 0; p < GP; p++)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int d = 0; d < 4; d++) rw[p][i][d] = 0u;            // groups beyond need_cols stay zero
  int q = slot;
  if (q < nq) issue(q);
  while (q < nq) {
#pragma unroll
    for (int p = 0; p < GP; p++) {
      const int g = (int)threadIdx.x + p * 64 * kCfarColsWaves;
      if (g < need_groups) {
#pragma unroll
        for (int d = 0; d < 4; d++) {                         // source columns c0 + 4 d .. + 3 of bins 4 g .. 4 g + 3
          uint32_t colw[4];                                   // colw[e] = column c0 + 4 d + e as {bin 4g, +1, +2, +3}
          transpose4x4_bytes(rw[p][0][d], rw[p][1][d], rw[p][2][d], rw[p][3][d], colw);
#pragma unroll
          for (int e = 0; e < 4; e++) *(uint32_t*)(tbase + (size_t)(kCfarTile - 1 - (4 * d + e)) * tstride + 4 * g) = colw[e];
        }
      }
    }
    __syncthreads();
    int b, tile;
    locate(q, b, tile);
    const int qn = q + slots;
    if (qn < nq) issue(qn);
    const int r0 = a.rows - kCfarTile - tile * kCfarTile;     // output row of tile row 0
    for (int lr = wave; lr < kCfarTile; lr += kCfarColsWaves) {
      uint8_t* raw = tbase + (size_t)lr * tstride;
      uint32_t cur[NCH][D];
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        const int dj = DJ(j);
        const int pos = j * CB + lane * 4 * dj;
#pragma unroll
        for (int d = 0; d < D; d++) cur[j][d] = (d < dj && j < nch && pos + 4 * d < a.need_cols) ? *(const uint32_t*)(raw + pos + 4 * d) : 0u;
      }
      const long long grow = (long long)b * a.rows + (r0 + lr);
      cfar_row<D, NCH, DL, true, PRE, true>(a, lane, lut, P4, raw, nullptr, list, cur, nch, grow, grow * (long long)a.kcap, []() {});
    }
    __syncthreads();                                          // every row of the tile has been consumed
    q = qn;
  }
}

// lut[I] for cacfar_rows_kernel (step C of its comment): 0 when I does not pass the static threshold.
static bool cfar_build_lut(const CfarArgs& a, uint32_t* lut) {
  for (int i = 0; i < 256; i++) lut[i] = 0u;
  if (!(a.scaling > 0.0) || !std::isfinite(a.scaling) || a.window > 8192) return false;
  const double c = 2.0 * (double)a.window / a.scaling;
  for (int i = 0; i < 256; i++) {
    if (!((double)i > a.static_threshold)) continue;                        // cfar.cpp:45
    const double B = (double)(i * i) * c;
    if (!(B < 1.0e9)) return false;                                         // tiny scalings: the table would not fit 31 bits
    const double T = std::ceil(B - 1e-3), Tn = std::ceil(B + 1e-3);
    const uint32_t t = T < 0.0 ? 0u : (uint32_t)T;
    lut[i] = (t << 1) | (Tn > T ? 1u : 0u);
  }
  return true;
}

struct CfarCloudArgs {
  const uint8_t* polar;
  int rows, cols, stride;
  long long batch_stride;
  const unsigned long long* det_bits;
  const int32_t* det_count;
  int words;
  const double* cos_t;
  const double* sin_t;
  double range_res;
  float* xyzi;
  int32_t* n_points;
  int cap_points;
  uint8_t* det_mask;
};

// Compaction in (row, bin) order.  grid = (image, kCfarCloudSplit row slices): every workgroup scans all row counts (cheap)
// and emits the rows of its slice, one wavefront per row: lane w takes word w of the row's detection bitmap, a wave
// scan of the popcounts places the words, and each lane walks the set bits of its own word.  (The first version gave one
// workgroup a whole image and walked every 64-bin word of every row in turn: 1.5 ms per batch whatever its size.)
__global__ __launch_bounds__(256) void cacfar_cloud_kernel(const CfarCloudArgs a) {
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
    const int v = r < a.rows ? a.det_count[(long long)b * a.rows + r] : 0;
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
  // One wavefront per row.  Lane w takes word w of the row's detection bitmap and writes the bins of its set bits into a
  // list in LDS (a wave scan of the popcounts places them); the list is then turned into points one detection per lane,
  // so the intensity gathers of a row are ONE memory round trip however the detections cluster (the form before walked
  // the set bits of its word with a dependent gather per step).  The next row's bitmap words are loaded meanwhile.
  unsigned short* dlist = (unsigned short*)(row_off + a.rows + 1) + (size_t)wave * 64 * 64;   // [<= 64 words x 64 bits]
  auto load_bits = [&](int rr, int w0) -> unsigned long long {
    const int wd = w0 + lane;
    return (rr < rend && wd < a.words) ? a.det_bits[((long long)b * a.rows + rr) * a.words + wd] : 0ull;
  };
  unsigned long long nxt = load_bits(rbeg + wave, 0);
  for (int r = rbeg + wave; r < rend; r += 4) {
    const double cos_t = a.cos_t[r], sin_t = a.sin_t[r];
    int base = row_off[r];
    for (int w0 = 0; w0 < a.words; w0 += 64) {                              // cols <= 8192: at most two rounds
      const int wd = w0 + lane;
      unsigned long long bits = nxt;
      nxt = w0 + 64 < a.words ? load_bits(r, w0 + 64) : load_bits(r + 4, 0);
      if (a.det_mask && wd < a.words)
        for (int j = 0; j < 64 && wd * 64 + j < a.cols; j++)
          a.det_mask[((long long)b * a.rows + r) * a.cols + wd * 64 + j] = (uint8_t)((bits >> j) & 1ull);
      const int pc = __popcll(bits);
      const int incl = wave_incl_scan_i32(pc);
      const int n = __builtin_amdgcn_readlane(incl, 63);
      int off = incl - pc;
      while (bits) {
        dlist[off++] = (unsigned short)(wd * 64 + __ffsll((long long)bits) - 1);
        bits &= bits - 1;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane, idx = base + j;
        if (j < n && idx < a.cap_points) {
          const int bin = dlist[j];
          const double range = a.range_res * (double)bin;
          float4 p;
          p.x = (float)(range * cos_t);                                       // cfar.cpp:63-65
          p.y = (float)(range * sin_t);
          p.z = 0.f;
          p.w = (float)img[(long long)r * a.stride + bin];
          ((float4*)a.xyzi)[(long long)b * a.cap_points + idx] = p;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      base += n;
    }
  }
}

}  // namespace

// The kernel arguments that follow from the filter's parameters alone (rows = azimuths, cols = bins of the ROTATED image);
// D / DL / nch = the chunk geometry (cacfar_rows_kernel's template arguments).
static void cfar_derive(CfarArgs& a, const cfear_cacfar_params* par, int rows, int cols, int& D, int& DL, int& nch) {
  a.rows = rows; a.cols = cols;
  a.window = par->window_size; a.guard = par->nb_guard_cells;
  const double false_alarm_rate_ = (double)par->false_alarm_rate;
  const double N = par->window_size * 2;                                     // cfar.cpp:32
  a.scaling = N * (std::pow(false_alarm_rate_, -1. / N) - 1.);               // cfar.cpp:12-16
  a.range_res = (double)par->range_res;
  a.static_threshold = (double)par->z_min;
  a.min_distance = (double)par->min_distance;
  a.max_distance = par->max_distance;
  {
    // the candidate pre-test in integers.  intensity > static_threshold for integer intensities: the smallest passing value;
    // range > min_distance && range < max_distance (cfar.cpp:43-45, range = range_res * bin in double): the bin interval,
    // found with the reference's own expression
    const double st = a.static_threshold;
    a.thr_i = st < 0.0 ? 0 : (st >= 255.0 ? 256 : (int)std::floor(st) + 1);
    int lo = 0, hi = cols;
    while (lo < cols && !(a.range_res * (double)lo > a.min_distance)) lo++;
    while (hi > 0 && !(a.range_res * (double)(hi - 1) < a.max_distance)) hi--;
    a.bin_lo = lo; a.bin_hi = hi;
    if (a.thr_i >= 256 || hi <= lo) a.bin_hi = a.bin_lo = 0;                  // nothing passes the static threshold / the range window
    // bins the arithmetic of the bins in [bin_lo, bin_hi) can reach
    const long long reach = a.bin_hi > 0 ? std::min<long long>(cols, (long long)a.bin_hi - 1 + a.guard + a.window) : 0;
    a.need_cols = (int)((reach + 15) / 16 * 16);
    a.lut_ok = cfar_build_lut(a, a.lut) ? 1 : 0;
    // lower-bound pre-filter: the aligned quads inside the windows of every bin of an 8-bin block
    auto floor_div = [](int x, int y) { return x >= 0 ? x / y : -((-x + y - 1) / y); };
    auto ceil_div = [&](int x, int y) { return -floor_div(-x, y); };
    a.pa0 = ceil_div(7 - a.guard - a.window, 4); a.pa1 = floor_div(-a.guard, 4);
    a.pb0 = ceil_div(7 + a.guard, 4); a.pb1 = floor_div(a.guard + a.window, 4);
    if (a.pa1 < a.pa0) a.pa1 = a.pa0;
    if (a.pb1 < a.pb0) a.pb1 = a.pb0;
    a.pre_on = a.lut_ok && a.guard + a.window <= 1024 && (a.pa1 > a.pa0 || a.pb1 > a.pb0);
    if (!a.pre_on) a.pa0 = a.pa1 = a.pb0 = a.pb1 = 0;
    a.pad_lo = a.pre_on ? (std::max(0, -a.pa0) + 3) / 4 * 4 : 0;
    a.pad_hi = a.pre_on ? std::max(0, a.pb1) + 2 : 0;
    a.kappa_lb = (float)(a.scaling / (2.0 * (double)a.window) * (1.0 - 3e-5));
  }
  // chunk geometry: D dwords per lane and chunk.  Per-chunk overhead ~ 60 wave instructions, per dword of a lane ~ 25:
  // the D in {4, 6, 8} with the cheapest cover of the reachable bins (without the pre-filter only D = 4 is built)
  D = 4; DL = 4; nch = std::max(1, (a.need_cols + 1023) / 1024);
  if (a.pre_on) {
    // measured on the Kvarntorp rows: ~10 us per chunk and ~9 us per dword of a lane (per 204 800 rows)
    auto cost = [](int n, int d, int dl) { return (long long)n * 10 + (long long)((n - 1) * d + dl) * 9; };
    long long best = cost(nch, 4, 4);
    for (int d : {6, 8}) {
      const int n = std::max(1, (a.need_cols + 256 * d - 1) / (256 * d));
      if (cost(n, d, d) < best) { best = cost(n, d, d); D = d; DL = d; nch = n; }
      if (n == 2) {                                        // two chunks: the second may be two dwords shorter.  (Shorter still --
        const int dl = d - 2;                              // 6 | 2, 8 | 2, 8 | 4 -- never costs LESS than a geometry tried before it:
                                                           // 4 x 2, 6 | 4 and 6 x 2 cover the same bins at the same cost, so those
                                                           // were never selected and are not built; tests/test_cacfar_plan_cpu.py)
        if (256 * d + 256 * dl >= a.need_cols && cost(2, d, dl) < best) { best = cost(2, d, dl); D = d; DL = dl; nch = 2; }
      }
    }
  }
  a.colsp = (nch - 1) * 256 * D + 256 * DL;
}

static size_t cfar_cols_lds(const CfarArgs& a, int D) {
  return 1024 + (size_t)kCfarTile * ((size_t)a.need_cols + 16) + (size_t)kCfarColsWaves * cfar_cols_wave_lds(a.colsp, a.pad_lo, a.pad_hi, 256 * D);
}

// ---- the dispatch tables: every CA-CFAR kernel that is built, and nothing else launches one ---------------------------------
// cfear_cacfar_plan (cfear_hip.h) documents the indices; cfar_rows_index / cfar_cols_index return -1 for a geometry that is
// not built (cfar_derive selects none: tests/test_cacfar_plan_cpu.py sweeps it).
using CfarRowsFn = void (*)(const CfarArgs);
using CfarColsFn = void (*)(const CfarArgs, int);
constexpr int kCfarRowsEntries = 20, kCfarColsEntries = 6;
static const CfarRowsFn kCfarRowsTable[kCfarRowsEntries] = {
    // D = 4: [wide][keys][pre]
    cacfar_rows_kernel<4, 4, 4, false, false>, cacfar_rows_kernel<4, 4, 4, false, true>,
    cacfar_rows_kernel<4, 4, 4, true, false>, cacfar_rows_kernel<4, 4, 4, true, true>,
    cacfar_rows_kernel<4, 8, 4, false, false>, cacfar_rows_kernel<4, 8, 4, false, true>,
    cacfar_rows_kernel<4, 8, 4, true, false>, cacfar_rows_kernel<4, 8, 4, true, true>,
    // D = 6, whole chunks: [nch > 2][keys]; DL = 4: [keys]
    cacfar_rows_kernel<6, 2, 6, false, true>, cacfar_rows_kernel<6, 2, 6, true, true>,
    cacfar_rows_kernel<6, 6, 6, false, true>, cacfar_rows_kernel<6, 6, 6, true, true>,
    cacfar_rows_kernel<6, 2, 4, false, true>, cacfar_rows_kernel<6, 2, 4, true, true>,
    // D = 8, whole chunks: [nch > 2][keys]; DL = 6: [keys]
    cacfar_rows_kernel<8, 2, 8, false, true>, cacfar_rows_kernel<8, 2, 8, true, true>,
    cacfar_rows_kernel<8, 4, 8, false, true>, cacfar_rows_kernel<8, 4, 8, true, true>,
    cacfar_rows_kernel<8, 2, 6, false, true>, cacfar_rows_kernel<8, 2, 6, true, true>};
static const CfarColsFn kCfarColsTable[kCfarColsEntries] = {
    cacfar_cols_kernel<4, 4, 4, false>, cacfar_cols_kernel<4, 4, 4, true>,
    cacfar_cols_kernel<6, 2, 4, true>, cacfar_cols_kernel<6, 2, 6, true>,       // (colsp <= 4096: at most two chunks of 1536)
    cacfar_cols_kernel<8, 2, 6, true>, cacfar_cols_kernel<8, 2, 8, true>};

static int cfar_rows_index(int D, int DL, int nch, bool keys, bool pre) {
  const int k = keys ? 1 : 0;
  if (D == 4) return DL == 4 && nch <= 8 ? (nch > 4 ? 4 : 0) + 2 * k + (pre ? 1 : 0) : -1;
  if (!pre) return -1;                                       // (without the pre-filter only D = 4 is built)
  if (D == 6) return DL == 6 ? (nch <= 6 ? 8 + (nch > 2 ? 2 : 0) + k : -1) : (DL == 4 && nch == 2 ? 12 + k : -1);
  if (D == 8) return DL == 8 ? (nch <= 4 ? 14 + (nch > 2 ? 2 : 0) + k : -1) : (DL == 6 && nch == 2 ? 18 + k : -1);
  return -1;
}
static int cfar_cols_index(int D, int DL, int nch, bool pre) {
  if (D == 4) return DL == 4 && nch <= 4 ? (pre ? 1 : 0) : -1;
  if (!pre || nch > 2 || (DL != D && nch != 2)) return -1;
  if (D == 6) return DL == 4 ? 2 : (DL == 6 ? 3 : -1);
  if (D == 8) return DL == 6 ? 4 : (DL == 8 ? 5 : -1);
  return -1;
}

// The one selection: everything cfear_cacfar_device launches follows from the plan this fills (and `a`, the kernel arguments
// that follow from the parameters).  desc as the caller hands it over (cols_route: the [range bins][azimuths] SOURCE images);
// base_mod16 = the image address modulo 16.
static void cfar_plan(CfarArgs& a, const cfear_polar_desc* desc, const cfear_cacfar_params* par, bool keys, bool cols_route,
                      unsigned base_mod16, struct cfear_cacfar_plan& p) {
  const int rows = cols_route ? desc->cols : desc->rows, cols = cols_route ? desc->rows : desc->cols, batch = desc->batch;
  int D, DL, nch;
  cfar_derive(a, par, rows, cols, D, DL, nch);
  memset(&p, 0, sizeof(p));
  p.D = D; p.DL = DL; p.nch = nch;
  p.pre_on = a.pre_on; p.lut_ok = a.lut_ok;
  p.need_cols = a.need_cols; p.colsp = a.colsp; p.bin_lo = a.bin_lo; p.bin_hi = a.bin_hi;
  p.pad_lo = a.pad_lo; p.pad_hi = a.pad_hi;
  p.keys = keys ? 1 : 0; p.cols_route = cols_route ? 1 : 0;
  p.total_rows = (int64_t)batch * rows;
  const int64_t batch_stride = batch > 1 ? desc->batch_stride : (int64_t)desc->rows * desc->stride;
  if (cols_route) {
    p.table_index = cfar_cols_index(D, DL, nch, a.pre_on != 0);
    p.lds_bytes = (int64_t)cfar_cols_lds(a, D);
    const bool geometry = desc->cols % kCfarTile == 0 && desc->rows % 16 == 0 && desc->stride % 16 == 0 && base_mod16 == 0 &&
                          !(batch > 1 && desc->batch_stride % 16 != 0) && (int64_t)desc->rows * desc->stride < ((int64_t)1 << 31);
    p.cols_supported = geometry && p.table_index >= 0 && a.colsp <= 4096 && p.lds_bytes <= 160 * 1024 - 256;
    return;
  }
  p.wide = D == 4 && nch > 4;
  p.table_index = cfar_rows_index(D, DL, nch, keys, a.pre_on != 0);
  p.lds_bytes = (int64_t)(1024 + (size_t)kRowsPerBlock * cfar_wave_lds(a.colsp, a.pad_lo, a.pad_hi, keys, 256 * D));
  // rows read in 16-byte pieces: the kernel's own test (cfear_cfar_row_direct), image by image
  int64_t inside = 0;                                        // rows of an image whose last piece ends inside it
  for (int r = 0; r < rows; r++) inside += cfear_cfar_row_direct(0u, r, rows, desc->stride, a.need_cols) ? 1 : 0;
  if ((batch_stride & 3) == 0) p.piece_rows = (base_mod16 & 3) == 0 ? inside * batch : 0;
  else
    for (int b = 0; b < batch; b++) p.piece_rows += (((int64_t)base_mod16 + (int64_t)b * batch_stride) & 3) == 0 ? inside : 0;
}

static int cfar_check_params(const cfear_cacfar_params* par) {
  return par && par->window_size >= 1 && par->nb_guard_cells >= 0 && par->range_res > 0.f;
}

extern "C" int cfear_cacfar_plan(const cfear_polar_desc* desc, const cfear_cacfar_params* par, int32_t flags,
                                 struct cfear_cacfar_plan* out) {
  if (!desc || !par || !out || (flags & ~(CFEAR_ROWKEYS_BINS_MAJOR | CFEAR_CACFAR_PLAN_KEYS | (15 << 12))) != 0)
    return CFEAR_ERR_INVALID_ARGUMENT;
  const bool cols_route = (flags & CFEAR_ROWKEYS_BINS_MAJOR) != 0;
  if (polar_desc_fault(desc, cols_route) != DescFault::kNone || !cfar_check_params(par)) return CFEAR_ERR_INVALID_ARGUMENT;
  CfarArgs a;
  memset(&a, 0, sizeof(a));
  cfar_plan(a, desc, par, cols_route || (flags & CFEAR_CACFAR_PLAN_KEYS) != 0, cols_route, (unsigned)(flags >> 12) & 15u, *out);
  return CFEAR_OK;
}

// [range bins][azimuths] sources through cacfar_cols_kernel: sd = the SOURCE images (rows = bins, cols = azimuths).
bool cfear_cacfar_cols_supported(const uint8_t* d_src, const cfear_polar_desc* sd, const cfear_cacfar_params* par) {
  CfarArgs a;
  memset(&a, 0, sizeof(a));
  struct cfear_cacfar_plan p;
  cfar_plan(a, sd, par, true, true, (unsigned)((uintptr_t)d_src & 15), p);
  return p.cols_supported != 0;
}

// Device-side CA-CFAR entry (also used by the odometry pipeline).  With `fused` the rows kernel leaves per-row key lists for
// surface_prep_kernel (cfear_cacfar_fused, common.hpp) and no cloud is built here; fused->bins_major: desc describes the
// [range bins][azimuths] SOURCE images and the decode is fused into the filter (cacfar_cols_kernel).
int cfear_cacfar_device(cfear_ctx* ctx, const uint8_t* d_polar, const cfear_polar_desc* desc,
                        const cfear_cacfar_params* par, float* d_xyzi, int32_t* d_n_points,
                        int32_t cap_points, uint8_t* d_det_mask, const cfear_cacfar_fused* fused) {
  const bool keys = fused && fused->row_keys;
  const bool cols_route = keys && fused->bins_major;
  CfarArgs a;
  memset(&a, 0, sizeof(a));
  struct cfear_cacfar_plan plan;
  cfar_plan(a, desc, par, keys, cols_route, (unsigned)((uintptr_t)d_polar & 15), plan);
  if (cols_route && !plan.cols_supported)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "fused CA-CFAR decode: unsupported image geometry");
  if (plan.table_index < 0 || plan.table_index >= (cols_route ? kCfarColsEntries : kCfarRowsEntries))   // a missing kernel is an error
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "CA-CFAR: no kernel for D = %d, DL = %d, %d chunks", plan.D, plan.DL, plan.nch);
  const int rows = cols_route ? desc->cols : desc->rows, cols = cols_route ? desc->rows : desc->cols, batch = desc->batch;
  const int words = (cols + 63) / 64;
  const int D = plan.D;
  a.polar = d_polar; a.stride = desc->stride; a.batch = batch;
  a.batch_stride = batch > 1 ? desc->batch_stride : (int64_t)desc->rows * desc->stride;
  a.total_rows = (long long)batch * rows;
  a.words = words;
  if (keys) {
    a.row_keys = fused->row_keys; a.row_cnt = fused->row_cnt; a.kcap = fused->kcap;
  } else {
    size_t bits_bytes = (size_t)batch * rows * words * 8, cnt_bytes = (size_t)batch * rows * 4;
    char* ws = (char*)cfear_workspace(ctx, kWsFilterRows, bits_bytes + cnt_bytes + 256);
    if (!ws) return cfear_set_error(ctx, CFEAR_ERR_HIP, "workspace allocation failed");
    a.det_bits = (unsigned long long*)ws;
    a.det_count = (int32_t*)(ws + (bits_bytes + 255) / 256 * 256);
  }
  a.list_cap = cols_route ? cfar_cols_list_cap(256 * D) : 256 * D + kCfarListSlack;
  if (cols_route) {
    const CfarColsFn fn = kCfarColsTable[plan.table_index];
    const size_t lds = (size_t)plan.lds_bytes;
    { const int rc_lds = cfear_allow_lds(ctx, (const void*)fn, lds); if (rc_lds != CFEAR_OK) return rc_lds; }
    const int tiles = rows / kCfarTile;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, 160 * 1024 / lds));
    const int slots = xcd_grid_slots(tiles, batch, ctx->n_cu, per_cu);
    ProfScope ps(ctx, "cacfar_cols");
    hipLaunchKernelGGL(fn, dim3((unsigned)(slots * kXcds)), dim3(64 * kCfarColsWaves), lds, ctx->stream, a, tiles);
    CFEAR_HIP_CHECK(ctx, hipGetLastError());
    return CFEAR_OK;
  }
  {
    const CfarRowsFn fn = kCfarRowsTable[plan.table_index];
    const size_t rows_lds = (size_t)plan.lds_bytes;
    if (rows_lds > 64 * 1024)
      { const int rc_lds = cfear_allow_lds(ctx, (const void*)fn, rows_lds); if (rc_lds != CFEAR_OK) return rc_lds; }
    // persistent wavefronts: as many workgroups as the chip holds at this LDS footprint (160 KiB per CU)
    const int n_cu = ctx->n_cu;
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, 160 * 1024 / rows_lds));
    const long long want = (a.total_rows + kRowsPerBlock - 1) / kRowsPerBlock;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(want, (long long)n_cu * per_cu));
    ProfScope ps(ctx, "cacfar_rows");
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), rows_lds, ctx->stream, a);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  if (keys) return CFEAR_OK;
  double *d_cos = nullptr, *d_sin = nullptr;
  int rc = cfear_trig_tables(ctx, rows, &d_cos, &d_sin);
  if (rc != CFEAR_OK) return rc;
  CfarCloudArgs c;
  c.polar = d_polar; c.rows = rows; c.cols = cols; c.stride = desc->stride; c.batch_stride = a.batch_stride;
  c.det_bits = a.det_bits; c.det_count = a.det_count; c.words = words;
  c.cos_t = d_cos; c.sin_t = d_sin; c.range_res = a.range_res;
  c.xyzi = d_xyzi; c.n_points = d_n_points; c.cap_points = cap_points; c.det_mask = d_det_mask;
  {
    ProfScope ps(ctx, "cacfar_cloud");
    hipLaunchKernelGGL(cacfar_cloud_kernel, dim3(batch, kCfarCloudSplit), dim3(256), (size_t)(rows + 1) * 4 + 4 * 64 * 64 * 2, ctx->stream, c);
  }
  CFEAR_HIP_CHECK(ctx, hipGetLastError());
  return CFEAR_OK;
}

extern "C" int cfear_filter_cacfar_rowkeys(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                           const cfear_cacfar_params* par, int32_t flags, uint32_t* row_keys,
                                           int32_t* row_counts, int32_t kcap) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!polar || !par || !row_keys || !row_counts) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  if ((flags & ~CFEAR_ROWKEYS_BINS_MAJOR) != 0) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "unknown flags");
  const bool bins_major = (flags & CFEAR_ROWKEYS_BINS_MAJOR) != 0;
  if (polar_desc_fault(desc, bins_major) != DescFault::kNone)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad polar descriptor");
  if (!cfar_check_params(par)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad CFAR parameters");
  if (kcap < 1) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "kcap must be >= 1");
  if (!cfear_is_device_ptr(polar) || !cfear_is_device_ptr(row_keys) || !cfear_is_device_ptr(row_counts))
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "images and outputs must be device memory");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  cfear_cacfar_fused fz;
  fz.row_keys = row_keys; fz.row_cnt = row_counts; fz.kcap = kcap; fz.bins_major = bins_major;
  return cfear_cacfar_device(ctx, polar, desc, par, nullptr, nullptr, 0, nullptr, &fz);
}

extern "C" int cfear_filter_cacfar(cfear_ctx* ctx, const uint8_t* polar, const cfear_polar_desc* desc,
                                   const cfear_cacfar_params* par, float* xyzi, int32_t* n_points,
                                   int32_t cap_points, uint8_t* det_mask) {
  if (!ctx) return CFEAR_ERR_INVALID_ARGUMENT;
  if (!polar || !par || !xyzi || !n_points || cap_points <= 0)
    return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "null argument");
  CFEAR_CHECK(check_desc(ctx, desc));
  if (!cfar_check_params(par)) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad CFAR parameters");
  CFEAR_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rows = desc->rows, cols = desc->cols, batch = desc->batch;
  HostStage st(ctx, kWsFilter);
  const uint8_t* d_polar;
  const cfear_polar_desc dd = st.images(d_polar, polar, *desc);
  float* d_xyzi;
  int32_t* d_np;
  uint8_t* d_mask = nullptr;
  st.out(d_xyzi, xyzi, (size_t)batch * cap_points * 16);
  st.out(d_np, n_points, (size_t)batch * 4);
  if (det_mask) st.out(d_mask, det_mask, (size_t)batch * rows * cols);
  CFEAR_CHECK(st.carve());
  CFEAR_CHECK(cfear_cacfar_device(ctx, d_polar, &dd, par, d_xyzi, d_np, cap_points, d_mask));
  CFEAR_CHECK(st.finish());
  if (st.any_host())
    for (int b = 0; b < batch; b++)
      if (n_points[b] > cap_points)
        return cfear_set_error(ctx, CFEAR_ERR_CAPACITY, "image %d: %d detections > cap_points %d", b, n_points[b], cap_points);
  return CFEAR_OK;
}
