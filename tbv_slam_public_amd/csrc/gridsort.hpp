// gridsort.hpp -- block-wide LDS sort of (grid cell, point index) pairs, shared by the kernels that
// replace a PCL voxel grid / kd-tree radius search with a sort-based uniform grid (surface.hip, coral.hip, p2p.hip),
// and the neighbour index coral.hip and p2p.hip build from the sorted keys (GridIndex, at the end).
#pragma once
#include "common.hpp"

constexpr int kGridSortThreads = 1024;
constexpr int kGridSortMaxPoints = 16384;        // 64-bit keys: 128 KiB of LDS
constexpr int kGridSortRadixMaxPoints = 8192;    // radix path: 2 x 32 KiB key buffers + 32 KiB counters

#if defined(__HIPCC__)
// Two-level variant for the common case (n <= 8192, no crowded grid row): a counting sort by grid ROW with LDS
// atomics, then every element finds its rank among the elements of its row.  With 1 m cells a row of two merged peak
// clouds holds ~80 points: ~80 LDS reads per element replace five radix passes.  The order is the unique order of the
// (cell, index) keys, so the result equals grid_sort_block's bit for bit.  cell_xy(i, ix, iy) -> column / row of point
// i (ix < dbx <= 65535, iy < dby <= 4096); rowcnt: dby + 1 uint32 of LDS outside the 128 KiB key region; red_i, red_m:
// 16 ints each.  Returns npad (like grid_sort_block), or 0 without having sorted when the variant does not apply.
constexpr int kGridRowSortMaxN = 8192;
template <typename CellXY>
__device__ int grid_sort_rows_block(uint8_t* smem, int n, int dbx, int dby, uint32_t* rowcnt, int* red_i, int* red_m,
                                    int max_row, CellXY cell_xy) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (n > kGridRowSortMaxN || dbx > 65535 || dby > 4096) return 0;
  unsigned long long* keys = (unsigned long long*)smem;            // [npad] result
  uint32_t* tmp = (uint32_t*)(smem + 64 * 1024);                    // [n] (ix << 13 | i), grouped by row
  unsigned short* rowid = (unsigned short*)(smem + 96 * 1024);      // [n] grid row of tmp[j]
  for (int y = tid; y <= dby; y += kGridSortThreads) rowcnt[y] = 0;
  __syncthreads();
  int cx[kGridRowSortMaxN / kGridSortThreads], cy[kGridRowSortMaxN / kGridSortThreads];
#pragma unroll
  for (int q = 0; q < kGridRowSortMaxN / kGridSortThreads; q++) {
    const int i = tid + q * kGridSortThreads;
    cx[q] = cy[q] = 0;
    if (i < n) {
      cell_xy(i, cx[q], cy[q]);
      atomicAdd(&rowcnt[cy[q]], 1u);
    }
  }
  __syncthreads();
  bool ok;
  {                                                                 // exclusive scan over the rows + largest row
    const int per_t = (dby + kGridSortThreads) / kGridSortThreads;  // rows per thread (<= 5)
    const int y0 = tid * per_t;
    int tot = 0, mx = 0;
    for (int y = y0; y < min(dby, y0 + per_t); y++) { const int c = (int)rowcnt[y]; tot += c; mx = max(mx, c); }
    const int incl = wave_incl_scan_i32(tot);
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    if (lane == 63) red_i[wave] = incl;
    if (lane == 0) red_m[wave] = mx;
    __syncthreads();
    int run = incl - tot;
    for (int wv = 0; wv < wave; wv++) run += red_i[wv];
    int mxall = 0;
    for (int wv = 0; wv < 16; wv++) mxall = max(mxall, red_m[wv]);
    ok = mxall <= max_row;
    for (int y = y0; y < min(dby, y0 + per_t); y++) { const int c = (int)rowcnt[y]; rowcnt[y] = (uint32_t)run; run += c; }
    __syncthreads();
  }
  if (!ok) return 0;
#pragma unroll
  for (int q = 0; q < kGridRowSortMaxN / kGridSortThreads; q++) {
    const int i = tid + q * kGridSortThreads;
    if (i < n) {
      const uint32_t pos = atomicAdd(&rowcnt[cy[q]], 1u);           // afterwards rowcnt[y] = end of row y
      tmp[pos] = ((uint32_t)cx[q] << 13) | (uint32_t)i;
      rowid[pos] = (unsigned short)cy[q];
    }
  }
  __syncthreads();
  const int npad = (n + kGridSortThreads - 1) / kGridSortThreads * kGridSortThreads;
  for (int j = tid; j < npad; j += kGridSortThreads) {
    if (j >= n) { keys[j] = ~0ull; continue; }
    const int y = rowid[j];
    const int s = y > 0 ? (int)rowcnt[y - 1] : 0, e = (int)rowcnt[y];
    const uint32_t key = tmp[j];
    int rank = 0;
    for (int i = s; i < e; i++) rank += tmp[i] < key;
    keys[s + rank] = ((unsigned long long)((uint32_t)y * (uint32_t)dbx + (key >> 13)) << 32) | (key & 8191u);
  }
  __syncthreads();
  return max(npad, kGridSortThreads);
}

// Sorts the n points of a 1024-thread workgroup by (cell, index): cells ascending, points of a cell in input
// order (stable).  cell_of(i) -> uint32 cell id < n_cells.  On return smem holds npad (>= n, a multiple of
// 1024) 64-bit keys (cell << 32 | index), padding = ~0; thread t owns elements [t * npad/1024, ...).
// red_i: 16 ints of LDS outside the key region.  Returns npad.  Block-wide collective (ends with a barrier).
//   n <= 8192 and cell bits + index bits <= 32: packed 32-bit keys, stable LSD radix sort on the cell digits
//   (4 bits per pass, thread-contiguous chunks keep the input order, per-thread u16 digit counters);
//   otherwise: bitonic sort of the 64-bit keys.
// Which path grid_sort_block takes for n points in n_cells cells.  ib: index bits, 2^ib >= npad; vb: cell-index bits.
__device__ __forceinline__ bool grid_sort_is_radix(int n, long long n_cells, int& ib, int& vb) {
  int npad = (n + kGridSortThreads - 1) / kGridSortThreads * kGridSortThreads;
  if (npad < kGridSortThreads) npad = kGridSortThreads;
  ib = 10;
  while ((1 << ib) < npad) ib++;
  vb = 1;
  while (((long long)1 << vb) < n_cells) vb++;
  return (npad <= kGridSortRadixMaxPoints) && (vb + ib <= 32);
}

template <typename CellFn>
__device__ int grid_sort_block(uint8_t* smem, int n, long long n_cells, int* red_i, CellFn cell_of) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned long long* keys = (unsigned long long*)smem;
  int npad = (n + kGridSortThreads - 1) / kGridSortThreads * kGridSortThreads;   // radix path: any multiple of 1024
  if (npad < kGridSortThreads) npad = kGridSortThreads;
  int ib, vb;
  const bool radix = grid_sort_is_radix(n, n_cells, ib, vb);
  if (!radix) {                                            // the bitonic network needs a power of two
    npad = 1024;
    while (npad < n) npad <<= 1;
  }
  if (radix) {
    uint32_t* kA = (uint32_t*)smem;
    uint32_t* kB = kA + npad;
    unsigned short* cnt = (unsigned short*)(kB + npad);   // [16][1024]
    const int per = npad / kGridSortThreads;               // 1..8 consecutive elements per thread
    for (int i = tid; i < npad; i += kGridSortThreads) {
      uint32_t key = 0xFFFFFFFFu;
      if (i < n) key = (cell_of(i) << ib) | (uint32_t)i;
      kA[i] = key;
    }
    __syncthreads();
    uint32_t* src = kA;
    uint32_t* dst = kB;
    for (int shift = ib; shift < ib + vb; shift += 4) {
#pragma unroll
      for (int d = 0; d < 16; d++) cnt[d * kGridSortThreads + tid] = 0;
      for (int q = 0; q < per; q++) {
        const uint32_t dg = (src[tid * per + q] >> shift) & 15u;
        cnt[dg * kGridSortThreads + tid]++;
      }
      __syncthreads();
      // exclusive scan of the 16 x 1024 counters in (digit, thread) order: 16 consecutive per thread
      unsigned short local[16];
      int tot = 0;
#pragma unroll
      for (int q = 0; q < 16; q++) { local[q] = cnt[tid * 16 + q]; tot += local[q]; }
      const int inc = wave_incl_scan_i32(tot);
      if (lane == 63) red_i[wave] = inc;
      __syncthreads();
      int run = inc - tot;
      for (int wv = 0; wv < wave; wv++) run += red_i[wv];
#pragma unroll
      for (int q = 0; q < 16; q++) { cnt[tid * 16 + q] = (unsigned short)run; run += local[q]; }
      __syncthreads();
      for (int q = 0; q < per; q++) {
        const uint32_t key = src[tid * per + q];
        const uint32_t dg = (key >> shift) & 15u;
        const int pos = cnt[dg * kGridSortThreads + tid]++;
        dst[pos] = key;
      }
      __syncthreads();
      uint32_t* t = src; src = dst; dst = t;
    }
    // widen to the 64-bit (cell, index) form; registers bridge the overlap
    uint32_t mine32[kGridSortRadixMaxPoints / kGridSortThreads];
#pragma unroll
    for (int q = 0; q < kGridSortRadixMaxPoints / kGridSortThreads; q++) mine32[q] = (q < per) ? src[tid * per + q] : 0xFFFFFFFFu;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGridSortRadixMaxPoints / kGridSortThreads; q++)
      if (q < per) {
        // padding is what the stable sort left behind the n points, not the key value: with 2^ib points in 2^vb cells
        // and vb + ib = 32 the last point of the last cell has the all-ones key too
        const uint32_t key = mine32[q];
        keys[tid * per + q] = tid * per + q >= n ? ~0ull
                                                 : (((unsigned long long)(key >> ib)) << 32) | (key & ((1u << ib) - 1u));
      }
    __syncthreads();
  } else {
    // General path: bitonic sort of 64-bit (cell, index) keys.
    for (int i = tid; i < npad; i += kGridSortThreads) {
      unsigned long long key = ~0ull;
      if (i < n) key = ((unsigned long long)cell_of(i) << 32) | (unsigned)i;
      keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (npad >> 1); t += kGridSortThreads) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const bool asc = (lo & k) == 0;
          const unsigned long long a = keys[lo], b = keys[hi];
          if ((a > b) == asc) { keys[lo] = b; keys[hi] = a; }
        }
        __syncthreads();
      }
    }
  }
  return npad;
}

__device__ __forceinline__ int lower_bound_u32(const uint32_t* a, int lo, int hi, uint32_t key) {
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ int upper_bound_u32(const uint32_t* a, int lo, int hi, uint32_t key) {
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; }
  return lo;
}

// ---- The grid index of coral.hip and p2p.hip: what replaces a FLANN radius search over one cloud. -----------------------
// One 1024-thread workgroup sorts n <= 16384 points by (cell, index) and keeps, in its dynamic LDS:
//   [0, kGridRowbegOff)   the sort's keys, afterwards: cell_key [V] | cell_start [V + 1] | the sorted points (float4 [n],
//                         when they fit; else in the caller's global scratch) | occ, wpref (when they fit)
//   kGridRowbegOff        rowbeg [dby + 1]: the row sort's counters, afterwards the first occupied cell of every grid row
//                         (only without the bitmap)
//   kGridSmallOff         1 KiB of small reductions: float [4][16] (block_bbox_f32), int [16] at + 256 and + 320 (the sort
//                         and the builder; free once the index is built); the caller's own start at + 384
constexpr int kGridMaxRows = 4096;
constexpr int kGridPerThread = kGridSortMaxPoints / kGridSortThreads;
constexpr size_t kGridRowbegOff = (size_t)kGridSortMaxPoints * 8 + 16;
constexpr size_t kGridSmallOff = (kGridRowbegOff + (size_t)(kGridMaxRows + 1) * 4 + 15) / 16 * 16;
constexpr size_t kGridLdsTotal = kGridSmallOff + 1024;

// The bounding box of the workgroup's points from every thread's own minima and maxima: wave shuffles, 16 partials in
// LDS, then every thread reads them.  `barrier` is the one block barrier in between (__syncthreads, or a vote of the
// caller's that is one).
template <typename Barrier>
__device__ __forceinline__ void block_bbox_f32(uint8_t* smem, float& mnx, float& mxx, float& mny, float& mxy, Barrier barrier) {
  float (*red_f)[16] = (float (*)[16])(smem + kGridSmallOff);          // [4][16]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int o = 32; o > 0; o >>= 1) {
    mnx = fminf(mnx, __shfl_xor(mnx, o)); mxx = fmaxf(mxx, __shfl_xor(mxx, o));
    mny = fminf(mny, __shfl_xor(mny, o)); mxy = fmaxf(mxy, __shfl_xor(mxy, o));
  }
  if (lane == 0) { red_f[0][wave] = mnx; red_f[1][wave] = mxx; red_f[2][wave] = mny; red_f[3][wave] = mxy; }
  barrier();
  mnx = red_f[0][0]; mxx = red_f[1][0]; mny = red_f[2][0]; mxy = red_f[3][0];
  for (int wv = 1; wv < 16; wv++) {
    mnx = fminf(mnx, red_f[0][wv]); mxx = fmaxf(mxx, red_f[1][wv]);
    mny = fminf(mny, red_f[2][wv]); mxy = fmaxf(mxy, red_f[3][wv]);
  }
}

struct GridIndex {
  int V, dbx, dby;                      // occupied cells; grid columns and rows
  int path;                             // CFEAR_CORAL_PATH_* (cfear_hip.h): which sort, home of the points and lookup
  bool spt_in_lds, bitmap;
  float4* spt;                          // the sorted points: LDS (spt_in_lds) or the caller's scratch
  const uint32_t* cell_key;             // [V] occupied cells, ascending
  const int32_t* cell_start;            // [V + 1] first sorted point of every occupied cell; [V] = n
  const int32_t* rowbeg;                // [dby + 1], without the bitmap
  const uint32_t* occ;                  // one bit per grid cell, with the bitmap
  const unsigned short* wpref;          // occupied cells before every 32-cell word of occ
  // [a, b): the sorted points in the cells [c0, c1) of grid row y (c0 <= c1, both inside the row or at its end).  With
  // the bitmap: points before cell c = cell_start[wpref[c / 32] + popcount(occ[c / 32] below c)], two LDS reads and one
  // dependent read; without: two binary searches over the row's occupied cells.
  __device__ __forceinline__ void run(int y, int c0, int c1, int& a, int& b) const {
    if (bitmap) {
      const int w0 = c0 >> 5, w1 = c1 >> 5;
      a = cell_start[(int)wpref[w0] + __popc(occ[w0] & ((1u << (c0 & 31)) - 1u))];
      b = cell_start[(int)wpref[w1] + __popc(occ[w1] & ((1u << (c1 & 31)) - 1u))];
    } else {
      a = cell_start[lower_bound_u32(cell_key, rowbeg[y], rowbeg[y + 1], (uint32_t)c0)];
      b = cell_start[lower_bound_u32(cell_key, rowbeg[y], rowbeg[y + 1], (uint32_t)c1)];
    }
  }
};

// Builds the index over n points in a dbx x dby grid (dby <= kGridMaxRows, dbx * dby < 2^31).  cell_xy(i, ix, iy) ->
// column / row of point i; emit(e, idx) -> the float4 stored at sorted position e for point idx; scratch: room for n
// float4 in global memory, used when the sorted points do not fit the LDS (may be null where the caller knows they do).
// t_sorted: optional, receives the cycle counter after the sort (a caller's phase timing).  Block-wide collective; on return
// the index is visible to every thread.
template <typename CellXY, typename Emit>
__device__ __forceinline__ GridIndex grid_index_build(uint8_t* smem, int n, int dbx, int dby, float4* scratch, CellXY cell_xy, Emit emit,
                                                      long long* t_sorted = nullptr) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int* red_i = (int*)(smem + kGridSmallOff + 256);                      // [16]
  int* red_c = (int*)(smem + kGridSmallOff + 320);                      // [16]
  GridIndex g;
  g.dbx = dbx; g.dby = dby;
  // ---- sort by (cell, index) ---------------------------------------------------------------------------------------
  unsigned long long* keys = (unsigned long long*)smem;
  int npad = grid_sort_rows_block(smem, n, dbx, dby, (uint32_t*)(smem + kGridRowbegOff), red_i, red_c, 512, cell_xy);
  int path = 0;
  if (npad == 0) {                                     // crowded grid row or a large cloud: generic block sort
    int ib, vb;
    path = grid_sort_is_radix(n, (long long)dbx * dby, ib, vb) ? CFEAR_CORAL_PATH_SORT_RADIX : CFEAR_CORAL_PATH_SORT_BITONIC;
    npad = grid_sort_block(smem, n, (long long)dbx * dby, red_i, [&](int i) {
      int ix, iy;
      cell_xy(i, ix, iy);
      return (uint32_t)(ix + iy * dbx);
    });
  }
  if (t_sorted) *t_sorted = __builtin_readcyclecounter();
  // ---- cell table (key, start) -> LDS; sorted points -> LDS or scratch -----------------------------------------------
  const int per = npad / kGridSortThreads;              // 1..16 consecutive sorted elements per thread
  unsigned long long mine[kGridPerThread];
  const unsigned prev_cell = (tid * per > 0) ? (unsigned)(keys[tid * per - 1] >> 32) : 0xFFFFFFFFu;
  int heads = 0;
#pragma unroll
  for (int q = 0; q < kGridPerThread; q++) {
    const int e = tid * per + q;
    mine[q] = (q < per && e < n) ? keys[e] : ~0ull;
  }
  {
    unsigned pv = prev_cell;
#pragma unroll
    for (int q = 0; q < kGridPerThread; q++) {
      const int e = tid * per + q;
      if (q < per && e < n) {
        const unsigned vx = (unsigned)(mine[q] >> 32);
        heads += (e == 0 || vx != pv);
        pv = vx;
      }
    }
  }
  const int incl = wave_incl_scan_i32(heads);
  if (lane == 63) red_i[wave] = incl;
  __syncthreads();                                      // also: every thread has read its keys
  int voff = incl - heads;
  for (int wv = 0; wv < wave; wv++) voff += red_i[wv];
  int V = 0;
  for (int wv = 0; wv < 16; wv++) V += red_i[wv];
  const size_t Vp = ((size_t)V + 4) & ~(size_t)3;
  uint32_t* cell_key = (uint32_t*)smem;                 // [V]
  int32_t* cell_start = (int32_t*)(smem + Vp * 4);      // [V + 1]
  int32_t* rowbeg = (int32_t*)(smem + kGridRowbegOff);  // [dby + 1]
  // The sorted points follow the cell table in LDS when they fit (the usual case: a few thousand peaks), so the
  // neighbour sweep reads them at LDS latency; larger clouds keep them in the global scratch.
  const size_t spt_off = (Vp * 4 + ((size_t)V + 1) * 4 + 15) & ~(size_t)15;
  const bool spt_in_lds = spt_off + (size_t)n * 16 <= kGridRowbegOff;
  float4* spt = spt_in_lds ? (float4*)(smem + spt_off) : scratch;
  {
    unsigned pv = prev_cell;
    int ord = voff;
#pragma unroll
    for (int q = 0; q < kGridPerThread; q++) {
      const int e = tid * per + q;
      if (q < per && e < n) {
        const unsigned vx = (unsigned)(mine[q] >> 32);
        const int idx = (int)(unsigned)(mine[q] & 0xFFFFFFFFu);
        if (e == 0 || vx != pv) { cell_key[ord] = vx; cell_start[ord] = e; ord++; }
        pv = vx;
        spt[e] = emit(e, idx);
      }
    }
  }
  if (tid == 0) cell_start[V] = n;
  __threadfence_block();
  __syncthreads();
  // ---- O(1) cell look-ups: ONE BIT per grid cell + the occupied cells before every 32-cell word (the map
  //      surface_sort_kernel uses), instead of two binary searches over the row's cells (ten dependent reads) per grid row
  //      and point.  Kept behind the sorted points when it fits the LDS (grids up to ~3 x 10^5 cells for the usual peak
  //      clouds); otherwise the first occupied cell of every grid row, for the binary searches. ------------------------
  const long long ncells_ll = (long long)dbx * dby;
  const size_t occ_off = spt_in_lds ? ((spt_off + (size_t)n * 16 + 15) & ~(size_t)15) : spt_off;
  const long long nw32_ll = (ncells_ll >> 5) + 1;
  const bool bitmap = occ_off + (size_t)nw32_ll * 6 + 16 <= kGridRowbegOff;
  uint32_t* occ = (uint32_t*)(smem + occ_off);
  const int nw32 = bitmap ? (int)nw32_ll : 0;
  unsigned short* wpref = (unsigned short*)(occ + nw32);
  if (!bitmap) {
    for (int y = tid; y <= dby; y += kGridSortThreads)
      rowbeg[y] = lower_bound_u32(cell_key, 0, V, (uint32_t)((long long)y * dbx));
    __syncthreads();
  } else {
    for (int w = tid; w < nw32; w += kGridSortThreads) occ[w] = 0u;
    __syncthreads();
    for (int o = tid; o < V; o += kGridSortThreads) { const uint32_t c = cell_key[o]; atomicOr(&occ[c >> 5], 1u << (c & 31)); }
    __syncthreads();
    const int perw = (nw32 + kGridSortThreads - 1) / kGridSortThreads;
    const int w0 = min(nw32, tid * perw), w1 = min(nw32, w0 + perw);
    int to = 0;
    for (int w = w0; w < w1; w++) to += __popc(occ[w]);
    const int inclw = wave_incl_scan_i32(to);
    if (lane == 63) red_c[wave] = inclw;
    __syncthreads();
    int runw = inclw - to;
    for (int wv = 0; wv < wave; wv++) runw += red_c[wv];
    for (int w = w0; w < w1; w++) { wpref[w] = (unsigned short)runw; runw += __popc(occ[w]); }
    __syncthreads();
  }
  g.V = V;
  g.path = path | (spt_in_lds ? 0 : CFEAR_CORAL_PATH_SCRATCH) | (bitmap ? 0 : CFEAR_CORAL_PATH_BSEARCH);
  g.spt_in_lds = spt_in_lds; g.bitmap = bitmap; g.spt = spt;
  g.cell_key = cell_key; g.cell_start = cell_start; g.rowbeg = rowbeg; g.occ = occ; g.wpref = wpref;
  return g;
}
#endif
