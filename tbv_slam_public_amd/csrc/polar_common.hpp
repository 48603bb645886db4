// polar_common.hpp -- what more than one of kstrong.hip, kstrong_legacy.hip, cacfar.hip and rotate.hip needs.
#pragma once

#include <algorithm>

#include "common.hpp"
#include "row_pieces.hpp"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
constexpr int kRowsPerBlock = 4;   // 4 wavefronts (rows) per 256-thread workgroup
constexpr int kMaxCols = 8192;     // bins of a row (the range axis)
constexpr int kMaxK = 1024;
constexpr int kXcds = 8;

// Why a batch of polar images is refused.  bins_major: the images are [range bins][azimuths], so the range axis -- the one
// kMaxCols limits -- is `rows`.  cfear_polar_rotate_ccw has no width limit and refuses kGeometry alone.
enum class DescFault { kNone, kGeometry, kTooWide };
inline DescFault polar_desc_fault(const cfear_polar_desc* d, bool bins_major = false) {
  if (!d || d->rows <= 0 || d->cols <= 0 || d->stride < d->cols || d->batch <= 0 ||
      (d->batch > 1 && d->batch_stride < (int64_t)d->rows * d->stride))
    return DescFault::kGeometry;
  return (bins_major ? d->rows : d->cols) > kMaxCols ? DescFault::kTooWide : DescFault::kNone;
}

// the answer of the host entry points that take [azimuths][bins] images
inline int check_desc(cfear_ctx* ctx, const cfear_polar_desc* d) {
  const DescFault f = polar_desc_fault(d);
  if (f == DescFault::kGeometry) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "bad polar descriptor");
  if (f == DescFault::kTooWide) return cfear_set_error(ctx, CFEAR_ERR_INVALID_ARGUMENT, "cols > %d unsupported", kMaxCols);
  return CFEAR_OK;
}

// Byte transpose of a 4 x 4 block in registers (six v_perm_b32): w0 .. w3 = four rows of four bytes; colw[e] = column e as
// {row 0, row 1, row 2, row 3}.
__device__ __forceinline__ void transpose4x4_bytes(const uint32_t w0, const uint32_t w1, const uint32_t w2, const uint32_t w3,
                                                   uint32_t (&colw)[4]) {
  const uint32_t t0 = __builtin_amdgcn_perm(w1, w0, 0x05010400u), t1 = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
  const uint32_t t2 = __builtin_amdgcn_perm(w3, w2, 0x05010400u), t3 = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
  colw[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u); colw[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
  colw[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u); colw[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}

// Persistent tile sweeps (kstrongest_cols_kernel, cacfar_cols_kernel): XCD x takes the images b = x (mod kXcds), `tiles` tiles
// each.  The slots per XCD: per_cu workgroups on every CU, fewer when the batch is small; the grid is slots * kXcds.
inline int xcd_grid_slots(int tiles, int batch, int n_cu, int per_cu) {
  const long long per_xcd = (long long)tiles * ((batch + kXcds - 1) / kXcds);
  return (int)std::max<long long>(1, std::min<long long>(per_xcd, std::max(1, n_cu * per_cu / kXcds)));
}

}  // namespace
