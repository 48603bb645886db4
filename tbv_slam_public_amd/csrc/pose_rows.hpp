// pose_rows.hpp -- the KITTI-row pose ([r | t] as 12 doubles, row by row: the 96-byte record a KITTI line holds) and its
// algebra, for the trajectory and graph kernels (evaluate.hip, trajsync.hip, graphfinish.hip) and their host halves.
//
// Everything is fp64.  Every routine has ONE operation order, shared with the Python restatements under tests/ and kept by
// -ffp-contract=off: the evaluator decides its segment ends by comparing sums of rounded distances, so a product that
// rounds differently is a different result.
//   product P Q          (p0 q0 + p1 q1) + p2 q2 per entry, ((p0 t0 + p1 t1) + p2 t2) + pt per row
//   inverse of [A | t]   two routines that round differently on purpose, pose_inv and affine_inverse below
//   alignment sums       a thread's strided serial sum, block_sum's tree (common.hpp): a unit's sums depend on the unit alone
#pragma once
#include <cstdio>

#include "common.hpp"
#include "eigen_quat.hpp"

constexpr double kIdentityRows[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// PoseCeresToEig (types.cpp:33-38) as a KITTI row: toRotationMatrix and the translation
__host__ __device__ __forceinline__ void pose3d_to_rows(const cfear_pose3d& P, double* m) {
  quat_to_rows(P.q, m);
  m[3] = P.p[0]; m[7] = P.p[1]; m[11] = P.p[2];
}

// One pose as a text row: std::fixed with the stream's 6 decimals, one space between the numbers, `end` behind the last
// (EvalTrajectory::Write, eval_trajectory.cpp:169-183; MatToString, types.cpp:64-73)
inline bool kitti_row_write(FILE* f, const double* m, const char* end) {
  for (int k = 0; k < 12; k++)
    if (fprintf(f, k == 11 ? "%.6f%s" : "%.6f ", m[k], end) <= 0) return false;
  return true;
}

// Affine3d::inverse() of [R | t]: Eigen's compute_inverse_size3_helper (the cofactors of column 0 give the determinant, every
// cofactor is multiplied by 1 / det), then t' = -(R' t).  Not pose_inv: that one divides.
inline void affine_inverse(const double in[12], double out[12]) {
  auto m = [&](int r, int c) { return in[4 * r + c]; };
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m(i1, j1) * m(i2, j2) - m(i1, j2) * m(i2, j1);
  };
  const double c0 = cof(0, 0), c1 = cof(1, 0), c2 = cof(2, 0);
  const double invdet = 1.0 / ((c0 * m(0, 0) + c1 * m(1, 0)) + c2 * m(2, 0));
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out[4 * r + c] = cof(c, r) * invdet;
  for (int r = 0; r < 3; r++) out[4 * r + 3] = -((out[4 * r] * in[3] + out[4 * r + 1] * in[7]) + out[4 * r + 2] * in[11]);
}

#if defined(__HIPCC__)
struct Pose { double m[12]; };

__device__ __forceinline__ Pose pose_load(const double* p) {
  Pose r;
#pragma unroll
  for (int k = 0; k < 12; k += 2) { const g_f64x2 v = gload<g_f64x2>(p + k); r.m[k] = v.x; r.m[k + 1] = v.y; }
  return r;
}
__device__ __forceinline__ void pose_store(double* p, const Pose& r) {
#pragma unroll
  for (int k = 0; k < 12; k += 2) { g_f64x2 v; v.x = r.m[k]; v.y = r.m[k + 1]; gstore<g_f64x2>(p + k, v); }
}
// np.linalg.inv as the devkit uses it (kitti_odometry.py:229-238): the cofactors of A, det = (a00 c00 + a01 c01) + a02 c02,
// adj / det (a division per entry) -- a real inverse, the 3 x 3 blocks of a 6-decimal pose file are not orthonormal.  Not
// affine_inverse: that one multiplies by 1 / det.
__device__ __forceinline__ Pose pose_inv(const Pose& P) {
  const double a00 = P.m[0], a01 = P.m[1], a02 = P.m[2], a10 = P.m[4], a11 = P.m[5], a12 = P.m[6], a20 = P.m[8], a21 = P.m[9],
               a22 = P.m[10];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double c10 = a02 * a21 - a01 * a22, c11 = a00 * a22 - a02 * a20, c12 = a01 * a20 - a00 * a21;
  const double c20 = a01 * a12 - a02 * a11, c21 = a02 * a10 - a00 * a12, c22 = a00 * a11 - a01 * a10;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  Pose I;
  I.m[0] = c00 / det; I.m[1] = c10 / det; I.m[2] = c20 / det;
  I.m[4] = c01 / det; I.m[5] = c11 / det; I.m[6] = c21 / det;
  I.m[8] = c02 / det; I.m[9] = c12 / det; I.m[10] = c22 / det;
#pragma unroll
  for (int r = 0; r < 3; r++) I.m[4 * r + 3] = -((I.m[4 * r] * P.m[3] + I.m[4 * r + 1] * P.m[7]) + I.m[4 * r + 2] * P.m[11]);
  return I;
}
__device__ __forceinline__ Pose pose_mul(const Pose& A, const Pose& B) {
  Pose R;
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) R.m[4 * r + c] = (A.m[4 * r] * B.m[c] + A.m[4 * r + 1] * B.m[4 + c]) + A.m[4 * r + 2] * B.m[8 + c];
    R.m[4 * r + 3] = ((A.m[4 * r] * B.m[3] + A.m[4 * r + 1] * B.m[7]) + A.m[4 * r + 2] * B.m[11]) + A.m[4 * r + 3];
  }
  return R;
}
__device__ __forceinline__ double norm3(double x, double y, double z) { return __dsqrt_rn((x * x + y * y) + z * z); }
// rotation_error, kitti_odometry.py:143-155
__device__ __forceinline__ double rotation_error(const Pose& P) {
  const double d = 0.5 * (((P.m[0] + P.m[5]) + P.m[10]) - 1.0);
  return acos(fmax(fmin(d, 1.0), -1.0));
}

// The sums a 3 x 3 alignment is solved from (cfear_align_from_sums), by one workgroup of kAlignThreads threads over one unit
// of the batch: the means of x and y over the items that count, then sum (y_i - my)(x_i - mx)^T.  red: 4 doubles of LDS.
// Src says where the positions are and how the sums are scaled:
//   n                    items of the unit
//   kSkips               whether counts(i) can be false: only then are the counted items summed (exactly, as doubles)
//   counts(i), x(i, k), y(i, k)
//   mean_div(counted)    what the sums of x and y are divided by
//   cov(sum)             what is stored for an entry of the 3 x 3 sum
// out[0..5] the means, out[6..14] the 3 x 3 sum row-major, out[15] the counted items (0.0 without kSkips).
constexpr int kAlignThreads = 256;
template <class Src>
__device__ __forceinline__ void align_sums(const Src& src, double* out, double* red) {
  double s[6] = {0, 0, 0, 0, 0, 0}, cnt = 0.0;
  for (int i = threadIdx.x; i < src.n; i += kAlignThreads) {
    if (Src::kSkips && !src.counts(i)) continue;
    if constexpr (Src::kSkips) cnt += 1.0;
#pragma unroll
    for (int k = 0; k < 3; k++) { s[k] += src.x(i, k); s[3 + k] += src.y(i, k); }
  }
  double counted = 0.0;
  if constexpr (Src::kSkips) counted = block_sum(cnt, red);
  const double div = src.mean_div(counted);
  double mean[6];
#pragma unroll
  for (int k = 0; k < 6; k++) mean[k] = block_sum(s[k], red) / div;
  double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < src.n; i += kAlignThreads) {
    if (Src::kSkips && !src.counts(i)) continue;
    double x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { x[k] = src.x(i, k) - mean[k]; y[k] = src.y(i, k) - mean[3 + k]; }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int q = 0; q < 3; q++) c[3 * r + q] += y[r] * x[q];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const double v = src.cov(block_sum(c[k], red));
    if (threadIdx.x == 0) out[6 + k] = v;
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = mean[k];
    out[15] = counted;
  }
}
#endif  // __HIPCC__
