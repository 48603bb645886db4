// eigen_quat.hpp -- the Eigen 3.3 quaternion conversions the reference's pose types go through, restated operation by
// operation in fp64 without contraction (-ffp-contract=off): Quaterniond(Matrix3d) and toRotationMatrix().  Host and device.
// Used by trajsync.hip (pose_interp), graphfinish.hip (PoseEigToCeres) and pose_rows.hpp (PoseCeresToEig).  Neither Eigen nor ROS is part
// of the reference tree or of this build ("restated, not pinned").
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ double sqrt_rn(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(v);
#else
  return std::sqrt(v);
#endif
}

// Eigen 3.3 Quaternion(Matrix3d), src/Geometry/Quaternion.h quaternionbase_assign_impl<Other, 3, 3>: q = (x, y, z, w), no
// normalisation.  m is a KITTI row (stride 4).  The trace is the unrolled redux of a 3-vector, m00 + (m11 + m22).
template <int I>
__host__ __device__ __forceinline__ void quat_pivot(const double* m, double* q) {
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double t = sqrt_rn(((m[5 * I] - m[5 * J]) - m[5 * K]) + 1.0);
  q[I] = 0.5 * t;
  t = 0.5 / t;
  q[3] = (m[4 * K + J] - m[4 * J + K]) * t;
  q[J] = (m[4 * J + I] + m[4 * I + J]) * t;
  q[K] = (m[4 * K + I] + m[4 * I + K]) * t;
}
__host__ __device__ __forceinline__ void quat_from_rows(const double* m, double* q) {
  double t = m[0] + (m[5] + m[10]);
  if (t > 0.0) {
    t = sqrt_rn(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[9] - m[6]) * t;
    q[1] = (m[2] - m[8]) * t;
    q[2] = (m[4] - m[1]) * t;
    return;
  }
  int i = 0;
  double mii = m[0];
  if (m[5] > m[0]) { i = 1; mii = m[5]; }
  if (m[10] > mii) i = 2;
  if (i == 0) quat_pivot<0>(m, q); else if (i == 1) quat_pivot<1>(m, q); else quat_pivot<2>(m, q);
}

// QuaternionBase::toRotationMatrix, in its tx = 2x form, into the 3 x 3 block of a KITTI row (stride 4); q = (x, y, z, w)
__host__ __device__ __forceinline__ void quat_to_rows(const double* q, double* m) {
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz;         m[2] = txz + twy;
  m[4] = txy + twz;         m[5] = 1.0 - (txx + tzz); m[6] = tyz - twx;
  m[8] = txz - twy;         m[9] = tyz + twx;         m[10] = 1.0 - (txx + tyy);
}
