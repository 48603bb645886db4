"""NumPy restatement of the end of the reference's pose-graph run, what csrc/graphfinish.hip is compared with.  Written from
  PoseGraph::Align                      tbv_slam/src/tbv_slam/posegraph.cpp:235-263
  best_fit_transform                    cfear_radarodometry/src/cfear_radarodometry/eval_trajectory.cpp:343-395
  PoseEigToCeres / PoseCeresToEig       cfear_radarodometry/src/cfear_radarodometry/types.cpp:25-38
  the maps of PoseGraphVis::ProcessFrame  posegraph.cpp:539-584
and from Eigen 3.3's Quaternion.h (toRotationMatrix, the matrix -> quaternion assignment, normalize) and PCL 1.10's
transformPointCloud<PointXYZI, double>.  A helper module, not a test.

Poses are [n, 7] float64 rows (p, q = x, y, z, w); a pose matrix is a KITTI row [12] (3 x 4, row-major).  Everything after the
SVD is ONE fp64 operation sequence (no product is fused), the one the kernels run: align_apply() and graph_map() given the
same inputs must equal the library bit for bit.  The sums before the SVD are NumPy's own (best_fit_transform), as the
reference's are Eigen's: they agree with the library's only to rounding (see alignment_bound)."""
import math

import numpy as np

IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])


def to_rows(pose):
    """PoseCeresToEig: Eigen's QuaternionBase::toRotationMatrix in its tx = 2x form, and the translation -> KITTI row [12]."""
    px, py, pz, x, y, z, w = (float(v) for v in pose)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([1.0 - (tyy + tzz), txy - twz, txz + twy, px,
                     txy + twz, 1.0 - (txx + tzz), tyz - twx, py,
                     txz - twy, tyz + twx, 1.0 - (txx + tyy), pz])


def quat_branch(m):
    """Which branch the matrix -> quaternion assignment takes for the KITTI row m: 3 = trace, else the pivot 0, 1 or 2."""
    if m[0] + (m[5] + m[10]) > 0.0:
        return 3
    i, mii = 0, m[0]
    if m[5] > m[0]:
        i, mii = 1, m[5]
    if m[10] > mii:
        i = 2
    return i


def quat_from_rows(m):
    """Eigen 3.3 quaternionbase_assign_impl<Other, 3, 3> -> (x, y, z, w), not normalised."""
    m = [float(v) for v in m]
    q = [0.0] * 4
    b = quat_branch(m)
    if b == 3:
        t = math.sqrt((m[0] + (m[5] + m[10])) + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[9] - m[6]) * t
        q[1] = (m[2] - m[8]) * t
        q[2] = (m[4] - m[1]) * t
        return q
    i = b
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(((m[5 * i] - m[5 * j]) - m[5 * k]) + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (m[4 * k + j] - m[4 * j + k]) * t
    q[j] = (m[4 * j + i] + m[4 * i + j]) * t
    q[k] = (m[4 * k + i] + m[4 * i + k]) * t
    return q


def from_rows(m):
    """PoseEigToCeres: the quaternion of the 3 x 3 block, then normalize() -- every coefficient divided by the norm, whose
    square is the 2-wide packet reduction (xx + zz) + (yy + ww)."""
    q = quat_from_rows(m)
    norm = math.sqrt((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3]))
    return np.array([float(m[3]), float(m[7]), float(m[11])] + [v / norm for v in q])


def mul_rows(a, b):
    """[a] [b] of two KITTI rows: (a0 b0 + a1 b1) + a2 b2 per entry, plus the translation of a in the last column."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    r = [0.0] * 12
    for i in range(3):
        for c in range(3):
            r[4 * i + c] = (a[4 * i] * b[c] + a[4 * i + 1] * b[4 + c]) + a[4 * i + 2] * b[8 + c]
        r[4 * i + 3] = ((a[4 * i] * b[3] + a[4 * i + 1] * b[7]) + a[4 * i + 2] * b[11]) + a[4 * i + 3]
    return np.array(r)


def affine_inverse(m):
    """Affine3d::inverse(): Eigen's 3 x 3 inverse (the cofactors of column 0 give the determinant, every cofactor times
    1 / det -- the block is inverted, not transposed), then t' = -(R' t)."""
    m = [float(v) for v in m]
    at = lambda r, c: m[4 * r + c]

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return at(i1, j1) * at(i2, j2) - at(i1, j2) * at(i2, j1)
    c0, c1, c2 = cof(0, 0), cof(1, 0), cof(2, 0)
    invdet = 1.0 / ((c0 * at(0, 0) + c1 * at(1, 0)) + c2 * at(2, 0))
    out = [0.0] * 12
    for r in range(3):
        for c in range(3):
            out[4 * r + c] = cof(c, r) * invdet
    for r in range(3):
        out[4 * r + 3] = -((out[4 * r] * m[3] + out[4 * r + 1] * m[7]) + out[4 * r + 2] * m[11])
    return np.array(out)


def fit_terms(A, B):
    """The centroids (divided by max(rows, 1)) and H = AA^T BB of best_fit_transform, :351-368."""
    A, B = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(B, np.float64).reshape(-1, 3)
    rows = max(A.shape[0], 1)
    cA, cB = A.sum(0) / rows, B.sum(0) / rows
    return cA, cB, (A - cA).T @ (B - cB)


def best_fit_transform(A, B):
    """best_fit_transform(A, B) -> KITTI row of [R | t]: R = V U^T of H's SVD, the third row of V^T negated when det R < 0,
    t = cB - R cA.  LAPACK's SVD stands in for Eigen's JacobiSVD: both return identities for a zero H."""
    cA, cB, H = fit_terms(A, B)
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2] *= -1
        R = Vt.T @ U.T
    t = cB - R @ cA
    return np.concatenate([R, t[:, None]], 1).reshape(12)


def align_apply(poses, align):
    """Every node becomes PoseEigToCeres(Tgtalign * GetPose()), :251-253 -> [n, 7]."""
    return np.array([from_rows(mul_rows(align, to_rows(p))) for p in np.asarray(poses, np.float64).reshape(-1, 7)]).reshape(-1, 7)


def ate_terms(poses, gt, has_gt):
    """|Tgt.p - p| of the nodes with ground truth, in node order: sqrt((dx dx + dy dy) + dz dz), :258."""
    out = []
    for p, g, h in zip(np.asarray(poses, np.float64).reshape(-1, 7), np.asarray(gt, np.float64).reshape(-1, 7), has_gt):
        if h:
            d = [float(g[k]) - float(p[k]) for k in range(3)]
            out.append(math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return out


def ate_of(poses, gt, has_gt):
    """d / std::max(N, 1), the serial sum of :254-262: a mean, not an RMS."""
    terms = ate_terms(poses, gt, has_gt)
    s = 0.0
    for t in terms:
        s += t
    return s / max(len(terms), 1)


def align(poses, gt, has_gt, align_row=None):
    """PoseGraph::Align -> (new poses [n, 7], Tgtalign as a KITTI row, ate).  align_row: a given Tgtalign (the library's own)
    instead of this module's fit, so that both sides run one operation sequence behind the SVD."""
    poses, gt = np.asarray(poses, np.float64).reshape(-1, 7), np.asarray(gt, np.float64).reshape(-1, 7)
    has = np.asarray(has_gt).astype(bool)
    if align_row is None:
        align_row = affine_inverse(best_fit_transform(gt[has, :3], poses[has, :3]))
    new = align_apply(poses, align_row)
    return new, np.asarray(align_row, np.float64), ate_of(new, gt, has)


def alignment_bound(A, B, depth):
    """(b_r, b_t): how far two computations of Tgtalign may lie apart, after check_alignment of tests/test_gpu_kitti_eval.py.
    Both sides take the singular pairs of an H they summed in their own order.  R is the orthogonal polar factor of H with
    the determinant fixed; a perturbation dH moves it by at most 2 |dH| / (s2 + s3).  |dH| per side: a sum of depth d over
    terms whose magnitudes add up to about 2 s1, i.e. 2 d 2^-53 s1, plus an SVD's backward error of ~10 * 2^-53 s1.  `depth`
    is the two sides' depths added.  Tgtalign's block is R^-1 = R^T to rounding, so it moves as far; its translation
    cA - R^-1 cB by at most b_r |cB| sqrt(3) + 32 * 2^-53 (|cA| + |cB|)."""
    cA, cB, H = fit_terms(A, B)
    sv = np.linalg.svd(H, compute_uv=False)
    u = 2.0 ** -53
    b_r = 2.0 * (2 * depth + 20) * u * sv[0] / (sv[1] + sv[2])
    b_t = b_r * np.linalg.norm(cB) * np.sqrt(3) + 32 * u * (np.linalg.norm(cA) + np.linalg.norm(cB))
    return b_r, b_t


NUMPY_DEPTH = 22      # NumPy's pairwise sum over up to a few thousand terms (8 lanes, blocks of 128, then a tree)


def transform_cloud(row, xyzi):
    """pcl::transformPointCloud<PointXYZI, double>: float(((m0 x + m1 y) + m2 z) + m3) for the three rows, intensity copied."""
    c = np.asarray(xyzi, np.float32).reshape(-1, 4)
    x, y, z = (c[:, k].astype(np.float64) for k in range(3))
    m = [np.float64(v) for v in row]
    out = c.copy()
    for r in range(3):
        out[:, r] = (((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3]).astype(np.float32)
    return out


def graph_map(poses, gt, has_gt, clouds, skip_frames=1, want_gt_map=True):
    """The two maps of PoseGraphVis::ProcessFrame for one graph -> (map [N, 4], map_gt [M, 4]) float32."""
    assert skip_frames >= 1
    m, mg = [np.zeros((0, 4), np.float32)], [np.zeros((0, 4), np.float32)]
    for k in range(0, len(clouds), skip_frames):                       # std::distance(begin, itr) % skip_frames == 0, :573
        m.append(transform_cloud(to_rows(poses[k]), clouds[k]))
        if want_gt_map and has_gt[k]:
            mg.append(transform_cloud(to_rows(gt[k]), clouds[k]))
    return np.concatenate(m, 0), np.concatenate(mg, 0)


# ---- inputs shared by the CPU and GPU tests ---------------------------------------------------------------------------------
def euler_pose(x, y, z, roll, pitch, yaw):
    """A pose [7] from a translation and roll / pitch / yaw (its quaternion normalised as PoseEigToCeres would leave it)."""
    cr, sr, cp, sp, cy, sy = math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(yaw / 2), math.sin(yaw / 2)
    q = np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])
    return np.concatenate([[x, y, z], q / np.linalg.norm(q)])


def lap(n, seed, planar=True, radius=40.0):
    """A closed lap of n nodes as ground truth and an estimate that is the lap moved rigidly and perturbed -> (est, gt) [n, 7]."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    gt = np.array([euler_pose(radius * math.cos(t), 0.7 * radius * math.sin(t), 0.0 if planar else 3.0 * math.sin(2 * t),
                              0.0 if planar else 0.05 * math.sin(t), 0.0 if planar else 0.08 * math.cos(3 * t), t + np.pi / 2) for t in a])
    X = to_rows(euler_pose(6.0, -4.0, 0.0 if planar else 1.5, 0.0 if planar else 0.03, 0.0 if planar else -0.04, 0.4))
    est = np.array([from_rows(mul_rows(X, to_rows(g))) for g in gt])
    est[:, :2] += rng.normal(0, 0.05, (n, 2))
    if not planar:
        est[:, 2] += rng.normal(0, 0.05, n)
    return est, gt
