"""A literal, serial restatement of EvalTrajectory's timestamp synchronisation (cfear_radarodometry/src/cfear_radarodometry/
eval_trajectory.cpp, cited as :line), what cfear_sync_trajectories (csrc/trajsync.hip) is compared with: One2OneCorrespondance
(:400-423), SearchByTime (:424-442), Interpolate (:443-460) and pose_interp (:461-491) walk interval by interval over
Python floats, as the reference walks its vector -- no sorted input is assumed and nothing is searched by bisection, so the
model shares no structure with the kernels.  roscpp's toSec and the three Eigen 3.3 quaternion routines are restated here
too (neither library is in the reference tree); WriteTUM (:185-211) and WriteCov (:214-232) are string formatters.
Also the inputs of the GPU tests (cases()), so that tests/test_trajsync_cpu.py can check what they claim to cover."""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
ROW_DTYPE = np.dtype([("est_index", "<i4"), ("gt_index", "<i4"), ("alpha", "<f8")])


def to_sec(ns):
    """ros::Time::toSec(): (double)sec + 1e-9 * (double)nsec."""
    sec, nsec = divmod(int(ns), 10 ** 9)
    return float(sec) + 1e-9 * float(nsec)


def quat_from_matrix(R):
    """Eigen 3.3 quaternionbase_assign_impl<Other, 3, 3>::run -> [x, y, z, w]; R: nested lists or a [3, 3] array."""
    m = [[float(R[r][c]) for c in range(3)] for r in range(3)]
    q = [0.0] * 4
    t = m[0][0] + (m[1][1] + m[2][2])               # the unrolled redux of a 3-vector
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def quat_branch(R):
    """Which branch quat_from_matrix takes: "trace", or the pivot 0 / 1 / 2."""
    if R[0][0] + (R[1][1] + R[2][2]) > 0.0:
        return "trace"
    i = 1 if R[1][1] > R[0][0] else 0
    return 2 if R[2][2] > R[i][i] else i


def quat_dot(a, b):
    """Eigen's dot of the four coefficients: a 2-wide packet sum, then the two lanes."""
    return (a[0] * b[0] + a[2] * b[2]) + (a[1] * b[1] + a[3] * b[3])


def slerp(t, a, b):
    """QuaternionBase::slerp (Eigen 3.3) -> ([x, y, z, w], True if the linear branch was taken)."""
    one = 1.0 - DBL_EPSILON
    d = quat_dot(a, b)
    abs_d = abs(d)
    linear = abs_d >= one
    if linear:
        scale0 = 1.0 - t
        scale1 = t
    else:
        theta = math.acos(abs_d)
        sin_theta = math.sin(theta)
        scale0 = math.sin((1.0 - t) * theta) / sin_theta
        scale1 = math.sin(t * theta) / sin_theta
    if d < 0.0:
        scale1 = -scale1
    return [scale0 * a[k] + scale1 * b[k] for k in range(4)], linear


def quat_to_matrix(q):
    """QuaternionBase::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def pose_interp(t, t1, t2, p1, p2):
    """:461-491 on KITTI rows ([12]) -> (the interpolated row, alpha)."""
    alpha = 0.0
    if t2 != t1:
        alpha = (t - t1) / (t2 - t1)
    a = [float(v) for v in p1]
    b = [float(v) for v in p2]
    rot1 = quat_from_matrix([a[0:3], a[4:7], a[8:11]])
    rot2 = quat_from_matrix([b[0:3], b[4:7], b[8:11]])
    R = quat_to_matrix(slerp(alpha, rot1, rot2)[0])
    tr = [(1.0 - alpha) * a[4 * r + 3] + alpha * b[4 * r + 3] for r in range(3)]
    tr[2] = 0.0                                       # result.translation()(2) = 0
    return [R[0][0], R[0][1], R[0][2], tr[0], R[1][0], R[1][1], R[1][2], tr[1], R[2][0], R[2][1], R[2][2], tr[2]], alpha


def search_by_time(ts, gt_sec, itr):
    """SearchByTime: -> (found, the position it leaves).  `for (auto&& it = itr; itr != last; it++)`: the loop variable IS
    the carried iterator."""
    n = len(gt_sec)
    if n <= 2:
        return False, 0
    last = n - 1
    while itr != last:
        if gt_sec[itr] <= ts and ts <= gt_sec[itr + 1]:
            return True, itr
        itr += 1
    return False, itr


def sync_pair(est, est_stamps, gt, gt_stamps, mode="chained"):
    """One pair.  est [n, 12] or None; -> dict(est, gt, stamps, rows, count): the kept rows in estimate order."""
    gt_sec = [to_sec(s) for s in gt_stamps]
    gt = np.asarray(gt, np.float64).reshape(-1, 12)
    keep_est, keep_gt, keep_stamp, rows = [], [], [], []
    guess = 0
    for i, stamp in enumerate(est_stamps):
        ts = to_sec(stamp)
        if mode == "independent":
            guess = 0                                 # Interpolate(t, out): init_guess = gt_vek.begin()
        found, guess = search_by_time(ts, gt_sec, guess)
        if found:
            pose, alpha = pose_interp(ts, gt_sec[guess], gt_sec[guess + 1], gt[guess], gt[guess + 1])
            keep_gt.append(pose)
            keep_stamp.append(int(stamp))
            rows.append((i, guess, alpha))
            if est is not None:
                keep_est.append(np.asarray(est[i], np.float64).reshape(12))
        else:
            guess = 0                                 # reset guess, :412
    n = len(rows)
    return dict(est=None if est is None else np.array(keep_est, np.float64).reshape(n, 12), gt=np.array(keep_gt, np.float64).reshape(n, 12),
                stamps=np.array(keep_stamp, np.int64), rows=np.array(rows, ROW_DTYPE), count=n)


def global_first_interval(est_stamps, gt_stamps):
    """Per estimate the first interval of the whole ground truth that contains it, or -1."""
    gt_sec = [to_sec(s) for s in gt_stamps]
    out = []
    for s in est_stamps:
        ts = to_sec(s)
        hit = [j for j in range(len(gt_sec) - 1) if gt_sec[j] <= ts <= gt_sec[j + 1]] if len(gt_sec) > 2 else []
        out.append(hit[0] if hit else -1)
    return out


def both_kept_differ(a, b):
    """The estimates two results (chained, independent) both keep with another gt_index: [(est_index, gt a, alpha a, gt b, alpha b)]."""
    ra = {int(r["est_index"]): r for r in a["rows"]}
    rb = {int(r["est_index"]): r for r in b["rows"]}
    return [(i, int(ra[i]["gt_index"]), float(ra[i]["alpha"]), int(rb[i]["gt_index"]), float(rb[i]["alpha"]))
            for i in sorted(set(ra) & set(rb)) if ra[i]["gt_index"] != rb[i]["gt_index"]]


# ---- the writers as string formatters -----------------------------------------------------------------------------------
def stamp_text(ns):
    sec, nsec = divmod(int(ns), 10 ** 9)
    return "%d.%09d " % (sec, nsec)


def tum_line(pose, stamp):
    p = [float(v) for v in pose]
    q = quat_from_matrix([p[0:3], p[4:7], p[8:11]])
    return stamp_text(stamp) + "%.4f %.4f %.4f " % (p[3], p[7], p[11]) + "%.4g %.4g %.4g %.4g" % tuple(q) + "\n"


def cov_line(cov, stamp):
    return stamp_text(stamp) + " ".join("%g" % float(v) for v in np.asarray(cov, np.float64).reshape(36)) + "\n"


def tum_text(poses, stamps):
    return "".join(tum_line(p, s) for p, s in zip(np.asarray(poses, np.float64).reshape(-1, 12), stamps))


def cov_text(cov, stamps):
    return "".join(cov_line(c, s) for c, s in zip(np.asarray(cov, np.float64).reshape(-1, 36), stamps))


# ---- inputs of the GPU tests -------------------------------------------------------------------------------------------
T0 = 1547000000 * 10 ** 9          # an Oxford bag's epoch: doubles resolve 2^-22 s = 238 ns here


def planar(x, y, th):
    c, s = math.cos(th), math.sin(th)
    return [c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, 0.0]


def rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def spatial(n, seed, big=False):
    """A 3-D path with a varying attitude; big: rotations of up to +-pi about every axis, which reach the negative-trace
    branches of the quaternion conversion and negative quaternion dots."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 12))
    amp = math.pi if big else 0.3
    ang = np.cumsum(rng.uniform(-0.4, 0.4, (n, 3)), 0) if not big else rng.uniform(-amp, amp, (n, 3))
    pos = np.cumsum(rng.uniform(-1.0, 2.0, (n, 3)), 0)
    for i in range(n):
        M = np.zeros((3, 4))
        M[:, :3] = rot_xyz(*ang[i])
        M[:, 3] = pos[i]
        P[i] = M.reshape(12)
    return P


def planar_path(n, seed):
    rng = np.random.default_rng(seed)
    th = np.cumsum(rng.uniform(-0.2, 0.25, n))
    x = np.cumsum(np.cos(th) * 1.5)
    y = np.cumsum(np.sin(th) * 1.5)
    return np.array([planar(x[i], y[i], th[i]) for i in range(n)])


def gt_grid(n, step_ns=20_000_000, start=T0, jitter=0, seed=0):
    """n ascending stamps, 50 Hz by default."""
    rng = np.random.default_rng(seed)
    s = start + step_ns * np.arange(n, dtype=np.int64)
    if jitter:
        s = s + rng.integers(0, jitter, n)
    return np.sort(s)


def est_between(n, gt_stamps, seed, lo=-0.1, hi=1.1):
    """n estimate stamps spread over the ground truth's span, widened by lo / hi (fractions of the span), ascending."""
    rng = np.random.default_rng(seed)
    if len(gt_stamps) == 0:
        return T0 + np.sort(rng.integers(0, 10 ** 9, n)).astype(np.int64)
    a, b = int(gt_stamps[0]), int(gt_stamps[-1])
    span = max(b - a, 1000)
    return np.sort(a + (rng.uniform(lo, hi, n) * span).astype(np.int64)).astype(np.int64)


def rounding_case():
    """Stamps near 1.547e18 ns that differ as integers and are equal as toSec doubles, chosen so that an integer comparison
    keeps a different set: -> (est_stamps, gt_stamps, the estimates an integer comparison would keep)."""
    g = [T0 + 1000, T0 + 2000, T0 + 3000, T0 + 4000]
    # 40 ns before the first and 40 ns after the last ground-truth stamp: outside as integers, inside as doubles
    e = [g[0] - 40, g[0] + 500, g[3] + 40, g[3] + 400]
    int_keep = [i for i, s in enumerate(e) if g[0] <= s <= g[3]]
    return np.array(e, np.int64), np.array(g, np.int64), int_keep


def case(name, est_stamps, gt_stamps, gt=None, est=None, seed=0):
    est_stamps = np.asarray(est_stamps, np.int64)
    gt_stamps = np.asarray(gt_stamps, np.int64)
    gt = planar_path(len(gt_stamps), seed + 1) if gt is None else np.asarray(gt, np.float64)
    est = spatial(len(est_stamps), seed + 2) if est is None else np.asarray(est, np.float64)
    return dict(name=name, est=est.reshape(-1, 12), est_stamps=est_stamps, gt=gt.reshape(-1, 12), gt_stamps=gt_stamps)


def _backward(n, at, gt_stamps, seed):
    """n ascending estimate stamps inside the ground truth; from index `at` on they restart from the beginning."""
    e = est_between(n, gt_stamps, seed, 0.3, 0.9)
    tail = est_between(n - at, gt_stamps, seed + 1, 0.05, 0.6)
    e[at:] = tail
    assert e[at] < e[at - 1]
    return e


def cases():
    """Every single-pair case of the GPU tests, by name (the issue's list)."""
    out = []
    g40 = gt_grid(40)
    for n_gt in (0, 1, 2, 3, 4):                                   # ground-truth length: <= 2 keeps nothing
        g = gt_grid(n_gt)
        out.append(case("gt_len_%d" % n_gt, est_between(9, g, 10 + n_gt, 0.0, 1.0) if n_gt else est_between(9, g, 10), g, seed=n_gt))
    for n_est in (0, 1, 63, 64, 65, 129):                          # the chain's and the prefix sum's chunk boundary
        out.append(case("est_len_%d" % n_est, est_between(n_est, g40, 20 + n_est, 0.02, 0.98), g40, seed=20 + n_est))
    out.append(case("est_before_and_after", est_between(70, g40, 31, -0.3, 1.3), g40, seed=31))
    e = np.concatenate([est_between(5, g40, 32, -0.5, -0.1), est_between(6, g40, 33, 1.1, 1.5)])
    out.append(case("est_all_outside", e, g40, seed=32))
    g200 = gt_grid(200, jitter=3_000_000, seed=5)
    out.append(case("backward_mid_chunk", _backward(100, 37, g200, 40), g200, seed=40))
    out.append(case("backward_at_chunk_boundary", _backward(130, 64, g200, 41), g200, seed=41))
    # estimates equal to ground-truth stamps: each lies in two intervals
    # After g40[5] + 7 ms the walk stands on interval 5; g40[5] itself lies in intervals 4 and 5, so the chained walk stays on 5
    # (alpha 0) where a search from the first pose takes 4 (alpha 1): max(position, a) against a.  The same again at 12 / 11.
    e = np.array([g40[5] + 7_000_000, g40[5], g40[5], g40[6], g40[9] + 7_000_000, g40[10], g40[12] + 9_000_000, g40[12], g40[0], g40[39], g40[20]], np.int64)
    out.append(case("est_equals_gt_stamp", e, g40, seed=42))
    g = gt_grid(12).copy()
    g[1] = g[0]                                                    # t2 == t1 in the first interval: alpha 0 (a later equal pair is
    g[4] = g[3]                                                    # never the first interval that contains its stamp)
    g[8] = g[9] = g[7]                                             # a run of three equal stamps
    # g[9] + 1 ms leaves the walk on interval 9; the step back to g[7] = g[8] = g[9] lies in intervals 6 .. 9 and stays on 9
    e = np.array([g[0], g[2] + 5_000_000, g[3], g[3] + 1_000_000, g[6] + 3_000_000, g[7], g[7], g[9] + 1_000_000, g[7], g[10] + 1_000_000, g[3]], np.int64)
    out.append(case("duplicate_gt_stamps", e, g, seed=43))
    e, g, _ = rounding_case()
    out.append(case("tosec_rounding", e, g, seed=44))
    g60 = gt_grid(60, jitter=2_000_000, seed=6)
    out.append(case("rotations_planar", est_between(90, g60, 45, 0.0, 1.0), g60, gt=planar_path(60, 45), seed=45))
    out.append(case("rotations_spatial", est_between(90, g60, 46, 0.0, 1.0), g60, gt=spatial(60, 46), seed=46))
    big = spatial(60, 47, big=True)
    big[10] = big[11]                                              # an identical-rotation pair: the linear slerp branch
    out.append(case("rotations_all_branches", est_between(400, g60, 47, 0.0, 1.0), g60, gt=big, seed=47))
    out.append(case("non_orthonormal_6_decimals", est_between(90, g60, 48, 0.0, 1.0), g60, gt=np.round(spatial(60, 48), 6),
                    est=np.round(spatial(90, 49), 6), seed=48))
    return out


def batch_300():
    """300 pairs of mixed lengths with empty pairs in the middle and explicit, non-contiguous offsets:
    -> (pairs, est_offsets, gt_offsets): pair t's estimates start at est_offsets[t] of arrays est_offsets[-1] long."""
    rng = np.random.default_rng(300)
    pairs, eo, go = [], [], []
    e_at, g_at = 3, 5
    for t in range(300):
        n_gt = int(rng.choice([0, 1, 2, 3, 7, 30, 90]))
        n_est = int(rng.choice([0, 1, 5, 63, 64, 65, 130]))
        if 140 <= t < 150:
            n_est = 0 if t % 2 else n_est
            n_gt = n_gt if t % 2 else 0
        g = gt_grid(n_gt, jitter=4_000_000, seed=t)
        e = est_between(n_est, g, 1000 + t, -0.1, 1.1)
        if t % 7 == 0 and n_est > 4:
            e[n_est // 2:] = e[:n_est - n_est // 2].copy()             # a backward step
        elif t % 5 == 1 and n_est >= 5 and n_gt >= 7:
            j = n_gt // 2                                              # into interval j, then back onto its first stamp: the chained
            e[1], e[2] = g[j] + max(int(g[j + 1] - g[j]) // 2, 1), g[j]    # walk stays on j, the independent search takes j - 1
        pairs.append(case("batch_%d" % t, e, g, gt=spatial(n_gt, t) if t % 3 else None, seed=t))
        eo.append(e_at)
        go.append(g_at)
        e_at += n_est + int(rng.integers(0, 4))
        g_at += n_gt + int(rng.integers(0, 3))
    return pairs, np.array(eo + [e_at], np.int64), np.array(go + [g_at], np.int64)
