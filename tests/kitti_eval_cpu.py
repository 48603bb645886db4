"""NumPy restatement of the KITTI odometry metric as the reference's devkit computes it
(radar_kitti_benchmark/python/kitti_odometry.py, `eval --align 6dof`): the independent checker of csrc/evaluate.hip for
inputs the reference has no record of.  tests/test_kitti_eval_cpu.py pins it to the reference's recorded outputs.

The arithmetic is written out elementwise, in one fixed order and without BLAS / LAPACK in the pose algebra, so that the
quantities that DECIDE something (the ground-truth distances and with them every last_frame) are the same bits as the
kernels', which follow the same order under -ffp-contract=off:

    inverse of [A | t]   cofactors c_ij of A, det = (a00 c00 + a01 c01) + a02 c02, inv = adj / det (a division per entry),
                         t' = -((i0 t0 + i1 t1) + i2 t2) per row
    product P Q          r = (p0 q0 + p1 q1) + p2 q2 per entry, t = ((p0 t0 + p1 t1) + p2 t2) + pt per row
    norms                sqrt((x x + y y) + z z)

Poses are [n][12] doubles, the rows of the 3 x 4 matrix as a KITTI file prints them."""
import numpy as np

LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)          # KittiEvalOdom.__init__, :90
ALIGNMENTS = ("none", "6dof")


def _split(P):
    P = np.asarray(P, np.float64).reshape(-1, 3, 4)
    return P[:, :, :3], P[:, :, 3]


def _join(R, t):
    return np.concatenate([R, t[:, :, None]], 2).reshape(-1, 12)


def inv(P):
    """General inverse of [A | t; 0 0 0 1]: the 3 x 3 blocks of a 6-decimal file are not orthonormal."""
    A, t = _split(P)
    a = lambda i, j: A[:, i, j]
    c00 = a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)
    c01 = a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)
    c02 = a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)
    c10 = a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)
    c11 = a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)
    c12 = a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)
    c20 = a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)
    c21 = a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)
    c22 = a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)
    det = (a(0, 0) * c00 + a(0, 1) * c01) + a(0, 2) * c02
    with np.errstate(all="ignore"):
        I = np.stack([np.stack([c00, c10, c20], 1), np.stack([c01, c11, c21], 1), np.stack([c02, c12, c22], 1)], 1) / det[:, None, None]
    ti = -((I[:, :, 0] * t[:, 0:1] + I[:, :, 1] * t[:, 1:2]) + I[:, :, 2] * t[:, 2:3])
    return _join(I, ti)


def mul(P, Q):
    A, ta = _split(P)
    B, tb = _split(Q)
    R = (A[:, :, 0:1] * B[:, 0:1, :] + A[:, :, 1:2] * B[:, 1:2, :]) + A[:, :, 2:3] * B[:, 2:3, :]
    t = ((A[:, :, 0] * tb[:, 0:1] + A[:, :, 1] * tb[:, 1:2]) + A[:, :, 2] * tb[:, 2:3]) + ta
    return _join(R, t)


def _norm3(t):
    return np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])


def rotation_error(P):
    """:143-155"""
    R, _ = _split(P)
    d = 0.5 * (((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - 1.0)
    return np.arccos(np.maximum(np.minimum(d, 1.0), -1.0))


def umeyama_rotation(cov):
    """u s v of :64-73 from the two leading singular pairs: u diag(1, 1, det u det v) v^T = u1 v1^T + u2 v2^T +
    (u1 x u2)(v1 x v2)^T, which does not read the third singular vectors (arbitrary in sign for planar data)."""
    u, _, vt = np.linalg.svd(cov)
    u1, u2, v1, v2 = u[:, 0], u[:, 1], vt[0], vt[1]
    return np.outer(u1, v1) + np.outer(u2, v2) + np.outer(np.cross(u1, u2), np.cross(v1, v2))


def align_terms(E, G):
    """The means of the positions and 1/n sum (y_i - my)(x_i - mx)^T, :49-61 (x = estimate, y = ground truth)."""
    x, y = _split(E)[1], _split(G)[1]
    n = x.shape[0]
    mx, my = x.sum(0) / n, y.sum(0) / n
    return mx, my, (y - my).T @ (x - mx) / n


def align_6dof(E, G):
    """umeyama_alignment(x = estimate, y = ground truth, with_scale=False), :32-79, :718-737"""
    mx, my, cov = align_terms(E, G)
    r = umeyama_rotation(cov)
    t = my - r @ mx
    return np.concatenate([r, t[:, None]], 1).reshape(1, 12)


def normalise(P):
    """:708-714"""
    P = np.asarray(P, np.float64).reshape(-1, 12)
    return mul(np.repeat(inv(P[:1]), len(P), 0), P)


def evaluate(est, gt, step_size=10, alignment="6dof", lengths=LENGTHS, align=None):
    """One (estimate, ground truth) pair -> dict: rows (first_frame, last_frame, length as int64 arrays; r_err / len,
    t_err / len, speed), the summary figures in radians and fractions, per-length means and counts, dist, the aligned
    poses and the alignment [r | t] ("align", 12 numbers).  `align` replaces the 6dof alignment's own [r | t] by a given one,
    applied in the same way: everything behind the SVD is then one operation sequence for whoever computed that [r | t]."""
    est, gt = np.asarray(est, np.float64).reshape(-1, 12), np.asarray(gt, np.float64).reshape(-1, 12)
    if est.shape[0] != gt.shape[0]:
        raise ValueError("estimate and ground truth differ in length")
    n = est.shape[0]
    if n < 2:
        raise ValueError("fewer than 2 poses")
    if step_size < 1:
        raise ValueError("step_size < 1")
    if alignment not in ALIGNMENTS:
        raise ValueError("alignment %r is not supported" % (alignment,))
    # normalise, :708-714
    E, G = normalise(est), normalise(gt)
    T = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0]])
    if alignment == "6dof":
        T = align_6dof(E, G) if align is None else np.asarray(align, np.float64).reshape(1, 12)
        E = mul(np.repeat(T, n, 0), E)
    # distances over the ground truth, :123-141 (cumsum adds serially, left to right)
    tg = _split(G)[1]
    dist = np.concatenate([[0.0], np.cumsum(_norm3(tg[:-1] - tg[1:]))])
    # segments, :197-249
    firsts = np.arange(0, n, step_size)
    L = np.asarray(lengths, np.float64)
    last = np.searchsorted(dist, dist[firsts][:, None] + L[None, :], side="right")     # first i with dist[i] > threshold
    ok = last < n
    f_idx = np.broadcast_to(firsts[:, None], last.shape)[ok]
    l_idx = last[ok]
    k_idx = np.broadcast_to(np.arange(len(L))[None, :], last.shape)[ok]
    len_ = L[k_idx]
    dG = mul(inv(G[f_idx]), G[l_idx])
    dE = mul(inv(E[f_idx]), E[l_idx])
    err = mul(inv(dE), dG)
    r_err = rotation_error(err) / len_
    t_err = _norm3(_split(err)[1]) / len_
    speed = len_ / (0.1 * (l_idx - f_idx + 1.0))
    m = len(len_)
    out = {"first_frame": f_idx.astype(np.int64), "last_frame": l_idx.astype(np.int64), "length": len_.astype(np.int64),
           "r_err": r_err, "t_err": t_err, "speed": speed, "n_rows": m, "dist": dist, "est_aligned": E, "gt_aligned": G,
           "align": T[0]}
    out["ave_t_err"] = t_err.sum() / m if m else 0.0            # :264-287
    out["ave_r_err"] = r_err.sum() / m if m else 0.0
    out["seg_count"] = np.array([(k_idx == k).sum() for k in range(len(L))], np.int64)
    out["seg_t_err"] = np.array([t_err[k_idx == k].mean() if (k_idx == k).any() else 0.0 for k in range(len(L))])
    out["seg_r_err"] = np.array([r_err[k_idx == k].mean() if (k_idx == k).any() else 0.0 for k in range(len(L))])
    # ATE, :477-505
    e = _norm3(tg - _split(E)[1])
    out["ate"] = np.sqrt(np.mean(e * e))
    # RPE, :508-583: rel_err = inv(gt_rel) pred_rel over consecutive frames
    rel = mul(inv(mul(inv(G[:-1]), G[1:])), mul(inv(E[:-1]), E[1:]))
    R, t = _split(rel)
    tr_abs = _norm3(t)
    tr_sq = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    rot_abs = rotation_error(rel)
    beta = -np.arcsin(R[:, 2, 0])                               # rot2eul(...)[0], :14-18: the angle about x
    alpha = np.arctan2(R[:, 2, 1] / np.cos(beta), R[:, 2, 2] / np.cos(beta))
    out["rpe_trans"], out["rpe_trans_dev"] = np.mean(tr_abs), np.std(tr_abs)
    out["rpe_rot"], out["rpe_rot_dev"] = np.mean(rot_abs), np.std(rot_abs)
    out["bias_x"], out["bias_y"], out["bias_theta"] = np.mean(t[:, 0]), np.mean(t[:, 1]), np.mean(alpha)
    out["rmse_trans"] = np.sqrt(np.mean(tr_sq))
    return out


FIGURES = ("ave_t_err", "ave_r_err", "ate", "rpe_trans", "rpe_trans_dev", "rpe_rot", "rpe_rot_dev", "bias_x", "bias_y",
           "bias_theta", "rmse_trans")


def result_lines(seq, s):
    """write_result, :608-630: the 12 lines of result.txt for one sequence.  This is where radians become degrees and
    fractions become percent; `s` maps the names of FIGURES to values (a dict from evaluate(), or a summary record)."""
    return ["Sequence-nr, {} \n".format(seq),
            "Trans.err.(%), {:.5f} \n".format(s["ave_t_err"] * 100),
            "Rot.err.(deg/100m), {:.5f} \n".format(s["ave_r_err"] / np.pi * 180 * 100),
            "ATE(m), {:.5f} \n".format(s["ate"]),
            "RPE(m), {:.5f} \n".format(s["rpe_trans"]),
            "RPE-dev(m), {:.5f} \n".format(s["rpe_trans_dev"]),
            "RPE(deg), {:.5f} \n".format(s["rpe_rot"] * 180 / np.pi),
            "RPE-dev(deg), {:.5f} \n".format(s["rpe_rot_dev"] * 180 / np.pi),
            "bias-x(m), {:.6f} \n".format(s["bias_x"]),
            "bias-y(m), {:.6f} \n".format(s["bias_y"]),
            "bias-theta(deg), {:.6f} \n".format(s["bias_theta"] * 180 / np.pi),
            "RMSE (m), {:.5f} \n".format(s["rmse_trans"])]


def error_lines(first_frame, r_err, t_err, length, speed):
    """save_sequence_errors, :251-262: str() of [first_frame (int), r_err / len, t_err / len, len (int), speed]."""
    return ["%d %s %s %d %s\n" % (int(f), repr(float(r)), repr(float(t)), int(L), repr(float(v)))
            for f, r, t, L, v in zip(first_frame, r_err, t_err, length, speed)]
