"""NumPy restatement of the voxel-order audit (cfear_voxel_order_audit_batch), vectorised per voxel.
It implements the definitions of include/cfear_hip.h with the same operation order as the device -- separate multiplies and
adds, sequential sums (np.cumsum accumulates left to right; np.sum does not) -- and shares no code with it or with the oracle.

Per voxel, with its n points in INPUT order and u = 2^-24:
  c_fwd, c_rev   sequential float32 sums first to last / last to first, divided by float32(n)
  S, A           fp64 sums of x and |x|;  g = (n-1)u / (1 - (n-1)u);  mid = S / n;  t = (g A) / n
  e              (t + u (|mid| + t)) + 2^-40 (|mid| + 1)
  pair classes   d2min, d2max from every point to the box [mid - e, mid + e]: sure-in d2max (1 + 8u) < r2, sure-out
                 d2min (1 - 8u) >= r2, exposed otherwise
  changed        the float test (dx = c.x - p.x; d = dx * dx; d += dy * dy; d < r2) differs between c_fwd and c_rev"""
import numpy as np

OK, ERR_INVALID_ARGUMENT, ERR_CAPACITY, ERR_EMPTY_CLOUD = 0, -1, -3, -6
TILE = 1024
MAX_POINTS = 40960
MAX_INDEX = 2.0 ** 23
U = np.float64(2.0 ** -24)
TINY = np.float64(2.0 ** -40)

RECORD_FIELDS = ("status", "n_points", "n_voxels", "n_centroids_reversed_differ", "n_pairs_exposed", "n_voxels_exposed",
                 "n_voxels_exposed_at_threshold", "n_voxels_changed_reversed", "max_voxel_points", "pad", "max_halfwidth")
RECORD_DTYPE = np.dtype([(n, "<i4") for n in RECORD_FIELDS[:-1]] + [("max_halfwidth", "<f8")])
VOXEL_DTYPE = np.dtype([("key", "<u4"), ("n_points", "<i4"), ("c_fwd", "<f4", 2), ("c_rev", "<f4", 2), ("e", "<f8", 2),
                        ("n_sure_in", "<i4"), ("n_exposed", "<i4"), ("changed_reversed", "<i4"), ("pad", "<i4")])
SURE_OUT, SURE_IN, EXPOSED = 0, 1, 2


def constants(radius, factor):
    """(leaf, inv_leaf, r2) as MapPointNormal and KdTreeFLANN::radiusSearch form them: radius is a float, the factor a double."""
    rf = np.float32(radius)
    leaf = np.float32(np.float64(rf) / np.float64(factor))
    return leaf, np.float32(1.0) / leaf, np.float32(np.float64(rf) * np.float64(rf))


def voxel_keys(cloud, radius=3.0, factor=1.0):
    """pcl::VoxelGrid's key of every point, or a status: floor(x * inv_leaf) - min_b in float, ijk0 + ijk1 * div_bx."""
    xy = np.ascontiguousarray(cloud, np.float32)[:, :2]
    n = xy.shape[0]
    if n == 0:
        return ERR_EMPTY_CLOUD
    if n > MAX_POINTS:
        return ERR_CAPACITY
    if not np.isfinite(xy).all():
        return ERR_INVALID_ARGUMENT
    inv_leaf = constants(radius, factor)[1]
    with np.errstate(over="ignore"):
        fx, fy = np.floor(xy[:, 0] * inv_leaf), np.floor(xy[:, 1] * inv_leaf)
    if not (np.abs(np.array([fx.min(), fx.max(), fy.min(), fy.max()])) <= MAX_INDEX).all():
        return ERR_CAPACITY
    min_bx, min_by = int(fx.min()), int(fy.min())
    div_bx, div_by = int(fx.max()) - min_bx + 1, int(fy.max()) - min_by + 1
    if div_bx * div_by > 2 ** 31 - 1:
        return ERR_CAPACITY
    ijk0 = (fx - np.float32(min_bx)).astype(np.int64)
    ijk1 = (fy - np.float32(min_by)).astype(np.int64)
    return (ijk0 + ijk1 * div_bx).astype(np.uint32)


def _seq_sum(a):
    return np.cumsum(a, dtype=a.dtype)[-1]


def audit(cloud, radius=3.0, factor=1.0, detail=False):
    """-> (record, voxel table in ascending key); with detail also a dict: mid [V, 2] and classes uint8 [V, n]."""
    cloud = np.ascontiguousarray(cloud, np.float32)
    rec = np.zeros((), RECORD_DTYPE)
    rec["n_points"] = cloud.shape[0]
    keys = voxel_keys(cloud, radius, factor)
    if isinstance(keys, int):
        rec["status"] = keys
        out = (rec, np.zeros(0, VOXEL_DTYPE))
        return out + ({"mid": np.zeros((0, 2)), "classes": np.zeros((0, cloud.shape[0]), np.uint8)},) if detail else out
    r2 = constants(radius, factor)[2]
    r2d = np.float64(r2)
    x, y = cloud[:, 0].copy(), cloud[:, 1].copy()
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    ukeys = np.unique(keys)
    vox = np.zeros(len(ukeys), VOXEL_DTYPE)
    mids = np.zeros((len(ukeys), 2))
    classes = np.zeros((len(ukeys), len(x)), np.uint8)
    for v, k in enumerate(ukeys):
        idx = np.flatnonzero(keys == k)                        # input order
        n = len(idx)
        fn = np.float32(n)
        cf = np.array([_seq_sum(x[idx]) / fn, _seq_sum(y[idx]) / fn], np.float32)
        cr = np.array([_seq_sum(x[idx[::-1]]) / fn, _seq_sum(y[idx[::-1]]) / fn], np.float32)
        nd, nm1 = np.float64(n), np.float64(n - 1)
        g = (nm1 * U) / (1.0 - nm1 * U)
        lo, hi, e = np.zeros(2), np.zeros(2), np.zeros(2)
        for a, c in enumerate((xd, yd)):
            S, A = _seq_sum(c[idx]), _seq_sum(np.abs(c[idx]))
            mid = S / nd
            t = (g * A) / nd
            e[a] = (t + U * (np.abs(mid) + t)) + TINY * (np.abs(mid) + 1.0)
            lo[a], hi[a] = mid - e[a], mid + e[a]
            mids[v, a] = mid
        nx = np.maximum(np.maximum(lo[0] - xd, xd - hi[0]), 0.0)
        ny = np.maximum(np.maximum(lo[1] - yd, yd - hi[1]), 0.0)
        fx = np.maximum(xd - lo[0], hi[0] - xd)
        fy = np.maximum(yd - lo[1], hi[1] - yd)
        d2min, d2max = nx * nx + ny * ny, fx * fx + fy * fy
        sure_in = d2max * (1.0 + 8.0 * U) < r2d
        sure_out = d2min * (1.0 - 8.0 * U) >= r2d
        exposed = ~sure_in & ~sure_out
        classes[v] = np.where(sure_in, SURE_IN, np.where(exposed, EXPOSED, SURE_OUT))
        changed = bool((members(cf, x, y, r2) != members(cr, x, y, r2)).any())
        vox[v] = (k, n, cf, cr, e, int(sure_in.sum()), int(exposed.sum()), int(changed), 0)
    rec["n_voxels"] = len(ukeys)
    rec["n_centroids_reversed_differ"] = int((vox["c_fwd"].view(np.uint32) != vox["c_rev"].view(np.uint32)).any(1).sum())
    rec["n_pairs_exposed"] = int(vox["n_exposed"].sum())
    rec["n_voxels_exposed"] = int((vox["n_exposed"] > 0).sum())
    rec["n_voxels_exposed_at_threshold"] = int(((vox["n_sure_in"] < 6) & (vox["n_sure_in"] + vox["n_exposed"] >= 6)).sum())
    rec["n_voxels_changed_reversed"] = int(vox["changed_reversed"].sum())
    rec["max_voxel_points"] = int(vox["n_points"].max())
    rec["max_halfwidth"] = vox["e"].max()
    return (rec, vox, {"mid": mids, "classes": classes}) if detail else (rec, vox)


def members(c, x, y, r2):
    """The oracle's radius test at centroid c (float32 [2]) for float32 points: which of them the cell would be built from."""
    dx, dy = np.float32(c[0]) - x, np.float32(c[1]) - y
    d = dx * dx
    d = d + dy * dy
    return d < r2


def audit_batch(clouds, radius=3.0, factor=1.0):
    """-> (records [n], the voxel tables one after the other, the first status that is not OK)."""
    out = [audit(c, radius, factor) for c in clouds]
    rec = np.array([r for r, _ in out], RECORD_DTYPE) if out else np.zeros(0, RECORD_DTYPE)
    vox = np.concatenate([v for _, v in out]) if out else np.zeros(0, VOXEL_DTYPE)
    bad = [int(s) for s in rec["status"] if s != OK]
    return rec, vox, (bad[0] if bad else OK)
