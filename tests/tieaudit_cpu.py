"""A NumPy restatement of the tie audit (include/cfear_hip.h: cfear_association_ties_batch, cfear_scan_closest_ties) that does
not import the library: all minimisers of every 1-NN query in float32, the radius and direction tests of AddScanPairCost
(n_scan_normal.cpp:213-261, pointnormal.cpp:238-254) in float64, the bitwise-difference rule, the record sums and the
per-query layout -- and the constructed cases both test files share."""
import math

import numpy as np

CELL_DTYPE = np.dtype([("mean", "<f8", (2,)), ("normal", "<f8", (2,)), ("cov", "<f8", (4,)), ("scale", "<f8"),
                       ("avg_intensity", "<f8"), ("lambda_min", "<f8"), ("lambda_max", "<f8"), ("nsamples", "<i4"), ("pad", "<i4")])
RECORD_FIELDS = ("n_queries", "n_in_radius", "n_associated", "n_tied", "n_tied_effective", "max_group", "status", "pad")
OK, ERR_TOO_FEW_RESIDUALS = 0, -4
TILE = 1024                     # CFEAR_TIE_TILE: target cells per LDS tile of the kernels
ANGLE_OUTLIER = math.cos(math.pi / 6.0)


def src_to_tar(tar_pose, src_pose):
    """Tsrctotar = Ttar^-1 * Tsrc as (l0, l1, l2, l3, t0, t1): vectorToAffine3d, Eigen's Affine inverse (adjugate / det) and
    product, in the order of the oracle's aff_inv / aff_mul."""
    ct, st = math.cos(tar_pose[2]), math.sin(tar_pose[2])
    a = (ct, -st, st, ct, float(tar_pose[0]), float(tar_pose[1]))
    cs, ss = math.cos(src_pose[2]), math.sin(src_pose[2])
    b = (cs, -ss, ss, cs, float(src_pose[0]), float(src_pose[1]))
    det = a[0] * a[3] - a[2] * a[1]
    inv = 1.0 / det
    i0, i1, i2, i3 = a[3] * inv, -a[1] * inv, -a[2] * inv, a[0] * inv
    i4 = -(i0 * a[4] + i1 * a[5])
    i5 = -(i2 * a[4] + i3 * a[5])
    return (i0 * b[0] + i1 * b[2], i0 * b[1] + i1 * b[3], i2 * b[0] + i3 * b[2], i2 * b[1] + i3 * b[3],
            i0 * b[4] + i1 * b[5] + i4, i2 * b[4] + i3 * b[5] + i5)


def _keys(cells):
    """What the residual and the weight read of a cell, as integers: mean, normal, cov, scale (bit patterns), nsamples."""
    c = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
    f = np.concatenate([c["mean"], c["normal"], c["cov"], c["scale"][:, None]], axis=1)
    return np.concatenate([np.ascontiguousarray(f).view("<u8"), c["nsamples"].astype(np.uint64)[:, None]], axis=1)


def minimisers(cells, qx, qy):
    """All minimisers of the float32 queries (qx, qy) among the float means of `cells`: d = dx * dx; d += dy * dy in float32;
    the first candidate, or d < best, starts a group; d == best joins it.  -> best (float32), lo, hi, count, differs."""
    n = len(qx)
    c = np.ascontiguousarray(cells, dtype=CELL_DTYPE)
    m = c.shape[0]
    best = np.zeros(n, np.float32)
    lo, hi, count = np.full(n, -1, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    differs = np.zeros(n, bool)
    if m == 0 or n == 0:
        return best, lo, hi, count, differs
    tx, ty = c["mean"][:, 0].astype(np.float32), c["mean"][:, 1].astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = qx.astype(np.float32)[:, None] - tx[None, :]
        dy = qy.astype(np.float32)[:, None] - ty[None, :]
        d = dx * dx
        d = d + dy * dy
    assert d.dtype == np.float32
    keys = _keys(c)
    for i in range(n):
        row = d[i]
        if np.isnan(row[0]):                     # nothing is < or == a NaN: the first candidate stays
            best[i], lo[i], hi[i], count[i] = row[0], 0, 0, 1
            continue
        b = np.fmin.reduce(row)                  # (a NaN behind the first candidate never wins)
        eq = np.nonzero(row == b)[0]
        best[i], lo[i], hi[i], count[i] = b, eq[0], eq[-1], len(eq)
        differs[i] = bool((keys[eq] != keys[eq[0]]).any())
    return best, lo, hi, count, differs


def closest_ties(cells, queries_xy, d):
    """cfear_scan_closest_ties -> lo, hi, count (int32): (-1, -1, 0) unless the float distance is < d * d in double."""
    q = np.asarray(queries_xy, np.float64).reshape(-1, 2)
    best, lo, hi, count, _ = minimisers(cells, q[:, 0].astype(np.float32), q[:, 1].astype(np.float32))
    with np.errstate(invalid="ignore"):
        inr = (count > 0) & (best.astype(np.float64) < d * d)
    return (np.where(inr, lo, -1).astype(np.int32), np.where(inr, hi, -1).astype(np.int32), np.where(inr, count, 0).astype(np.int32))


def audit(scans, poses, radius=2.0, itr=1, residuals_per_block=1):
    """One job of cfear_association_ties_batch: scans = cell arrays (the last one the free source), poses [n_scans][3].
    -> (record dict, per_query int32 [(n_scans - 1) * n_src, 3], associated set {(tar_scan, lo, src)})."""
    scans = [np.ascontiguousarray(s, dtype=CELL_DTYPE) for s in scans]
    poses = np.asarray(poses, np.float64).reshape(len(scans), 3)
    src, last = scans[-1], len(scans) - 1
    n_src = src.shape[0]
    r = 2 * radius if itr == 1 else radius
    rec = dict.fromkeys(RECORD_FIELDS, 0)
    pq = np.zeros((last * n_src, 3), np.int32)
    assoc = set()
    for t in range(last):
        T = src_to_tar(poses[t], poses[last])
        px = T[0] * src["mean"][:, 0] + T[1] * src["mean"][:, 1] + T[4]
        py = T[2] * src["mean"][:, 0] + T[3] * src["mean"][:, 1] + T[5]
        best, lo, hi, count, differs = minimisers(scans[t], px.astype(np.float32), py.astype(np.float32))
        with np.errstate(invalid="ignore"):
            inr = (count > 0) & (best.astype(np.float64) < r * r)
        nsx = T[0] * src["normal"][:, 0] + T[1] * src["normal"][:, 1]
        nsy = T[2] * src["normal"][:, 0] + T[3] * src["normal"][:, 1]
        nt = scans[t]["normal"][np.maximum(lo, 0)] if scans[t].shape[0] else np.zeros((n_src, 2))
        sim = np.maximum(nsx * nt[:, 0] + nsy * nt[:, 1], 0.0)
        ass = inr & (sim > ANGLE_OUTLIER)
        tied = inr & (count >= 2)
        rec["n_queries"] += n_src
        rec["n_in_radius"] += int(inr.sum())
        rec["n_associated"] += int(ass.sum())
        rec["n_tied"] += int(tied.sum())
        rec["n_tied_effective"] += int((tied & differs).sum())
        rec["max_group"] = max(rec["max_group"], int(count[inr].max(initial=0)))
        blk = pq[t * n_src:(t + 1) * n_src]
        blk[:, 0], blk[:, 1], blk[:, 2] = np.where(inr, lo, -1), np.where(inr, hi, -1), np.where(inr, count, 0)
        assoc |= {(t, int(lo[s]), int(s)) for s in np.nonzero(ass)[0]}
    rec["status"] = ERR_TOO_FEW_RESIDUALS if rec["n_associated"] * residuals_per_block <= 1 else OK
    return rec, pq, assoc


def audit_batch(jobs, radius=2.0, itr=1, residuals_per_block=1):
    """-> (list of record dicts, per_query of the whole batch, offsets [n + 1]) in the layout of the C call."""
    recs, pqs, offs = [], [], [0]
    for scans, poses in jobs:
        rec, pq, _ = audit(scans, poses, radius, itr, residuals_per_block)
        recs.append(rec)
        pqs.append(pq)
        offs.append(offs[-1] + pq.shape[0])
    return recs, (np.concatenate(pqs) if pqs else np.zeros((0, 3), np.int32)), np.array(offs, np.int64)


def record_tuple(rec):
    return tuple(int(rec[k]) for k in RECORD_FIELDS)


# ---- constructed cases -------------------------------------------------------------------------------------------------
def make_cells(means, normals=None, nsamples=None):
    means = np.asarray(means, np.float64).reshape(-1, 2)
    c = np.zeros(means.shape[0], CELL_DTYPE)
    c["mean"] = means
    c["normal"] = (1.0, 0.0) if normals is None else normals
    c["cov"] = (0.1, 0.0, 0.0, 0.1)
    c["scale"], c["avg_intensity"], c["lambda_min"], c["lambda_max"] = 1.0, 1.0, 1.0, 1.0
    c["nsamples"] = 1 if nsamples is None else nsamples
    return c


CLOSEST_D = 2.0


def closest_case():
    """The 37-cell target (not a multiple of 64) and the queries of the GetClosestTies test.
    cells 0-2: double means 1e-9 apart (equal floats), nsamples 3, 4, 5; cells 3, 4: bitwise equal; cells 5-8: (+-1, 0) and
    (0, +-1), four DISTINCT cells equidistant from the origin; 28 more on a line, the first of them at (10, -12)."""
    means = [(5.0, 5.0), (5.0 + 1e-9, 5.0), (5.0, 5.0 - 1e-9), (-7.25, 3.5), (-7.25, 3.5), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.0, -1.0)]
    means += [(10.0 + 1.37 * k, -12.0 + 0.9 * k) for k in range(28)]
    cells = make_cells(means)
    cells["nsamples"][:3] = (3, 4, 5)
    assert cells.shape[0] == 37
    inside = float(np.nextafter(np.float32(8.0), np.float32(9.0)))      # one float ulp inside d of (10, -12)
    queries = np.array([(0.0, 0.0),              # four cells at distance 1: count 4, lo 5, hi 8
                        (5.1, 5.2),              # the three cells with equal float means
                        (-7.0, 3.0),             # the two bitwise-equal cells
                        (8.0, -12.0),            # exactly d from (10, -12): excluded, the test is strict
                        (inside, -12.0),         # one float ulp inside
                        (500.0, 500.0),          # far
                        (float("nan"), 0.0),     # never in radius
                        (-7.3, 3.4), (-1.2, -0.1), (-0.4, -0.7), (-30.0, -30.0)])
    return cells, queries


def _rot(a):
    return np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])


def _to_frame(pose, world):
    """world points -> the frame of `pose` (x, y, theta)"""
    return (np.asarray(world, np.float64).reshape(-1, 2) - np.asarray(pose[:2])) @ _rot(pose[2])


def _job(rng, n_scans, n_src, tile_case=False):
    """One constructed job.  The source cells are scattered over 60 m; every fixed scan holds a noisy copy of most of them,
    some fillers, and the planted cases -- planted on EXACT copies of a source cell's position, so the query of that cell
    finds them whatever the last bit of the transform is:
      source 0  a bitwise copy of its target cell appended           -> tied, not effective
      source 1  a copy with another nsamples appended                -> tied, effective
      source 2  a copy whose double mean differs by 1e-9 (equal floats) and whose cov differs -> tied, effective
      source 3  a copy with the normal turned by 90 degrees INSERTED IN FRONT: the lowest of the group fails the direction
                test, the highest would pass -> tied, effective, not associated
      source 4  alone at 80 m, its only target cell 3 m away: between radius and 2 * radius -> in radius at itr 1 only
    tile_case: a fixed scan of TILE + 1 cells whose last cell ties with cell 5."""
    poses = np.column_stack([rng.uniform(-3, 3, n_scans), rng.uniform(-3, 3, n_scans), rng.uniform(-0.6, 0.6, n_scans)])
    ps = poses[-1]
    src_mean = rng.uniform(-30, 30, (n_src, 2))
    ang = rng.uniform(-math.pi, math.pi, n_src)
    if n_src > 4:
        src_mean[4] = (80.0, 80.0)
    src = make_cells(src_mean, np.column_stack([np.cos(ang), np.sin(ang)]), rng.integers(6, 40, n_src))
    world = src_mean @ _rot(ps[2]).T + ps[:2]
    world_ang = ang + ps[2]
    scans = []
    for t in range(n_scans - 1):
        pt = poses[t]
        keep = np.nonzero(rng.uniform(size=n_src) < 0.85)[0]
        keep = np.union1d(keep, np.arange(min(n_src, 4)))
        keep = keep[keep != 4]
        noise = rng.normal(0.0, 0.25, (len(keep), 2))
        noise[keep < 4] = 0.0
        w = world[keep] + noise
        a = world_ang[keep] + rng.uniform(-0.3, 0.3, len(keep)) - pt[2]          # within 17 degrees: passes the 30-degree test
        n_fill = (TILE - len(keep)) if tile_case else 10
        fill = rng.uniform(-150, 150, (n_fill, 2)) if tile_case else rng.uniform(-40, 40, (n_fill, 2))
        fa = rng.uniform(-math.pi, math.pi, n_fill)
        tar = make_cells(np.concatenate([_to_frame(pt, w), fill]),
                         np.column_stack([np.cos(np.concatenate([a, fa])), np.sin(np.concatenate([a, fa]))]),
                         rng.integers(6, 40, len(keep) + n_fill))
        if tile_case:
            assert tar.shape[0] == TILE
            tar[5], tar[int(np.nonzero(keep == 0)[0][0])] = tar[int(np.nonzero(keep == 0)[0][0])].copy(), tar[5].copy()
            dup = tar[5:6].copy()
            dup["nsamples"] += 1
            tar = np.concatenate([tar, dup])                                      # cell TILE: the second tile's only cell
            scans.append(tar)
            continue
        at = {int(s): int(i) for i, s in enumerate(keep)}
        extra = [tar[at[0]:at[0] + 1].copy()]
        if n_src > 4:
            b = tar[at[1]:at[1] + 1].copy()
            b["nsamples"] += 1
            c = tar[at[2]:at[2] + 1].copy()
            c["mean"][0, 0] += 1e-9
            c["cov"][0, 0] = 0.2
            assert np.float32(c["mean"][0, 0]) == np.float32(tar["mean"][at[2], 0]) and abs(c["mean"][0, 0]) > 0.05
            ring = make_cells(_to_frame(pt, world[4] + (3.0, 0.0)), [(math.cos(world_ang[4] - pt[2]), math.sin(world_ang[4] - pt[2]))], 9)
            extra += [b, c, ring]
        tar = np.concatenate([tar] + extra)
        if n_src > 4:
            bad = tar[at[3]:at[3] + 1].copy()
            bad["normal"][0] = (-bad["normal"][0, 1], bad["normal"][0, 0])
            tar = np.concatenate([bad, tar])
        scans.append(tar)
    return scans + [src], poses


def constructed_jobs():
    """Seven jobs: n_scans 2, 3, 4; source sizes 1, 63, 64, 65, 257, 300 (wavefront and workgroup boundaries, the 256-stride
    loop); every pose a rotation and a translation; the last job has the fixed scan of TILE + 1 cells."""
    rng = np.random.default_rng(20261020)
    shapes = [(2, 1), (3, 63), (4, 64), (2, 65), (3, 257), (4, 300)]
    return [_job(rng, ns, n) for ns, n in shapes] + [_job(rng, 2, 65, tile_case=True)]
