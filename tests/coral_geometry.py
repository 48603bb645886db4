"""CorAl test geometries and the helpers the geometry tests share: cloud builders with fixed seeds, a restatement of the
thresholds by which the grid index of coral_kernel and p2p_kernel (grid_index_build, tbv_slam_public_amd/csrc/gridsort.hpp)
picks its sort, the home of the sorted points and the cell lookup -- used ONLY to choose inputs; the tests assert the path
bits the kernels report -- and exact_coral, the per-point entropies from exact rational covariances."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

# ---- the index's limits and path bits (include/cfear_hip.h: CFEAR_CORAL_PATH_*, the pad of cfear_coral_result and of
#      cfear_p2p_result) ---------------------------------------------------------------------------------------------------
MAX_POINTS = 16384                     # kGridSortMaxPoints
MAX_GRID_ROWS = 4096                   # kGridMaxRows
MAX_CELLS = 2 ** 31 - 1
ROWBEG_OFF = MAX_POINTS * 8 + 16       # kGridRowbegOff: LDS bytes for cell table + sorted points + occupancy bitmap
PATH_SCRATCH, PATH_BSEARCH = 1, 2      # bit 0: sorted points in the global scratch; bit 1: binary-search lookup
SORT_ROWS, SORT_RADIX, SORT_BITONIC = 0, 1, 2          # bits 2-3


def path_bits(scratch, bsearch, sort):
    return int(bool(scratch)) | (int(bool(bsearch)) << 1) | (int(sort) << 2)


def describe(bits):
    return "%s/%s/%s" % ("scratch" if bits & 1 else "lds", "bsearch" if bits & 2 else "bitmap",
                         ("rows", "radix", "bitonic", "?")[(bits >> 2) & 3])


def scratch_bytes(cap):
    """coral_scratch_bytes: 48 bytes per merged point of the largest job, rounded up to 256."""
    return (cap * 48 + 255) // 256 * 256


def predict_path(n, V, dbx, dby, max_row=0):
    """The path the grid index takes for n points (CorAl: the merged cloud; P2P: the reference cloud) in V occupied cells
    of a dbx x dby grid whose fullest grid row holds max_row points: path bits, or None where both kernels refuse the
    cloud for its size or grid (CFEAR_ERR_CAPACITY; their other refusals are their own).  Mirrors the refusals at the
    top of coral_kernel / p2p_kernel and after their bounding boxes, and gridsort.hpp: the sort (grid_sort_rows_block's
    entry test and crowded-row test with max_row 512, grid_sort_is_radix); `spt_in_lds` and `bitmap` of
    grid_index_build."""
    ncells = dbx * dby
    if n > MAX_POINTS or dby > MAX_GRID_ROWS or ncells > MAX_CELLS:
        return None
    if n <= 8192 and dbx <= 65535 and max_row <= 512:
        sort = SORT_ROWS
    else:
        npad = max(1024, (n + 1023) // 1024 * 1024)
        ib = 10
        while (1 << ib) < npad:
            ib += 1
        vb = 1
        while (1 << vb) < ncells:
            vb += 1
        sort = SORT_RADIX if (npad <= 8192 and vb + ib <= 32) else SORT_BITONIC
    Vp = (V + 4) & ~3
    spt_off = (Vp * 4 + (V + 1) * 4 + 15) & ~15
    in_lds = spt_off + n * 16 <= ROWBEG_OFF
    occ_off = ((spt_off + n * 16 + 15) & ~15) if in_lds else spt_off
    bitmap = occ_off + ((ncells >> 5) + 1) * 6 + 16 <= ROWBEG_OFF
    return path_bits(not in_lds, not bitmap, sort)


def merged_points(ref, src, ref_pose, src_pose, offset=(0.0, 0.0, 0.0)):
    """(P_src, P_ref): the float32 points both sides work on (pcl::transformPointCloud rounds to float)."""
    from tests.test_oracle_coral import _compose, _tf
    return (_tf(np.asarray(src, np.float32), _compose(np.asarray(src_pose, float), np.asarray(offset, float))),
            _tf(np.asarray(ref, np.float32), np.asarray(ref_pose, float)))


def grid_of_points(P, radius=1.0):
    """The grid of both kernels over the float32 points P [n, >= 2] (cell = radius * 1.0001, float arithmetic as the
    kernels' cell functions): dict(n, V, dbx, dby, max_row) -- predict_path's arguments."""
    inv = np.float32(1.0 / (radius * 1.0001))
    bx, by = np.floor(P[:, 0] * inv), np.floor(P[:, 1] * inv)
    ix = (bx - np.float32(bx.min())).astype(np.int64)
    iy = (by - np.float32(by.min())).astype(np.int64)
    dbx, dby = int(ix.max()) + 1, int(iy.max()) + 1
    return dict(n=len(P), V=len(np.unique(iy * dbx + ix)), dbx=dbx, dby=dby, max_row=int(np.bincount(iy).max()))


def grid_of(ref, src, ref_pose, src_pose, offset=(0.0, 0.0, 0.0), radius=1.0):
    """CorAl's grid: over the merged cloud."""
    ps, pr = merged_points(ref, src, ref_pose, src_pose, offset)
    return grid_of_points(np.concatenate([ps, pr]), radius)


def grid_of_cloud(ref, radius):
    """P2P's grid: over the reference cloud alone, as it is given."""
    return grid_of_points(np.asarray(ref, np.float32), radius)


def predict(ref, src, ref_pose, src_pose, offset=(0.0, 0.0, 0.0), radius=1.0):
    return predict_path(**grid_of(ref, src, ref_pose, src_pose, offset, radius))


# ---- cloud builders: float32 [n, 4] = x, y, z (0), intensity; fixed seeds ----------------------------------------------
def _cloud(x, y, rng):
    c = np.zeros((len(x), 4), np.float32)
    c[:, 0], c[:, 1] = x, y
    c[:, 3] = rng.uniform(60, 255, len(x))
    return c


def clutter(seed, n, x0, x1, y0, y1):
    """Uniform clutter in a box."""
    rng = np.random.default_rng(seed)
    return _cloud(rng.uniform(x0, x1, n), rng.uniform(y0, y1, n), rng)


def wall(seed, n, x0, x1, y, thick=0.3):
    """A wall segment along x: n points within +-thick of the line y (more than 512 of them in one grid row make the
    two-level row sort decline)."""
    rng = np.random.default_rng(seed)
    return _cloud(rng.uniform(x0, x1, n), y + rng.uniform(-thick, thick, n), rng)


def cluster_pair(seed, n_ref, n_src, box, shift=(0.05, -0.03), jitter=0.02):
    """Two overlapping clouds over one box (x0, x1, y0, y1): the source is a resampled, shifted and jittered copy of the
    reference's points, so most points have neighbours in both clouds."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = box
    ref = _cloud(rng.uniform(x0, x1, n_ref), rng.uniform(y0, y1, n_ref), rng)
    pick = rng.integers(0, n_ref, n_src)
    src = _cloud(ref[pick, 0] + shift[0] + rng.normal(0, jitter, n_src), ref[pick, 1] + shift[1] + rng.normal(0, jitter, n_src), rng)
    return ref, src


def with_far_cluster(seed, ref, src, dx, dy=0.0, n_far=120, size=8.0):
    """Both clouds extended by a small common cluster (dx, dy) metres away: the grid grows by dx / radius columns and
    dy / radius rows, and the far points are valid too, so a wrong row table or cell start changes values, not just
    zeros."""
    fr, fs = cluster_pair(seed, n_far, n_far, (dx, dx + size, dy, dy + size))
    return np.concatenate([ref, fr]), np.concatenate([src, fs])


def points(xy, intensity=100.0):
    """A hand-placed neighbourhood: [(x, y), ...] -> cloud."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    c = np.zeros((len(xy), 4), np.float32)
    c[:, :2] = xy
    c[:, 3] = intensity
    return c


def lattice(xs, ys, step=0.25, origin=(0.0, 0.0), intensity=100.0):
    """Points origin + step * (i, j) for the given integer index lists (all pairs): with step and origin dyadic every
    coordinate, difference and squared distance is exact in float32, also a distance equal to the radius."""
    return points([(origin[0] + step * i, origin[1] + step * j) for j in ys for i in xs], intensity)


def thin_line(seed, n, length, angle, origin=(40.0, 25.0), wobble=0.0):
    """n points on a segment of the given direction, rounded to float32 (a straight wall as float represents it: the
    points leave the line by an ulp of their coordinates, a few 1e-6 m), plus an optional normal wobble."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, length, n)
    w = rng.normal(0, wobble, n) if wobble > 0 else np.zeros(n)
    c, s = math.cos(angle), math.sin(angle)
    return _cloud(origin[0] + c * t - s * w, origin[1] + s * t + c * w, rng)


# ---- per-point tolerance of the GPU comparison ------------------------------------------------------------------------
# Largest |oracle - exact_coral| over the valid points of the thin / near-collinear neighbourhoods and the crafted
# inputs of tests/test_oracle_coral.py (test_oracle_against_exact_thin_neighbourhoods re-checks them), per radius.
# Both the oracle (two-pass covariance) and the kernel (one-pass moments about the query) evaluate
# det = c00 c11 - c01^2 in fp64; its rounding error grows with radius^4 while the 1e-8 under the logarithm does not,
# so the entropy of a thin neighbourhood is uncertain by about u * radius^4 / (det + 1e-8 / (2 pi e)).  The GPU's
# tolerance at a radius is 4 x the measured value (two independent summation orders, one-pass against two-pass, and a
# factor 2 of headroom), never below the 1e-6 that tests/test_gpu_coral.py uses up to radius 1.  Measured on the CPU
# only; not tuned against what the kernel returns.
#   radius            0.3        1.0        3.0        8.0
#   measured       2.085e-10  2.135e-08  1.663e-06  2.158e-04   (worst: the float-rounded straight lines at 45 degrees;
#   tabulated       2.09e-10   2.14e-08   1.67e-06   2.16e-04    the crafted lattices at radius 1 stay below 1e-15)
#   GPU atol          1e-6       1e-6     6.68e-06   8.64e-04
ORACLE_VS_EXACT = {0.3: 2.09e-10, 1.0: 2.14e-08, 3.0: 1.67e-06, 8.0: 2.16e-04}
THIN_RADII = (0.3, 1.0, 3.0, 8.0)


def thin_inputs(radius):
    """(ref, src) pairs of thin neighbourhoods scaled to the radius: straight lines at four angles as float32 holds
    them, and lines with a normal wobble of 1e-4, 1e-3 and 1e-2 m."""
    out = []
    for k, (ang, wob) in enumerate([(0.0, 0.0), (0.3, 0.0), (math.pi / 4, 0.0), (1.2, 0.0), (0.3, 1e-4), (1.2, 1e-3), (0.5, 1e-2)]):
        out.append((thin_line(100 + k, 90, 6.0 * radius, ang, wobble=wob), thin_line(200 + k, 80, 6.0 * radius, ang, wobble=wob)))
    return out


def per_point_atol(radius):
    """atol for a per-point entropy at this radius: 4 x the measured oracle error at the smallest tabulated radius
    >= radius, at least 1e-6."""
    for r in sorted(ORACLE_VS_EXACT):
        if radius <= r:
            return max(1e-6, 4.0 * ORACLE_VS_EXACT[r])
    raise ValueError("no tolerance measured beyond radius %g" % max(ORACLE_VS_EXACT))


# ---- exact restatement ---------------------------------------------------------------------------------------------------
_K = Fraction(2.0 * math.pi * math.exp(1.0))           # the doubles the reference's expression holds, as rationals
_EPS = Fraction(0.00000001)
_U = Fraction(1, 2 ** 53)


def _half_log(arg):
    with localcontext() as ctx:
        ctx.prec = 50
        return float((Decimal(arg.numerator) / Decimal(arg.denominator)).ln() / 2)


def _exact_entropy(pts, q):
    """pts: list of (Fraction x, Fraction y), more than 2 -> (1/2 log(2 pi e det + 1e-8), validity is rounding-dependent)."""
    n = len(pts)
    mx, my = sum(p[0] for p in pts) / n, sum(p[1] for p in pts) / n
    den = n - 1                                        # float(n) - 1.0 is exact for n < 2^24
    c00 = sum((p[0] - mx) ** 2 for p in pts) / den
    c01 = sum((p[0] - mx) * (p[1] - my) for p in pts) / den
    c11 = sum((p[1] - my) ** 2 for p in pts) / den
    arg = _K * (c00 * c11 - c01 * c01) + _EPS           # det >= 0 exactly (Cauchy-Schwarz), so arg >= 1e-8
    # An fp64 evaluation may still see arg <= 0 (NaN: the point turns invalid) when the rounding error of the
    # determinant reaches arg.  The second moments about the query bound every intermediate of the two-pass and of the
    # one-pass form; each of the ~n + 8 operations behind a covariance entry adds at most one unit roundoff u, and the
    # determinant has two products of two entries.
    q00 = sum((p[0] - q[0]) ** 2 for p in pts) / den
    q11 = sum((p[1] - q[1]) ** 2 for p in pts) / den
    bound = 4 * (n + 8) * _U * _K * q00 * q11
    return _half_log(arg), arg <= 4 * bound


def exact_coral(ref, src, ref_pose, src_pose, offset=(0.0, 0.0, 0.0), radius=1.0, weight=False):
    """CorAlRadarQuality with exact covariances.  The float32 transformed points and the float32 distance test
    d2 < float(r * r) are part of the definition (tests/test_oracle_coral.py::_tf, _numpy_coral); mean, covariance and
    determinant are exact rationals; only 1/2 log(.) is rounded (50 digits, then to double).  O(n^2) in Python: a few
    hundred points at most.  -> dict(joint [n], sep [n], valid [n] bool, marginal [n] bool: validity depends on
    rounding, quality [joint, sep, overlap], ok, count_valid); per-point values carry the intensity weight like the
    oracle's, source points first."""
    ps, pr = merged_points(ref, src, ref_pose, src_pose, offset)
    inten = np.concatenate([np.asarray(src, np.float32)[:, 3], np.asarray(ref, np.float32)[:, 3]]).astype(np.float64)
    r2 = np.float32(radius * radius)
    n_src, n = len(ps), len(ps) + len(pr)
    fs = [(Fraction(float(x)), Fraction(float(y))) for x, y in ps]
    fr = [(Fraction(float(x)), Fraction(float(y))) for x, y in pr]
    joint, sep = np.full(n, 100.0), np.full(n, 100.0)
    valid, marginal = np.zeros(n, bool), np.zeros(n, bool)

    def near(P, q):
        dx, dy = q[0] - P[:, 0], q[1] - P[:, 1]                  # float32 throughout, as FLANN's L2_Simple
        return np.nonzero(dx * dx + dy * dy < r2)[0]
    for idx in range(n):
        is_src = idx < n_src
        q = ps[idx] if is_src else pr[idx - n_src]
        i_s, i_r = near(ps, q), near(pr, q)
        if len(i_r if is_src else i_s) < 1:                        # overlap_req_ = 1
            continue
        own = [fs[i] for i in i_s] if is_src else [fr[i] for i in i_r]
        both = [fs[i] for i in i_s] + [fr[i] for i in i_r]
        if len(own) <= 2 or len(both) <= 2:
            continue
        fq = (Fraction(float(q[0])), Fraction(float(q[1])))
        es, m_s = _exact_entropy(own, fq)
        ej, m_j = _exact_entropy(both, fq)
        w = inten[idx] if weight else 1.0
        sep[idx], joint[idx], valid[idx], marginal[idx] = w * es, w * ej, True, m_s or m_j
    cnt = int(valid.sum())
    w_sum = float(inten[valid].sum()) if weight else float(cnt)
    quality = np.array([math.fsum(joint[valid]) / w_sum if cnt else 0.0, math.fsum(sep[valid]) / w_sum if cnt else 0.0, cnt / n])
    return dict(joint=joint, sep=sep, valid=valid, marginal=marginal, quality=quality, ok=cnt / n >= 0.1, count_valid=cnt)


# ---- the crafted neighbourhoods of the edge tests (radius 1, dyadic coordinates): name -> (ref, src) ---------------------
def _at_radius(sign, axis, inside):
    """A source triple around the origin and a reference triple whose nearest point is exactly 1 m from the source's
    middle point (excluded: d2 < r^2 is strict) or one float ulp inside (included); nothing else is within reach.
    sign / axis move the reference into the neighbouring grid cell to the left, right, below or above."""
    d = float(np.nextafter(np.float32(1.0), np.float32(0.0))) if inside else 1.0
    s = [(0.0, 0.0), (0.0, 0.25), (0.0, -0.25)]
    r = [(sign * d, 0.0), (sign * 1.25, 0.25), (sign * 1.25, -0.25)]
    if axis == "y":
        s, r = [(y, x) for x, y in s], [(y, x) for x, y in r]
    return points(r), points(s)


def edge_cases():
    out = {}
    # a source triple with one reference point (own 3, joint 4: the reference point's own set is 1, its joint set 4)
    # and, 16 m away, a source pair in a reference triple (own 2: invalid; the triple's points: own 3)
    out["own_2_and_3"] = (points([(0.25, 0.25), (16.0, 0.0), (16.25, 0.25), (16.5, 0.0)]),
                          points([(0.0, 0.0), (0.25, 0.0), (0.5, 0.25), (16.25, 0.0), (16.0, 0.25)]))
    for sign, sn in ((1.0, "p"), (-1.0, "m")):
        for axis in "xy":
            out["at_radius_%s%s" % (sn, axis)] = _at_radius(sign, axis, False)
            out["inside_radius_%s%s" % (sn, axis)] = _at_radius(sign, axis, True)
    # 13 x 13 lattice of step 0.25 (3 m square: many pairs exactly 1 m apart) against itself shifted by 1/8: queries in
    # the first and last grid row and column, whose 3 x 3 block leaves the grid
    out["lattice_borders"] = (lattice(range(13), range(13)), lattice(range(13), range(13), origin=(0.125, 0.125)))
    out["one_cell"] = (lattice(range(3), range(3), origin=(0.125, 0.125)), lattice(range(3), range(3), origin=(0.1875, 0.1875)))
    out["one_grid_row"] = (lattice(range(40), range(3), origin=(0.125, 0.125)), lattice(range(40), range(3), origin=(0.1875, 0.1875)))
    out["one_grid_column"] = (lattice(range(3), range(40), origin=(0.125, 0.125)), lattice(range(3), range(40), origin=(0.1875, 0.1875)))
    # duplicates: every covariance is exactly zero -> entropy 1/2 log(1e-8)
    out["duplicates"] = (points([(2.0, 3.0)] * 3), points([(2.0, 3.0)] * 4))
    out["single_source_point"] = (lattice(range(5), range(5)), points([(0.375, 0.375)]))
    return out


# ---- the path matrix: name -> (ref, src, wanted path bits), radius 1, identity poses ----------------------------------------
def _find_far(seed, ref, src, want, dy, dxs):
    """The first far-cluster distance of dxs at which predict() gives the wanted bits (the window in which a radix sort
    meets a binary-search lookup is a few per cent of the grid size wide)."""
    z = np.zeros(3)
    for dx in dxs:
        r, s = with_far_cluster(seed, ref, src, float(dx), dy)
        if predict(r, s, z, z) == want:
            return r, s
    raise AssertionError("no far-cluster distance gives " + describe(want))


def _trim_to_lds_edge(ref, src):
    """(src prefix that still keeps the sorted points in LDS, the prefix one point longer that does not)."""
    z = np.zeros(3)
    lo, hi = 1, len(src)                               # spt_off + 16 n grows with every point: one boundary
    assert not predict(ref, src[:lo], z, z) & PATH_SCRATCH and predict(ref, src, z, z) & PATH_SCRATCH
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if predict(ref, src[:mid], z, z) & PATH_SCRATCH:
            hi = mid
        else:
            lo = mid
    return src[:lo], src[:hi]


def matrix_jobs():
    """One job at least for every {LDS, scratch} x {bitmap, binary search} combination and every sort that can occur
    with it (LDS + bitmap + bitonic cannot: a bitonic sort needs more than 8192 points, which do not fit the LDS, or
    more than 2^19 cells, which do not fit the bitmap)."""
    B = path_bits
    out = {}
    small = cluster_pair(1, 1000, 1000, (0, 25, 0, 25))                                  # 2000 points, 26 x 26 cells
    crowd = [np.concatenate([c, wall(2 + k, 620, 0, 25, 12.0 + 0.05 * k)]) for k, c in enumerate(small)]
    big = cluster_pair(3, 3900, 3900, (0, 60, 0, 60))                                    # 7800 points: scratch
    big_crowd = [np.concatenate([c[:3500], wall(4 + k, 400, 0, 60, 30.0 + 0.05 * k, thick=0.2)]) for k, c in enumerate(big)]
    huge = cluster_pair(5, 8192, 8192, (0, 75, 0, 75))                                   # n = 16384 exactly
    # many occupied cells (isolated clutter) with a dense pair and a crowded row: the only way to a radix sort (at most
    # 2^19 cells) whose grid still does not fit the bitmap behind a large cell table
    dense = cluster_pair(6, 1400, 1400, (0, 25, 0, 25))
    sparse_crowd = [np.concatenate([c, clutter(7 + k, 2100, 0, 200, 0, 200), wall(9 + k, 330, 0, 90, 100.5 + 0.05 * k, thick=0.2)])
                    for k, c in enumerate(dense)]
    out["lds_bitmap_rows"] = (*small, B(0, 0, SORT_ROWS))
    out["lds_bitmap_radix"] = (*crowd, B(0, 0, SORT_RADIX))
    out["lds_bsearch_rows"] = (*with_far_cluster(10, *small, 3000.0, 400.0), B(0, 1, SORT_ROWS))
    out["lds_bsearch_radix"] = (*with_far_cluster(11, *crowd, 3000.0, 200.0), B(0, 1, SORT_RADIX))
    out["lds_bsearch_bitonic"] = (*with_far_cluster(12, *crowd, 3000.0, 400.0), B(0, 1, SORT_BITONIC))
    out["scratch_bitmap_rows"] = (*big, B(1, 0, SORT_ROWS))
    out["scratch_bitmap_radix"] = (*big_crowd, B(1, 0, SORT_RADIX))
    out["scratch_bitmap_bitonic_16384"] = (*huge, B(1, 0, SORT_BITONIC))
    out["scratch_bsearch_rows"] = (*with_far_cluster(13, *big, 3000.0, 400.0), B(1, 1, SORT_ROWS))
    out["scratch_bsearch_radix"] = (*_find_far(14, *sparse_crowd, B(1, 1, SORT_RADIX), 50.0, range(2300, 2800, 10)), B(1, 1, SORT_RADIX))
    out["scratch_bsearch_bitonic"] = (*with_far_cluster(15, *cluster_pair(16, 4600, 4500, (0, 60, 0, 60)), 3000.0, 400.0), B(1, 1, SORT_BITONIC))
    # the sizes on either side of the spt_in_lds boundary
    mid = cluster_pair(17, 3400, 4200, (0, 50, 0, 50))
    s_lds, s_scr = _trim_to_lds_edge(*mid)
    out["lds_edge"] = (mid[0], s_lds, B(0, 1, SORT_ROWS))           # the LDS is full: no room for the bitmap of a 51 x 50 grid
    out["scratch_edge"] = (mid[0], s_scr, B(1, 0, SORT_ROWS))
    # 2^10 points in 2^22 cells, a crowded row, and the LAST point alone with its neighbours in the LAST cell: the radix
    # sort's key of that point is all ones, the value its padding has
    k_ref = np.concatenate([wall(20, 330, 0, 60, 0.5, thick=0.2), points([(2047.3, 2047.3), (2047.5, 2047.4), (2047.4, 2047.6), (2047.6, 2047.5)])])
    k_src = np.concatenate([wall(21, 686, 0, 60, 0.55, thick=0.2), points([(2047.35, 2047.3), (2047.5, 2047.45), (2047.45, 2047.6), (2047.62, 2047.52)])])
    out["radix_all_ones_key"] = (k_ref, k_src, B(0, 1, SORT_RADIX))
    return out
