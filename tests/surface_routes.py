"""Surface-point test geometries and the helpers the route tests share: the route word's constants, a host-side
restatement of the thresholds by which the surface kernels (tbv_slam_public_amd/csrc/surface.hip) pick a route -- used
ONLY to choose inputs and to guard which branch a case runs on; the tests assert the word the kernels report
(cfear_scan_surface_path) and judge correctness against the CPU oracle alone -- the cell comparison every surface test
uses, and cloud builders with fixed seeds."""
import numpy as np

# ---- the route word (include/cfear_hip.h: CFEAR_SURF_PATH_*) ---------------------------------------------------------------
KIND_MASK, FAST, SINGLE, GLOBAL = 3, 1, 2, 3
ROWS, K64, WFLOAT, SLABS, READ2 = 0x4, 0x8, 0x10, 0x20, 0x40
TIER16, TIER4, TIER1, TOP_BUCKET, CEN_SCRATCH = 0x80, 0x100, 0x200, 0x400, 0x800
PREPARED, REASON_SHIFT, REASON_MASK = 0x1000, 13, 0xE000
REASON_REACH, REASON_ROTATION, REASON_POINTS, REASON_CELLS, REASON_ORDER, REASON_ROWS3 = 1, 2, 3, 4, 5, 6
SLAB_COUNT_SHIFT, SLAB_COUNT_MASK = 16, 0xFF0000
REASONS = {0: "-", 1: "reach", 2: "rotation", 3: "points", 4: "cells", 5: "order", 6: "rows3"}
# every bit and field value a test can see: name -> predicate on a route word (the coverage test lists them)
FEATURES = {
    "fast": lambda p: p & KIND_MASK == FAST, "single": lambda p: p & KIND_MASK == SINGLE, "global": lambda p: p & KIND_MASK == GLOBAL,
    "rows": lambda p: bool(p & ROWS), "k32": lambda p: p & KIND_MASK == FAST and not p & K64, "k64": lambda p: bool(p & K64),
    "wbyte": lambda p: p & KIND_MASK == FAST and not p & WFLOAT, "wfloat": lambda p: bool(p & WFLOAT),
    "one_slab": lambda p: p & KIND_MASK == FAST and not p & SLABS, "slabs": lambda p: bool(p & SLABS), "read2": lambda p: bool(p & READ2),
    "tier16": lambda p: bool(p & TIER16), "tier4": lambda p: bool(p & TIER4), "tier1": lambda p: bool(p & TIER1),
    "top_bucket": lambda p: bool(p & TOP_BUCKET), "cen_scratch": lambda p: bool(p & CEN_SCRATCH),
    "prepared": lambda p: bool(p & PREPARED), "unprepared": lambda p: p & KIND_MASK != FAST and p != 0 and not p & PREPARED,
}
for _r in range(1, 7):
    FEATURES["reason_" + REASONS[_r]] = (lambda r: lambda p: (p & REASON_MASK) >> REASON_SHIFT == r)(_r)

# ---- the kernels' limits ------------------------------------------------------------------------------------------------
MAX_POINTS = 16384                     # kMaxPoints: the LDS sort of the single-kernel path; 32 points per thread of the fast one
FAST_MAX_POINTS = 32768                # kFastMaxPoints
FAST_MAX_CELLS = 1 << 18               # kFastMaxCells
MAX_GRID_ROWS = 4096                   # kMaxGridRows
FAST_BUDGET = 78 * 1024 - 512          # kFastLds - 512
SLAB_VOXELS = 2048                     # kSlabVoxels = 4 * kFastThreads


def describe(path):
    if path is None:
        return "refused"
    kind = ("none", "fast", "single", "global")[path & KIND_MASK]
    out = [kind]
    if path & ROWS:
        out.append("rows")
    if path & KIND_MASK == FAST:
        out += ["k64" if path & K64 else "k32", "wfloat" if path & WFLOAT else "wbyte",
                "slabs=%d" % ((path & SLAB_COUNT_MASK) >> SLAB_COUNT_SHIFT)]
        out += [n for b, n in ((READ2, "read2"), (TIER16, "t16"), (TIER4, "t4"), (TIER1, "t1"), (TOP_BUCKET, "top"), (CEN_SCRATCH, "cen-scratch")) if path & b]
    elif kind != "none":
        out += ["reason=" + REASONS[(path & REASON_MASK) >> REASON_SHIFT], "prepared" if path & PREPARED else "unprepared"]
    return "/".join(out)


def _al16(b):
    return (b + 15) & ~15


def layout(cloud, radius=3.0, factor=1.0):
    """The voxel grid the kernels (and pcl::VoxelGrid) put over a cloud, in their float arithmetic, and the sorted layout:
    dict(n, reach, dbx, dby, ncells, V, cell [n] (cell of every point), vcell [V] (occupied cells ascending), count [V],
    start [V + 1] (position of every voxel's run in the sorted array), cand [V] (points in the 3 x 3 block around it))."""
    cloud = np.asarray(cloud, np.float32)
    leaf = np.float32(float(np.float32(radius)) / float(factor))
    inv = np.float32(1.0) / leaf
    reach = max(1, int(np.ceil(float(np.float32(radius)) / float(leaf))))
    bx, by = np.floor(cloud[:, 0] * inv), np.floor(cloud[:, 1] * inv)
    ix = (bx - np.float32(int(bx.min()))).astype(np.int64)
    iy = (by - np.float32(int(by.min()))).astype(np.int64)
    dbx, dby = int(bx.max()) - int(bx.min()) + 1, int(by.max()) - int(by.min()) + 1
    cell = iy * dbx + ix
    vcell, count = np.unique(cell, return_counts=True)
    start = np.concatenate([[0], np.cumsum(count)])
    cand = None
    if dbx * dby <= FAST_MAX_CELLS:
        g = np.zeros((dby + 2, dbx + 2), np.int64)
        g[vcell // dbx + 1, vcell % dbx + 1] = count
        s = sum(g[1 + dy:dby + 1 + dy, 1 + dx:dbx + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
        cand = s[vcell // dbx, vcell % dbx]
    return dict(n=len(cloud), reach=reach, dbx=dbx, dby=dby, ncells=dbx * dby, V=len(vcell), cell=cell, vcell=vcell,
                count=count, start=start, cand=cand)


def _handed(n, reason, prepared, rows):
    kind = GLOBAL if n > MAX_POINTS else SINGLE
    return kind | (ROWS if rows else 0) | (reason << REASON_SHIFT) | (PREPARED if prepared else 0)


def predict(cloud, radius=3.0, factor=1.0, rotation=None, rows=False):
    """The route word the kernels report for this cloud (the cloud as the grid sees it: after compensation), or None where
    they refuse it (CFEAR_ERR_CAPACITY).  rotation: mot[2] of a requested compensation.  Mirrors surface.hip:
    surface_prep_kernel's hand-overs, then surface_sort_job's LDS budget, slab fit and tier split."""
    cloud = np.asarray(cloud, np.float32)
    L = layout(cloud, radius, factor)
    n, dbx, dby, ncells, V = L["n"], L["dbx"], L["dby"], L["ncells"], L["V"]
    refused = ncells > 0x7fffffff or dby > MAX_GRID_ROWS
    if L["reach"] != 1:
        return None if refused else _handed(n, REASON_REACH, False, rows)
    if rotation is not None and not abs(rotation) <= 1e5:
        return None if refused else _handed(n, REASON_ROTATION, False, rows)
    if n > FAST_MAX_POINTS:
        return None if refused else _handed(n, REASON_POINTS, False, rows)
    if refused:
        return None
    if ncells > FAST_MAX_CELLS:
        return _handed(n, REASON_CELLS, True, rows)
    nw32 = (ncells >> 5) + 1
    ord_bytes = _al16(nw32 * 6)
    ord2_off = ord_bytes + _al16((V + 2) * 2)
    if ord2_off + _al16(n * 2) > FAST_BUDGET:
        return _handed(n, REASON_ORDER, True, rows)
    w = np.maximum(cloud[:, 3] - np.float32(60.0), np.float32(0.0))
    wbyte = bool(np.all((w <= 255.0) & (w == np.trunc(w))))
    pb = 9 if wbyte else 12
    avail = FAST_BUDGET - ord2_off
    single = V <= SLAB_VOXELS and ((n + 3) & ~3) * pb + V * 6 + 48 <= avail
    path = FAST | (ROWS if rows else 0) | (K64 if n > MAX_POINTS else 0) | (0 if wbyte else WFLOAT) | (READ2 if ncells > 65536 else 0)
    vcell, start, cand = L["vcell"], L["start"], L["cand"]

    def o(c):                                              # occupied cells before cell c
        return int(np.searchsorted(vcell, c, "left"))

    def pbefore(c):                                        # points in cells < c
        return int(start[o(c)])
    kb = np.where(cand >= 6, np.minimum(12, np.frexp(np.maximum(cand - 1, 0).astype(np.float64))[1]), 0)   # bucket = bit length of C - 1
    slabs, ya = 0, 0
    while ya < dby:
        p0 = 0 if single else pbefore(max(ya - 1, 0) * dbx)
        vbeg = 0 if single else o(ya * dbx)

        def fits(yb):
            npts, nv = pbefore(min(yb + 1, dby) * dbx) - p0, o(yb * dbx) - vbeg
            return nv <= SLAB_VOXELS and ((npts + 3) & ~3) * pb + nv * 6 + 48 <= avail
        lo, hi = (dby, dby) if single else (ya + 1, dby)
        if not single and not fits(lo):
            return _handed(n, REASON_ROWS3, True, rows)
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if fits(mid):
                lo = mid
            else:
                hi = mid - 1
        yb = lo
        p1 = n if single else pbefore(min(yb + 1, dby) * dbx)
        vend = V if single else o(yb * dbx)
        cap_pts = (p1 - p0 + 3) & ~3
        nv = vend - vbeg
        cen_o = (ord2_off + _al16(cap_pts * pb) + _al16(nv * 2) + nv * 4 + 7) & ~7
        cen_cap = (FAST_BUDGET - cen_o) // 8 if cen_o < FAST_BUDGET else 0
        k, c = kb[vbeg:vend], cand[vbeg:vend]
        n16, n4, nlist = int((k >= 7).sum()), int((k >= 5).sum()), int((k >= 3).sum())
        path |= (TIER16 if n16 else 0) | (TIER4 if n4 > n16 else 0) | (TIER1 if nlist > n4 else 0)
        path |= (TOP_BUCKET if (c > 4096).any() else 0) | (CEN_SCRATCH if n4 > cen_cap else 0)
        slabs += 1
        ya = yb
    return path | (SLABS if slabs > 1 else 0) | (min(slabs, 255) << SLAB_COUNT_SHIFT)


# ---- the comparison every surface test uses ------------------------------------------------------------------------------
def cmp_cells(got, exp):
    assert got.shape[0] == exp.shape[0]
    np.testing.assert_array_equal(got["nsamples"], exp["nsamples"])
    # fp64 sums are reduced in a different (tree) order on the GPU: rounding-level differences only
    np.testing.assert_allclose(got["mean"], exp["mean"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(got["cov"], exp["cov"], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(got["normal"], exp["normal"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got["scale"], exp["scale"], rtol=1e-8)
    np.testing.assert_allclose(got["avg_intensity"], exp["avg_intensity"], rtol=1e-12)
    np.testing.assert_allclose(got["lambda_min"], exp["lambda_min"], rtol=1e-8, atol=1e-12)


# ---- cloud builders: float32 [n, 4] = x, y, z (0), intensity (integers in 61..255 unless stated); fixed seeds -----------------
def _cloud(x, y, rng, intensity=None):
    c = np.zeros((len(x), 4), np.float32)
    c[:, 0], c[:, 1] = x, y
    c[:, 3] = rng.integers(61, 256, len(x)) if intensity is None else intensity
    return c


def uniform(seed, n, side_x, side_y=None, x0=0.0, y0=0.0):
    """n points uniform in a box of side_x x side_y metres whose lower corner is (x0, y0)."""
    rng = np.random.default_rng(seed)
    return _cloud(x0 + rng.uniform(0, side_x, n), y0 + rng.uniform(0, side_y or side_x, n), rng)


def walls(seed, n, side, x0=0.0, y0=0.0):
    """A dense scan: 80 % of the points along 40 wall segments (0.15 m noise), the rest clutter, in a side x side box."""
    rng = np.random.default_rng(seed)
    s = side / 240.0
    seg = rng.integers(0, 40, n)
    a0 = rng.uniform(0, 2 * np.pi, 40)[seg]
    d0 = (rng.uniform(10, 110, 40) * s)[seg]
    t = rng.uniform(-25, 25, n) * s
    wall = np.stack([d0 * np.cos(a0) - t * np.sin(a0), d0 * np.sin(a0) + t * np.cos(a0)], 1) + rng.normal(0, 0.15, (n, 2))
    clutter = rng.uniform(-side / 2, side / 2, (n, 2))
    xy = np.clip(np.where((rng.random(n) < 0.8)[:, None], wall, clutter), -side / 2, side / 2) + side / 2
    return _cloud(x0 + xy[:, 0], y0 + xy[:, 1], rng)


def blob(seed, n, cx, cy, spread=0.6):
    """n points clustered inside the 3 m voxel whose lower corner is (cx, cy)."""
    rng = np.random.default_rng(seed)
    return _cloud(cx + 1.5 + rng.uniform(-spread, spread, n), cy + 1.5 + rng.uniform(-spread, spread, n), rng)


def order_blocks(seed, pad=None):
    """The cloud whose cells depend on the order of the points inside a voxel: 24 blocks near x = 1000 m (a float ulp is
    6e-5 m there), each 9 - 39 random points inside one 3 m voxel and, in the neighbouring voxel, a ladder of 41 points at
    centroid.x + 3 + j ulp, j = -20 .. 20 -- which of them lie inside the radius depends on the last bit of the float
    centroid, a sequential sum in input order.  pad: more points (kept 9 m away by the caller) to reach a route.  Shuffled.
    Asserts that the oracle of the reversed cloud differs in nsamples in at least 5 cells."""
    from oracle import pyoracle as O
    rng = np.random.default_rng(seed)
    parts = []
    for b in range(24):
        vx, vy = 3.0 * 333, 3.0 * 4 * b                    # blocks four voxels apart: no common neighbours
        m = int(rng.integers(9, 40))
        pts = _cloud(vx + rng.uniform(0.2, 2.8, m), vy + rng.uniform(0.2, 2.8, m), rng)
        c = pts[:, :2].astype(np.float64).mean(0).astype(np.float32)
        lx = np.float32(c[0] + np.float32(3.0))
        ulp = np.spacing(lx)
        ladder = _cloud(lx + np.arange(-20, 21).astype(np.float32) * ulp, np.full(41, c[1], np.float32), rng)
        parts += [pts, ladder]
    cloud = np.concatenate(parts + ([pad] if pad is not None else []))
    cloud = cloud[rng.permutation(len(cloud))]
    fwd = O.surface_points(cloud, 3.0, 1.0, (0, 0), True)
    rev = O.surface_points(cloud[::-1], 3.0, 1.0, (0, 0), True)
    assert fwd.shape == rev.shape
    changed = int((fwd["nsamples"] != rev["nsamples"]).sum())
    assert changed >= 5, "the fixture no longer sees the in-voxel order: %d cells differ" % changed
    return cloud


def run_lengths(seed):
    """Voxel runs of every length 1 .. 40 at every start offset mod 8 of the sorted array (the rank pass reads sixteen
    indices per trip from the 16-byte boundary below a run and masks the rest): a dense block of voxels, 14 per grid row,
    whose point counts are chosen so; asserts the coverage with layout()."""
    rng = np.random.default_rng(seed)
    want = {(ln, o) for ln in range(1, 41) for o in range(8)}
    lengths, pos = [], 0
    while want:
        o = pos & 7
        todo = sorted(ln for ln, oo in want if oo == o)
        ln = todo[0] if todo else 1
        want.discard((ln, o))
        lengths.append(ln)
        pos += ln
    parts = []
    for i, ln in enumerate(lengths):
        vx, vy = 3.0 * (i % 14), 3.0 * (i // 14)
        parts.append(_cloud(vx + rng.uniform(0.1, 2.9, ln), vy + rng.uniform(0.1, 2.9, ln), rng))
    cloud = np.concatenate(parts)
    cloud = cloud[rng.permutation(len(cloud))]
    L = layout(cloud)
    seen = {(int(c), int(s) & 7) for c, s in zip(L["count"], L["start"][:-1])}
    assert {(ln, o) for ln in range(1, 41) for o in range(8)} <= seen
    return cloud
