"""The k-strongest matrix: one small input per kstrongest_rows_kernel<NCHUNK, VEC, MASK> instantiation and per selection
path of kstrong_row (tbv_slam_public_amd/csrc/kstrong.hip), shared by tests/test_kstrong_plan_cpu.py (every case reaches the
instantiation it names: cfear_kstrong_plan, no GPU; every row reaches the path it names; the model below equals the oracle)
and tests/test_gpu_kstrong_matrix.py (every case equals the oracle bit for bit on the strided view).

Two statements of the selection paths, kept apart on purpose:
  named_path(row, k, z_min)   the table of the paths by their CONDITIONS, from counts of the row alone
  row_path(row, k, z_min)     the branch decisions of kstrong_row in its own order, bracketing trials included, and the keys
                              each branch keeps
A row's recipe is labelled with named_path when the table below is built; the CPU test asserts that row_path takes that path
and keeps the oracle's keys -- which is what entitles the model to speak for the kernel.

  path                     condition (n_ge = bins >= uchar(z_min), T = the k-th largest intensity)
  le64                     n_ge <= 64: one candidate per lane
  loop                     64 < n_ge <= k: per-lane loops (needs k >= 65)
  hist_list                64 < n_ge <= 256, n_ge > k, at most 64 bins >= T
  hist+tiescan             the same with more than 64 bins >= T (a plateau at the cut, or k > 64)
  bracket+hist_list        n_ge > 256 and some threshold passes between k and 256 bins; then as above
  bracket+hist+tiescan     likewise
  bracket+tiescan_exact    n_ge > 256 and no threshold passes between k and 256 bins: two neighbouring thresholds bracket k
                           (always when k > 256)"""
import collections
import zlib

import numpy as np

PATHS = ("le64", "loop", "hist_list", "hist+tiescan", "bracket+hist_list", "bracket+hist+tiescan", "bracket+tiescan_exact")
DENSE_PATHS = PATHS[2:]
NCHUNKS = (1, 2, 4, 8)
K_FEW = (12, 65, 300)                                         # every instantiation
K_ALL = (1, 12, 40, 64, 65, 101, 256, 257, 300, 1024)        # one NCHUNK 1 and one NCHUNK 4 layout
Z_MASK = (0, 0.9, 256)                                        # uchar((int)z_min) == 0
Z_PLAIN = (1, 60, 127, 128, 200, 255, -1, 300)                # 255 and -1: every candidate is 255; 300 -> 44
NARROW = (1, 5, 7, 10, 15, 17)
RANGE_RES = 0.0438


def u_zmin(z_min):
    """radar_driver.cpp:58 and radar_filters.cpp:212: float -> int (toward zero) -> uchar."""
    return int(np.float32(z_min)) & 255


def table_index(nchunk, vec, mask):
    """The dispatch entry as include/cfear_hip.h documents it."""
    return 4 * NCHUNKS.index(nchunk) + 2 * int(bool(vec)) + int(bool(mask))


def entry_name(i):
    return "rows<%d,%s,%s>" % (NCHUNKS[i // 4], "vec" if i & 2 else "bytes", "mask" if i & 1 else "plain")


# ---- the two statements of the paths -----------------------------------------------------------------------------------------
def _keys(row, sel):
    pos = np.flatnonzero(sel)
    return np.sort((row[pos].astype(np.uint32) << 24) | pos.astype(np.uint32))


def named_path(row, k, z_min):
    uz = u_zmin(z_min)
    ge = np.cumsum(np.bincount(row, minlength=256)[::-1])[::-1]          # ge[t] = bins >= t
    n_ge = int(ge[uz])
    if n_ge <= 64:
        return "le64"
    if n_ge <= k:
        return "loop"
    pre = ""
    if n_ge > 256:
        if not any(k <= ge[t] <= 256 for t in range(uz + 1, 256)):
            return "bracket+tiescan_exact"
        pre = "bracket+"
    T = max(t for t in range(uz, 256) if ge[t] >= k)
    return pre + ("hist_list" if ge[T] <= 64 else "hist+tiescan")


def row_path(row, k, z_min, parent_order=False):
    """(path, kept keys ascending, cut intensity T or None) as kstrong_row decides them.  keys = intensity << 24 | bin.
    parent_order: the bracketing loop's comparison order before the fix ("> 256" tested before "< k"), to show what it did."""
    uz = u_zmin(z_min)
    row = np.asarray(row, np.uint8)
    n_ge = int((row >= uz).sum())
    if n_ge <= k or n_ge <= 64:                      # every candidate becomes a key; the ranking keeps the k largest
        return ("le64" if n_ge <= 64 else "loop"), _keys(row, row >= uz)[-k:], None
    pre, thr, n_c, exact = "", uz, n_ge, False
    T = n_gt = n_eq = 0
    if n_ge > 256:
        pre = "bracket+"
        lo, c_lo, hi, c_hi, first = uz, n_ge, 256, 0, True
        while hi - lo > 1:
            mid = 256 - max(1, ((256 - lo) * 128) // c_lo) if first else (lo + hi) >> 1
            mid = min(max(mid, lo + 1), hi - 1)
            first = False
            cnt = int((row >= mid).sum())
            below, above = cnt < k, cnt > 256
            if parent_order and above:
                below = False
            if below:
                hi, c_hi = mid, cnt
            elif above:
                lo, c_lo = mid, cnt
            else:
                thr, n_c = mid, cnt
                break
        if n_c > 256:
            exact, T, n_gt, n_eq = True, lo, c_hi, c_lo - c_hi
    if not exact:                                    # histogram of the n_c <= 256 keys >= thr
        hist = np.bincount(row[row >= thr], minlength=256)
        cum = 0
        for T in range(255, -1, -1):
            if cum + hist[T] >= k:
                n_gt, n_eq = cum, int(hist[T])
                break
            cum += int(hist[T])
        if n_gt + n_eq <= 64:                        # the keys >= T, cut by rank
            return pre + "hist_list", _keys(row, row >= T)[-k:], T
        path = pre + "hist+tiescan"
    else:
        path = "bracket+tiescan_exact"
    skip_eq = n_eq - (k - n_gt)                      # the lowest-range ties go
    eq = np.flatnonzero(row == T)
    sel = row > T
    sel[eq[max(skip_eq, 0):]] = True
    return path, _keys(row, sel), T


# ---- row recipes ------------------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "kind n path")            # path: named_path of the row in image 0


def _fill(rng, cols, uz):
    """Bins below the threshold: random, every seventh exactly uz - 1 (an off-by-one compare would keep it)."""
    if uz == 0:
        return np.zeros(cols, np.uint8)
    bg = rng.integers(0, uz, cols).astype(np.uint8)
    bg[::7] = uz - 1
    return bg


def _ends(cols):
    """Bins of 255 in the random and plateau rows: the border bins 1 and cols - 1 (the latter in the row's last 16-byte piece),
    bins 3 and cols - 4, whose peak scores read the three bytes before and after the row, and the middle."""
    return np.unique(np.clip([1, 3, cols // 2, cols - 4, cols - 1], 0, cols - 1))


def make_row(kind, n, cols, uz, rng):
    n = min(n, cols)
    if kind == "empty":                              # nothing >= z_min (z_min = 0: a plateau of zeros, every bin a candidate)
        return _fill(rng, cols, uz)
    if kind == "last_bin":
        row = _fill(rng, cols, uz)
        row[cols - 1] = max(uz, 1)
        return row
    if kind == "wall":                               # n adjacent candidates: one lane owns several 16-byte pieces of them
        row = _fill(rng, cols, uz)
        start = int(rng.integers(0, cols - n + 1))
        row[start:start + n] = rng.integers(uz, 256, n)
        return row
    if kind == "arange":
        return (np.arange(cols) % 256).astype(np.uint8)
    row = _fill(rng, cols, uz)
    ends = _ends(cols)
    others = np.setdiff1d(np.arange(cols), ends)
    bins = np.concatenate([ends, rng.permutation(others)[:max(n - ends.size, 0)]])[:n]
    if kind == "random":                             # n candidates at random bins, random intensities >= z_min, 255 at the ends
        row[bins] = rng.integers(uz, 256, bins.size)
        row[ends[:n]] = 255
    elif kind == "plateau":                          # n bins of one intensity, the (five) end bins of them at 255 above it
        row[bins] = uz + (255 - uz) // 3
        row[ends[:n]] = 255
    elif kind == "plateau255":                       # thr_gt = 256: nothing lies above the cut
        row[bins] = 255
    else:
        raise ValueError(kind)
    return row


COUNTS = (65, 200, 256, 257, 1 << 20)                 # (the last: cols of them)


def _recipes(cols):
    if cols < 64:
        return [("random", cols), ("empty", 0), ("last_bin", 1), ("plateau", cols), ("plateau255", cols), ("arange", cols), ("random", cols)]
    r = [("random", 65)]                             # first and last row: candidates in the row's last 16-byte piece
    r += [("empty", 0), ("last_bin", 1), ("wall", 64)]
    r += [("random", n) for n in COUNTS[1:]] + [("plateau", n) for n in COUNTS]
    r += [("arange", cols), ("plateau255", 300)]
    return r                                         # 15 rows


# ---- cases --------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name cols rows batch offset stride batch_stride k z_min min_distance inst recipes")
LAYOUTS = ("contig", "pitched", "offset1", "offset2", "offset3", "odd", "batch2_bytes", "batch3_vec", "stride16")


def _up(x, m):
    return (x + m - 1) // m * m


def _geometry(cols, rows, layout):
    """(offset, stride, batch, batch_stride) -- the image's place in its buffer of 255s."""
    if layout == "contig":
        return 0, cols, 1, rows * cols
    if layout == "pitched":                          # a cv::Mat ROI of a wider image
        s = _up(cols, 16) + 16
        return 0, s, 1, rows * s
    if layout.startswith("offset"):
        return int(layout[-1]), cols, 1, rows * cols
    if layout == "odd":
        s = (cols | 1) + 2
        return 0, s, 1, rows * s
    if layout == "batch2_bytes":                     # batch stride no multiple of 4: the second image is misaligned
        s = _up(cols, 4)
        return 0, s, 2, rows * s + 2
    if layout == "batch3_vec":
        s = _up(cols, 16)
        return 0, s, 3, rows * s + 16
    if layout == "stride16":
        return 0, 16, 1, rows * 16
    raise ValueError(layout)


def _image(name, b, cols, recipes, uz):
    rng = np.random.default_rng(zlib.crc32(("%s/%d" % (name, b)).encode()))
    return np.stack([make_row(kind, n, cols, uz, rng) for kind, n in recipes])


def _case(name, cols, layout, k, z_min, inst, recipes=None, min_distance=2.5):
    recipes = _recipes(cols) if recipes is None else recipes
    rows = len(recipes)
    assert 5 <= rows <= 15 and rows % 4, (name, rows)
    offset, stride, batch, bs = _geometry(cols, rows, layout)
    img0 = _image(name, 0, cols, recipes, u_zmin(z_min))
    labelled = tuple(Row(kind, n, named_path(img0[r], k, z_min)) for r, (kind, n) in enumerate(recipes))
    return Case(name, cols, rows, batch, offset, stride, bs, k, z_min, min_distance if cols > 64 else 0.0, inst, labelled)


def _build():
    cases = []
    # every instantiation at k = 12, 65, 300: (nchunk, vec, mask) -> width, layout
    inst_table = [
        ((1, 1, 1), 300, "pitched"), ((1, 1, 0), 1024, "contig"), ((1, 0, 1), 300, "offset1"), ((1, 0, 0), 300, "odd"),
        ((2, 1, 1), 1025, "pitched"), ((2, 1, 0), 2048, "batch3_vec"), ((2, 0, 1), 1025, "contig"), ((2, 0, 0), 2048, "offset2"),
        ((4, 1, 1), 3768, "contig"), ((4, 1, 0), 2049, "pitched"), ((4, 0, 1), 2049, "batch2_bytes"), ((4, 0, 0), 4096, "offset3"),
        ((8, 1, 1), 4097, "pitched"), ((8, 1, 0), 8192, "contig"), ((8, 0, 1), 8191, "contig"), ((8, 0, 0), 4097, "odd")]
    plain = 0
    for inst, cols, layout in inst_table:
        for j, k in enumerate(K_FEW):
            if inst[2]:
                z = Z_MASK[j]
            else:
                z = Z_PLAIN[plain % len(Z_PLAIN)]
                plain += 1
            cases.append(_case("n%d-%s-%s-%d-%s-k%d-z%g" % (inst[0], "vec" if inst[1] else "bytes", "mask" if inst[2] else "plain", cols, layout, k, z),
                               cols, layout, k, z, inst))
    # the whole k list on one NCHUNK 1 and one NCHUNK 4 layout (k = 12, 65, 300 of them are above)
    for k in K_ALL:
        cases.append(_case("klist-n1-1024-pitched-k%d-z60" % k, 1024, "pitched", k, 60, (1, 1, 0)))
        cases.append(_case("klist-n4-3768-batch3-k%d-z0" % k, 3768, "batch3_vec", k, 0, (4, 1, 1)))
    # the widths of the list not used above
    cases.append(_case("n8-8191-batch2-k40-z128", 8191, "batch2_bytes", 40, 128, (8, 0, 0)))
    cases.append(_case("n4-4096-contig-k64-z200", 4096, "contig", 64, 200, (4, 1, 0)))
    # masked, ragged and at most 256 bins (200 % 16 == 8): the histogram paths WITHOUT bracketing under the validity masks,
    # which no width of the list can reach (z_min = 0 makes every bin a candidate)
    for layout, vec in (("pitched", 1), ("offset3", 0)):
        for k in (12, 65):
            cases.append(_case("n1-200-%s-k%d-z0" % (layout, k), 200, layout, k, 0, (1, vec, 1),
                               recipes=[("random", 200), ("empty", 0), ("plateau", 200), ("arange", 200), ("plateau255", 200), ("random", 200),
                                        ("random", 200)]))
    # narrower than one 16-byte piece, and 17: rows gathered byte by byte, peak bitmaps of the first / last 16 bins overlap
    for i, cols in enumerate(NARROW):
        for layout in ("contig", "stride16") if cols <= 16 else ("contig", "pitched"):
            z = (0, 60, 200)[i % 3]
            vec = int(_geometry(cols, 7, layout)[1] % 4 == 0)
            cases.append(_case("narrow-%d-%s-k12-z%d" % (cols, layout, z), cols, layout, 12, z, (1, vec, int(z == 0))))
    # the witness of the bracketing defect: 256 < count < k at a trial (k > 256)
    cases.append(_case(WITNESS, 1024, "contig", 300, 0, (1, 1, 1), recipes=[("arange", 1024)] * 5))
    by_name = {c.name: c for c in cases}
    assert len(by_name) == len(cases)
    return by_name


WITNESS = "witness-arange1024-k300-z0"
CASES = _build()
ZMIN_CONVERSION_CASES = [(cols, z) for cols in (300, 2049) for z in (256, 0.9, 300, -1)]


def images(case):
    """uint8 [batch, rows, cols], the same every time: row r of every image follows recipe r, seeded by the case and the image."""
    return np.stack([_image(case.name, b, case.cols, [(r.kind, r.n) for r in case.recipes], u_zmin(case.z_min)) for b in range(case.batch)])


def buffer(case, img=None):
    """(bytes, view): the images laid out with the case's offset, row pitch and batch stride in a buffer of 255s -- a kernel
    that reads padding as row data sees returns that are not there -- and the [batch, rows, cols] view of them in it."""
    img = images(case) if img is None else img
    buf = np.full(case.offset + case.batch * case.batch_stride + 64, 255, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[case.offset:], (case.batch, case.rows, case.cols), (case.batch_stride, case.stride, 1))
    view[...] = img
    return buf, view


def plan(case, base=None):
    from tbv_slam_public_amd import api
    return api.kstrong_plan(case.rows, case.cols, case.k, case.z_min, RANGE_RES, case.min_distance, stride=case.stride, batch=case.batch,
                            batch_stride=case.batch_stride, base=case.offset if base is None else base)


def oracle(view2d, k, z_min, min_distance, stride):
    """Everything the filter call returns, from the oracle on the strided view of one image (its padding included)."""
    from oracle import pyoracle as O
    sr, si, sc = O.kstrongest(view2d, k, z_min, stride=stride)
    pk = O.peaks(view2d, k, sr, sc, stride=stride)
    return dict(sel_range=sr, sel_intensity=si, sel_count=sc, is_peak=pk,
                xyzi=O.kstrongest_cloud(sr, si, sc, RANGE_RES, min_distance), xyzi_peaks=O.kstrongest_cloud(sr, si, sc, RANGE_RES, min_distance, mask=pk))
