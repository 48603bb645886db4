"""NumPy restatement of cfear_cen2019_order_audit: which landmarks of a Cen2019 sweep hang on the order among equal h in
cen2019features' unstable std::sort.  It is the DEFINITION the kernels are compared against; it
imports tests/cen2019_cpu.py and changes nothing in it.

The order-free form of cen2019_cpu uses keys through comparisons only, so it holds for every total order that refines
"descending h" (-0 == +0).  With T = rows - 1, a `run` a maximal stretch of bins with s < 0, and the TOUCHERS of a run [u, v]
its own candidates, the candidate at v + 1 and the one at u - 1 if u - 1 < T:
  sure(c)       in every run c touches, h(c) is the largest h among the touchers and no other toucher attains it
  possible(c)   in every run c touches, h(c) is the largest h among the touchers
  sure <= fresh(order) <= possible for every order, so the order's cut K has h_lo <= h(K) <= h_hi, h_hi the h of the
  max_points-th largest possible candidate and h_lo that of the max_points-th largest sure one (-inf: fewer exist).
  P_in = {h > h_hi} is processed under every order, P_out = {h >= h_lo} holds every order's processed set; the band is
  P_out - P_in, and a band of one candidate is K itself: it joins P_in.
  R_in / R_out: order_free()'s marking rule on P_in / P_out, "the run's best own candidate is processed and sits at r < T"
  replaced by "an own candidate is processed, a top-h own candidate sits at r < T [R_in: and none at r >= T]".
  A target of R_in is CERTAIN if its run (clipped at min_range_bins) is the same maximal run in R_out.
The witness is the sweep filtered with ties by DESCENDING flat index: one legal order's outcome.

ordered() is a vectorised order_free() for either tie direction; test_cen2019_audit_cpu.py proves it equal to
cen2019_cpu.order_free() and to cen2019_cpu.literal() with the ties reversed."""
import numpy as np

from tests import cen2019_cpu as R

F = np.float32
RECORD_DTYPE = np.dtype([(n, np.int32) for n in (
    "n_candidates", "n_fresh", "n_sure_fresh", "n_possibly_fresh", "n_band", "n_rows_straddle_tied", "n_marks_in", "n_marks",
    "n_marks_out", "n_targets", "n_targets_certain", "n_targets_reversed", "n_targets_changed_reversed",
    "n_marks_changed_reversed")] + [("h_hi", F), ("h_lo", F)])
assert RECORD_DTYPE.itemsize == 64
BIG = np.iinfo(np.int64).max
RANDOM_WITHOUT_MARGIN = (15, 33, 83, 181)        # of cen2019_cpu.random_case(0 .. 199): mean_h_margin() does not hold


def straddle_tied_case():
    """cen2019_cpu.straddle_case() with row 2 changed so that the largest own h of its one run (the whole row, T = 5) is
    attained on both sides of T: bins 2, 4 and 9 hold the same byte between the same pair of neighbour bytes (104 and a dark
    bin), so they share g and h.  Ties ascending: bin 2 < T comes first and marks the whole row; descending: bin 9 >= T comes
    first and marks bins 0 .. 9, after which every other candidate finds its bin marked."""
    img = R.straddle_case().copy()
    img[2, :10] = (104, 104, 106, 0, 106, 104, 104, 104, 104, 106)
    return img


def device_random_cases():
    """the k of random_case(k), k < 200, that the device is compared on: those whose mean_h no fp64 summation order changes"""
    return [k for k in range(200) if k not in RANDOM_WITHOUT_MARGIN]


class ReversedTies:
    """literal(tie_rng=ReversedTies()): ties by descending flat index"""

    @staticmethod
    def permutation(n):
        return np.arange(n)[::-1]


def _runs(mask):
    """the maximal runs of every row of a mask, in (row, bin) order: row, first bin, last bin [n] and the run of every pixel
    [rows, cols] (-1 outside)"""
    rows, cols = mask.shape
    m = np.zeros((rows, cols + 2), np.int8)
    m[:, 1:-1] = mask
    d = np.diff(m, axis=1)
    row, u = np.nonzero(d == 1)
    v = np.nonzero(d == -1)[1] - 1
    rid = np.cumsum((d[:, :cols] == 1).ravel()).reshape(rows, cols) - 1
    rid[~mask] = -1
    return row, u, v, rid


def _at(per_run, idx):
    """per_run[idx] where idx may be -1 (no run: the value is 0 and the caller masks it), also when there is no run at all"""
    return np.append(per_run, per_run.dtype.type(0))[idx]


def prepare(img):
    """what the audit needs of a sweep whatever max_points is"""
    im = R.images(img)
    rows, cols = img.shape
    T = rows - 1
    h = im["h"] + F(0)                                                      # -0 and +0 are one value
    with np.errstate(invalid="ignore"):
        cand = h > im["mean_h"]
    neg = im["s"] < 0
    row, u, v, rid = _runs(neg)
    n = row.size
    col = np.broadcast_to(np.arange(cols), (rows, cols))
    right = (v + 1 < cols) & cand[row, np.minimum(v + 1, cols - 1)]         # the toucher right of the run, left of it
    left = (u >= 1) & (u - 1 < T) & cand[row, np.maximum(u - 1, 0)]
    h_right = np.where(right, h[row, np.minimum(v + 1, cols - 1)], -np.inf).astype(F)
    h_left = np.where(left, h[row, np.maximum(u - 1, 0)], -np.inf).astype(F)
    own = cand & neg
    own_top = np.full(n, -np.inf, F)
    np.maximum.at(own_top, rid[own], h[own])
    htop = np.maximum(own_top, np.maximum(h_right, h_left))
    at_own_top = own & (h == _at(own_top, rid))                                  # rid -1 where not own: masked by `own`
    ntop = np.bincount(rid[own & (h == _at(htop, rid))], minlength=n) + (right & (h_right == htop)) + (left & (h_left == htop))
    own_lo = np.bincount(rid[at_own_top & (col < T)], minlength=n) > 0      # a top-h own candidate at r < T, at r >= T
    own_hi = np.bincount(rid[at_own_top & (col >= T)], minlength=n) > 0
    # the runs a candidate touches: its own, or the one left of it and (r < T) the one right of it
    run_l = np.full((rows, cols), -1)
    run_l[:, 1:] = rid[:, :-1]
    run_r = np.full((rows, cols), -1)
    run_r[:, :-1] = rid[:, 1:]
    run_r[:, T:] = -1
    run_l[neg] = -1
    run_r[neg] = -1
    touched = (rid, run_l, run_r)
    possible, sure = cand.copy(), cand.copy()
    for t in touched:
        has = t >= 0
        top = has & (h == _at(htop, t))
        possible &= ~has | top
        sure &= ~has | (top & (_at(ntop, t) == 1))
    return dict(im=im, img=img, h=h, cand=cand, neg=neg, row=row, u=u, v=v, rid=rid, col=col, T=T, own=own, own_lo=own_lo,
                own_hi=own_hi, touched=touched, possible=possible, sure=sure, flat=bool(im["maxg"] == 0), ordered={})


def _level(h_of, max_points):
    """h of the max_points-th largest (inf: max_points == 0 -- nothing is processed; -inf: fewer exist -- everything is)"""
    if max_points <= 0:
        return F(np.inf)
    if h_of.size < max_points:
        return F(-np.inf)
    return F(np.partition(h_of, h_of.size - max_points)[h_of.size - max_points])


def _mark(pre, P, full_own):
    """order_free()'s marks of a processed set; full_own [runs]: the run's own rule marks it whole (if an own candidate is
    processed)"""
    row, u, v, rid, neg, T = pre["row"], pre["u"], pre["v"], pre["rid"], pre["neg"], pre["T"]
    rows, cols = neg.shape
    n = row.size
    nb = ((v + 1 < cols) & P[row, np.minimum(v + 1, cols - 1)]) | ((u >= 1) & (u - 1 < T) & P[row, np.maximum(u - 1, 0)])
    ownP = P & neg
    last = np.full(n, -1)
    np.maximum.at(last, rid[ownP], pre["col"][ownP])
    M = np.where(nb | ((last >= 0) & full_own), v, last)
    Rm = P & ~neg
    Rm[neg] = pre["col"][neg] <= M[rid[neg]]
    return Rm


def ordered(pre, max_points, reverse=False):
    """order_free() for ties by ascending (reverse: descending) flat index: R, P, fresh and counts (candidates, fresh,
    processed)"""
    h, cand, rid, row, u, v, T = pre["h"], pre["cand"], pre["rid"], pre["row"], pre["u"], pre["v"], pre["T"]
    rows, cols = cand.shape
    if reverse not in pre["ordered"]:
        flat = np.nonzero(cand.ravel())[0]
        order = flat[np.lexsort((-flat if reverse else flat, -h.ravel()[flat]))]
        rank = np.full(rows * cols, BIG, np.int64)
        rank[order] = np.arange(order.size)
        rank = rank.reshape(rows, cols)
        n = row.size
        own_best = np.full(n, BIG, np.int64)
        np.minimum.at(own_best, rid[pre["own"]], rank[pre["own"]])
        r_right = np.where(v + 1 < cols, rank[row, np.minimum(v + 1, cols - 1)], BIG)
        r_left = np.where((u >= 1) & (u - 1 < T), rank[row, np.maximum(u - 1, 0)], BIG)
        best = np.minimum(own_best, np.minimum(r_right, r_left))
        fresh = cand.copy()
        for t in pre["touched"]:
            has = t >= 0
            fresh &= ~has | (rank == _at(best, t))
        own_best_lo = np.zeros(n, bool)                                     # the run's best own candidate sits at r < T
        sel = pre["own"] & (rank == _at(own_best, rid))
        own_best_lo[rid[sel]] = pre["col"][sel] < T
        pre["ordered"][reverse] = (rank, fresh, np.sort(rank[fresh]), own_best_lo, order.size)
    rank, fresh, fresh_ranks, own_best_lo, n_cand = pre["ordered"][reverse]
    if max_points <= 0:
        cut = -1
    elif fresh_ranks.size >= max_points:
        cut = int(fresh_ranks[max_points - 1])
    else:
        cut = n_cand - 1
    P = rank <= cut
    return dict(R=_mark(pre, P, own_best_lo), P=P, fresh=fresh, counts=(n_cand, int(fresh.sum()), cut + 1))


def emit(pre, Rm, min_range_bins, R_out=None):
    """cen2019_cpu.emit() without loops: targets [n, 2] in (row, bin) order.  With R_out also certain [n]: the target's run is
    the same maximal run (clipped at min_range_bins) in R_out."""
    rows, cols = Rm.shape
    clip = Rm.copy()
    clip[:, :min(min_range_bins, cols)] = False
    row, u, v, rid = _runs(clip)
    below, above = np.roll(Rm, 1, axis=0), np.roll(Rm, -1, axis=0)
    c = np.zeros((rows, cols + 1), np.int64)
    np.cumsum(below | above, axis=1, out=c[:, 1:])
    keep = (v < cols - 1) & (c[row, np.minimum(v + 1, cols)] - c[row, u] > 0)   # an unmarked bin ends it; checkAdjacentMarked
    hpos = clip & (pre["h"] > 0)                                            # getMaxInRegion: the last bin with h > 0, else the first
    tgt = np.full(row.size, -1)
    np.maximum.at(tgt, rid[hpos], pre["col"][hpos])
    tgt = np.where(tgt >= 0, tgt, u)
    targets = np.stack([row[keep], tgt[keep]], axis=1).astype(np.int32).reshape(-1, 2)
    if R_out is None:
        return targets
    vn = np.minimum(v + 1, cols - 1)
    same = ~R_out[row, vn] & ((u == min_range_bins) | ~R_out[row, np.maximum(u - 1, 0)])
    return targets, same[keep]


def audit(img, max_points=1000, min_range_bins=0, pre=None):
    """-> dict(record RECORD_DTYPE scalar array [1], targets [n, 2] (this library's), certain uint8 [n], marks uint8
    [rows, cols]: bit 0 R_in, bit 1 R, bit 2 R_out, bit 3 R of the reversed order; R_in, R_out, R, R_rev, targets_rev)"""
    pre = pre or prepare(img)
    rows, cols = img.shape
    rec = np.zeros(1, RECORD_DTYPE)
    if pre["flat"]:
        rec["h_hi"] = rec["h_lo"] = np.nan
        z = np.zeros((rows, cols), bool)
        return dict(record=rec, targets=np.zeros((0, 2), np.int32), certain=np.zeros(0, np.uint8), marks=np.zeros((rows, cols), np.uint8),
                    R_in=z, R_out=z, R=z, R_rev=z, targets_rev=np.zeros((0, 2), np.int32))
    h, cand, T = pre["h"], pre["cand"], pre["T"]
    h_hi = _level(h[pre["possible"]], max_points)
    h_lo = _level(h[pre["sure"]], max_points)
    band = cand & (h >= h_lo) & (h <= h_hi)
    n_band = int(band.sum())
    P_in = cand & (h > h_hi)
    P_out = cand & (h >= h_lo)
    if n_band == 1:                                                         # that candidate is every order's K
        P_in, n_band = P_out.copy(), 0
    R_in = _mark(pre, P_in, pre["own_lo"] & ~pre["own_hi"])
    R_out = _mark(pre, P_out, pre["own_lo"])
    own_out = np.bincount(pre["rid"][P_out & pre["neg"]], minlength=pre["row"].size) > 0
    straddle = (pre["u"] < T) & (pre["v"] >= T) & own_out & pre["own_lo"] & pre["own_hi"]
    fwd, rev = ordered(pre, max_points), ordered(pre, max_points, True)
    targets = emit(pre, fwd["R"], min_range_bins)
    targets_rev = emit(pre, rev["R"], min_range_bins)
    t_in, same = emit(pre, R_in, min_range_bins, R_out)
    sure_t = {tuple(t) for t in t_in[same].tolist()}
    certain = np.array([tuple(t) in sure_t for t in targets.tolist()], np.uint8).reshape(-1)
    assert int(certain.sum()) == len(sure_t)                                # a certain target is one of this library's
    a, b = {tuple(t) for t in targets.tolist()}, {tuple(t) for t in targets_rev.tolist()}
    r = rec[0]
    r["n_candidates"], r["n_fresh"] = fwd["counts"][0], fwd["counts"][1]
    r["n_sure_fresh"], r["n_possibly_fresh"] = int(pre["sure"].sum()), int(pre["possible"].sum())
    r["n_band"], r["n_rows_straddle_tied"] = n_band, int(straddle.sum())
    r["n_marks_in"], r["n_marks"], r["n_marks_out"] = int(R_in.sum()), int(fwd["R"].sum()), int(R_out.sum())
    r["n_targets"], r["n_targets_certain"] = len(targets), int(certain.sum())
    r["n_targets_reversed"], r["n_targets_changed_reversed"] = len(targets_rev), len(a ^ b)
    r["n_marks_changed_reversed"] = int((fwd["R"] ^ rev["R"]).sum())
    r["h_hi"], r["h_lo"] = h_hi, h_lo
    marks = (R_in * 1 + fwd["R"] * 2 + R_out * 4 + rev["R"] * 8).astype(np.uint8)
    return dict(record=rec, targets=targets, certain=certain, marks=marks, R_in=R_in, R_out=R_out, R=fwd["R"], R_rev=rev["R"],
                targets_rev=targets_rev, fresh=fwd["fresh"])
