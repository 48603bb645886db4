"""GPU: kstrongest_rowpairs_kernel<NCHUNK, MASK> -- two azimuth rows per wavefront, selected in one ranking pass when they hold
at most 64 candidates together -- against the CPU oracle and against the single-row table (CFEAR_OPT_KSTRONG_ROW_PAIRS = 0),
bit for bit.  Every image is built by construction: zeros with chosen bytes set, so the candidate count of every row is known
and, from the counts and the rule alone (rows 2p and 2p + 1 of an image, both present, counts adding up to at most 64), which
pairs take the joint path and which fall back to kstrong_row on each staged row.  No tolerances: every output is an integer."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RANGE_RES = 0.0438
MIN_DISTANCE = 2.5                                   # ceil(2.5 / 0.0438) = 58: bins <= 58 are kept but not part of the cloud
COLS = (48, 1040, 2064, 3360, 3768)                  # NCHUNK 1, 2, 4, 4, 4 (3768: the row ends 8 bytes into a 16-byte piece)
NCHUNK = {24: 1, 48: 1, 1040: 2, 2064: 4, 3360: 4, 3768: 4}


def joint_pairs(counts):
    """Per pair (2p, 2p + 1) of one image: True = joint path, False = fallback (the rule of the kernel, from the counts alone)."""
    counts = list(counts)
    return [2 * p + 1 < len(counts) and counts[2 * p] + counts[2 * p + 1] <= 64 for p in range((len(counts) + 1) // 2)]


def put(img, r, positions, values):
    positions = np.asarray(positions, np.int64)
    assert len(np.unique(positions)) == len(positions) and (positions >= 0).all() and (positions < img.shape[1]).all()
    img[r, positions] = values


def scatter_row(img, r, n, lo, hi, seed):
    """n candidates at random bins of row r -- always the first and the last bin among them -- with intensities in [lo, hi]
    (a narrow interval: ties at every cut)."""
    cols = img.shape[1]
    n = min(n, cols)
    if n == 0:
        return 0
    rng = np.random.default_rng(seed)
    pos = rng.choice(cols, n, replace=False)
    if n >= 2:
        pos[:2] = (0, cols - 1)
        pos = np.unique(pos)
        while len(pos) < n:
            pos = np.unique(np.append(pos, rng.integers(0, cols)))
    put(img, r, pos, rng.integers(lo, hi + 1, len(pos)))
    return n


def counted(cols, counts, lo=60, hi=70, seed=0):
    img = np.zeros((len(counts), cols), np.uint8)
    got = [scatter_row(img, r, n, lo, hi, 1000 * seed + r) for r, n in enumerate(counts)]
    return img, got


@contextlib.contextmanager
def single_row_table():
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    assert ctx.get_option(L.OPT_KSTRONG_ROW_PAIRS) == 1                       # the default route is the pair kernel
    ctx.set_option(L.OPT_KSTRONG_ROW_PAIRS, 0)
    try:
        yield
    finally:
        ctx.set_option(L.OPT_KSTRONG_ROW_PAIRS, 1)


def _filter(dev, k, z_min, min_distance, want_peaks=False):
    import torch
    from tbv_slam_public_amd import api
    r = api.filter_kstrongest(dev, k, z_min, RANGE_RES, min_distance, want_peaks=want_peaks)
    torch.cuda.synchronize()
    api.default_context().synchronize()
    return {name: v.cpu().numpy() for name, v in r.items()}


def _rowkeys(dev, k, z_min, min_distance):
    from tbv_slam_public_amd import api
    keys, cnt = api.filter_kstrongest_rowkeys(dev, k, z_min, RANGE_RES, min_distance)
    return keys.cpu().numpy().view(np.uint32), cnt.cpu().numpy()


def check(imgs, k, z_min=60, min_distance=MIN_DISTANCE, what=""):
    """imgs [batch][rows][cols] (or one image): both entry points on the default route against the oracle and against the
    single-row table."""
    import torch
    from oracle import pyoracle as O
    from tests.test_gpu_filters import _rowkeys_expected
    imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
    dev = torch.from_numpy(imgs).cuda()
    got = _filter(dev, k, z_min, min_distance)
    with single_row_table():
        one = _filter(dev, k, z_min, min_distance)
    for b in range(imgs.shape[0]):
        sr, si, sc = O.kstrongest(imgs[b], k, z_min)
        for name, ref in (("sel_count", sc), ("sel_range", sr), ("sel_intensity", si)):    # whole arrays: unused slots are -1 / 0
            np.testing.assert_array_equal(got[name][b], ref, err_msg="%s image %d %s" % (what, b, name))
    for name in got:
        if name == "xyzi":                                                      # rows beyond n_points are not written
            for b in range(imgs.shape[0]):
                assert got["n_points"][b] == one["n_points"][b]
                np.testing.assert_array_equal(got[name][b, :got["n_points"][b]], one[name][b, :one["n_points"][b]], err_msg="%s %s" % (what, name))
        else:
            np.testing.assert_array_equal(got[name], one[name], err_msg="%s %s against the single-row table" % (what, name))
    if k <= 64:
        keys, cnt = _rowkeys(dev, k, z_min, min_distance)
        with single_row_table():
            keys1, cnt1 = _rowkeys(dev, k, z_min, min_distance)
        np.testing.assert_array_equal(cnt, cnt1, err_msg=what)
        for b in range(imgs.shape[0]):
            exp = _rowkeys_expected(imgs[b], k, z_min, RANGE_RES, min_distance)
            np.testing.assert_array_equal(cnt[b, :, 0], [len(e) for e in exp], err_msg="%s image %d" % (what, b))
            assert (cnt[b, :, 1] == 0).all()
            for r, e in enumerate(exp):
                np.testing.assert_array_equal(keys[b, r, :len(e)], e, err_msg="%s image %d row %d" % (what, b, r))
                np.testing.assert_array_equal(keys1[b, r, :len(e)], e, err_msg="%s image %d row %d (single-row table)" % (what, b, r))


# ---- shapes --------------------------------------------------------------------------------------------------------------------
SHAPE_COUNTS = (20, 30, 50, 30, 40)                  # pairs: 50 joint, 80 falls back, the fifth row alone


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", (1, 2, 3, 5))
def test_shapes(rows, cols):
    """rows 1, 2, 3, 5 (an absent second row, whole pairs, both) at every width class; a batch of three different images."""
    imgs, kinds = [], []
    for b in range(3):
        want = [SHAPE_COUNTS[(r + b) % 5] for r in range(rows)]
        img, counts = counted(cols, want, seed=10 * rows + b)
        assert counts == [min(n, cols) for n in want]
        imgs.append(img)
        kinds += joint_pairs(counts)
    if rows >= 2 and cols > 48:
        assert True in kinds
    if rows >= 3 and cols > 48:
        assert False in kinds
    check(np.stack(imgs), 40, what="rows %d cols %d" % (rows, cols))


# ---- pair sums -----------------------------------------------------------------------------------------------------------------
PAIR_SUMS = ((0, 0), (64, 0), (0, 64), (32, 32), (33, 32), (70, 0), (300, 5))


def test_the_case_lists_hold_both_kinds_for_every_nchunk():
    for cols in COLS:
        counts = [min(n, cols) for pair in PAIR_SUMS for n in pair]
        kinds = joint_pairs(counts)
        assert True in kinds and False in kinds, (cols, NCHUNK[cols], kinds)
    assert joint_pairs([min(n, 3360) for pair in PAIR_SUMS for n in pair]) == [True, True, True, True, False, False, False]
    assert joint_pairs([41, 41]) == [False] and joint_pairs([64]) == [False] and joint_pairs([1, 2, 3]) == [True, False]


@pytest.mark.parametrize("cols", COLS)
def test_pair_sums(cols):
    """0 + 0, 64 + 0, 0 + 64, 32 + 32 joint; 33 + 32 = 65, a dense row beside an empty one and a histogram row in the pair fall
    back (at 48 bins a row holds at most 48 candidates: 32 + 32 is the joint pair, 33 + 32 and 48 + 5 the fallbacks)."""
    img, counts = counted(cols, [n for pair in PAIR_SUMS for n in pair], seed=cols)
    kinds = joint_pairs(counts)
    assert True in kinds and False in kinds
    if cols > 300:
        assert counts == [n for pair in PAIR_SUMS for n in pair]
    for k in (40, 12):
        check(img, k, what="pair sums cols %d k %d" % (cols, k))


# ---- the cut, k = 40 -----------------------------------------------------------------------------------------------------------
def cut_image(cols):
    """Ten pairs; returns (image, counts)."""
    rows = []

    def row(positions, values):
        r = np.zeros(cols, np.uint8)
        positions = np.asarray(positions, np.int64)
        assert len(np.unique(positions)) == len(positions) and (positions >= 0).all() and (positions < cols).all()
        r[positions] = values
        rows.append(r)

    rng = np.random.default_rng(cols)
    spread = lambda n: np.sort(rng.choice(cols, n, replace=False))
    # 0: one row with a drop (41 .. 64 candidates) beside one without
    row(spread(41), rng.integers(60, 256, 41)); row(spread(23), rng.integers(60, 256, 23))
    row(spread(10), rng.integers(60, 256, 10)); row(spread(54), rng.integers(60, 64, 54))
    row(spread(64), rng.integers(60, 62, 64)); row([], [])
    # 3: both with a drop -- 82 candidates, so the pair falls back
    row(spread(41), rng.integers(60, 256, 41)); row(spread(41), rng.integers(60, 256, 41))
    # 4: equal intensities at the cut (all of them): the range decides
    row(spread(50), 100); row(spread(14), 100)
    # 5: all 64 candidates in the 16 bytes of ONE lane and its neighbours (one run of 64 adjacent bins), beside an empty row and
    # 6: beside a row whose candidates sit in the same bins
    run = 16 * min(5, cols // 16 - 4) + np.arange(64) if cols >= 64 else np.arange(cols)
    row(run, rng.integers(60, 70, len(run))); row([], [])
    row(run[:40], rng.integers(60, 70, 40)); row(run[:24], rng.integers(60, 70, 24))
    # 7: candidates in the last chunk's last live lane (the last bins of the row), both rows
    row(cols - 1 - np.arange(30), rng.integers(60, 70, 30)); row(cols - 1 - np.arange(34), rng.integers(60, 70, 34))
    # 8: the last bins of row 0 and the first bins of row 1 (adjacent bytes of the image)
    row(cols - 1 - np.arange(20), rng.integers(60, 70, 20)); row(np.arange(44), rng.integers(60, 70, 44))
    # 9: a drop with every candidate of the dropped kind below bin 58 (min_distance removes kept bins of one row only)
    row(np.arange(45), rng.integers(60, 70, 45)); row(100 + np.arange(19), rng.integers(60, 70, 19))
    img = np.stack(rows)
    return img, [int((r >= 60).sum()) for r in img]


@pytest.mark.parametrize("cols", (1040, 2064, 3360, 3768))
def test_the_cut(cols):
    img, counts = cut_image(cols)
    assert joint_pairs(counts) == [True, True, True, False, True, True, True, True, True, True]
    assert counts[0] == 41 and counts[3] == 54 and counts[4] == 64                  # drop > 0 beside a row with <= 40
    check(img, 40, what="cut cols %d" % cols)


# ---- parameters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (12, 40, 64, 100))
def test_k(k):
    """k = 12: both rows of a joint pair are cut; k = 64 and 100: nothing of a joint pair is (k = 100: more than 64 slots per
    row, no row keys; joint only while the sum is <= 64)."""
    for cols in (1040, 3360):
        img, counts = counted(cols, [20, 30, 13, 51, 60, 41, 100, 0, 150, 20, 64], seed=k)
        assert joint_pairs(counts) == [True, True, False, False, False, False]
        check(img, k, what="k %d cols %d" % (k, cols))


@pytest.mark.parametrize("cols", (1040, 3360))
def test_min_distance(cols):
    """min_distance removes some of the kept bins, and all kept bins of one row (the other row of the pair keeps its own)."""
    img = np.zeros((4, cols), np.uint8)
    rng = np.random.default_rng(cols)
    put(img, 0, np.arange(0, 60, 2), rng.integers(60, 70, 30))                      # bins 0 .. 58: all removed at min bin 58
    put(img, 1, 40 + np.arange(30), rng.integers(60, 70, 30))                       # bins 40 .. 69: some removed
    put(img, 2, 500 + np.arange(50), rng.integers(60, 70, 50))                      # cut at k = 40, none removed
    put(img, 3, np.arange(10), rng.integers(60, 70, 10))                            # all removed
    assert joint_pairs([30, 30, 50, 10]) == [True, True]
    check(img, 40, what="min_distance cols %d" % cols)
    check(img, 40, min_distance=0.0, what="min_distance 0 cols %d" % cols)          # bin 0 alone is removed (range > 0)
    check(img, 40, min_distance=RANGE_RES * (cols + 5), what="min_distance beyond the row, cols %d" % cols)


@pytest.mark.parametrize("cols", COLS)
def test_z_min_200(cols):
    """z_min >= 128: the THI form of the byte compare; bytes below 200 are set too and are no candidates."""
    img, counts = counted(cols, [25, 39, 40, 30, 12], lo=200, hi=203, seed=cols)
    noise, _ = counted(cols, [40, 40, 40, 40, 40], lo=1, hi=199, seed=cols + 1)
    img = np.where(img > 0, img, noise)
    assert [int((r >= 200).sum()) for r in img] == counts
    assert joint_pairs(counts) == [True, False, False]
    check(img, 40, z_min=200, what="z_min 200 cols %d" % cols)
    check(img, 12, z_min=200, what="z_min 200 k 12 cols %d" % cols)


@pytest.mark.parametrize("cols", (24, 48, 1040, 2064, 3768))
def test_z_min_0(cols):
    """z_min = 0: the MASK instantiations -- every bin is a candidate, so a pair is joint only up to 32 bins per row."""
    rng = np.random.default_rng(cols)
    img = rng.integers(0, 256, (5, cols)).astype(np.uint8)
    assert joint_pairs([cols] * 5) == [cols <= 32, cols <= 32, False]
    for k in (12, 40):
        check(img, k, z_min=0, what="z_min 0 cols %d k %d" % (cols, k))


# ---- routes the pair kernel does not take ---------------------------------------------------------------------------------------
def test_peaks_take_the_single_row_route():
    """want_peaks: the peaks' halo bytes are not kept by the pair kernel, so the launch takes the table of 16 with the option at 1 --
    the results, peaks included, are the oracle's and those under option 0."""
    import torch
    from tbv_slam_public_amd import api, _lib as L
    from tests import kstrong_cases as K
    img, counts = counted(2064, [20, 30, 50, 30, 40], seed=5)
    dev = torch.from_numpy(img).cuda()
    assert api.default_context().get_option(L.OPT_KSTRONG_ROW_PAIRS) == 1
    got = _filter(dev, 40, 60, MIN_DISTANCE, want_peaks=True)
    with single_row_table():
        one = _filter(dev, 40, 60, MIN_DISTANCE, want_peaks=True)
    ref = K.oracle(img, 40, 60, MIN_DISTANCE, 2064)
    for name in ("sel_count", "sel_range", "sel_intensity", "is_peak"):
        np.testing.assert_array_equal(got[name][0], ref[name], err_msg=name)
        np.testing.assert_array_equal(got[name], one[name], err_msg=name)
    for cloud, count in (("xyzi", "n_points"), ("xyzi_peaks", "n_peaks")):
        n = ref[cloud].shape[0]
        assert got[count][0] == n == one[count][0]
        np.testing.assert_array_equal(got[cloud][0, :n], ref[cloud])
        np.testing.assert_array_equal(one[cloud][0, :n], ref[cloud])


def test_the_option_accepts_0_and_1_only():
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    assert ctx.get_option(L.OPT_KSTRONG_ROW_PAIRS) == 1
    with pytest.raises(L.CfearError):
        ctx.set_option(L.OPT_KSTRONG_ROW_PAIRS, 2)
    assert ctx.get_option(L.OPT_KSTRONG_ROW_PAIRS) == 1


def test_image_offsets_out_of_order():
    """The fuser's prefetched sweep: three streams whose images sit in one device buffer in shuffled order, with gaps
    (cfear_odometry_process_offsets) -- every field of the frame record equals the single-row table's."""
    import torch
    from tbv_slam_public_amd import api, synth
    F, B = 2, 3
    seqs = np.stack([synth.scene_v1(40 + b, F)[0] for b in range(B)])          # [B][F][400][3360]
    size = 400 * 3360
    slot = size + 4096
    order = np.random.default_rng(1).permutation(B * F)
    ring = torch.zeros(B * F * slot, dtype=torch.uint8, device="cuda")
    off = np.zeros((B, F), np.int64)
    for b in range(B):
        for f in range(F):
            off[b, f] = int(order[b * F + f]) * slot
            ring[off[b, f]:off[b, f] + size] = torch.from_numpy(seqs[b, f].reshape(-1)).cuda()
    assert not (np.diff(off[:, 0]) > 0).all()                                  # the images are out of order

    def run():
        od = api.OdometryKeyframeFuser(B, 400, 3360)
        return [od.process_offsets(ring, off[:, f], off[:, f + 1] if f + 1 < F else None).copy() for f in range(F)]

    got = run()
    with single_row_table():
        one = run()
    for f in range(F):
        assert (got[f]["n_points"] > 1000).all()
        for name in got[f].dtype.names:
            np.testing.assert_array_equal(got[f][name], one[f][name], err_msg="%s frame %d" % (name, f))
