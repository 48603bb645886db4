"""GPU: cfear_kstrong_rowkeys_derive -- the row keys of several k-strongest parameter sets from the sel_* lists of ONE sweep --
against cfear_filter_kstrongest_rowkeys run directly with each class's parameters, bit for bit: the counts and the first
`count` keys of every (class, row).  Uniform random, five-valued and constant rows; 96 bins (one chunk) and 1030 bins (two
chunks, a ragged tail); k_sup 1, 3 and 64; thresholds at, just above and far above intensities that occur; near cuts of 0,
the preset's and one beyond every bin.  No tolerances: every output is an integer."""
import functools
import itertools

import numpy as np
import pytest

from tests import grid_cpu as G

pytestmark = pytest.mark.gpu

RANGE_RES = 0.0438
SHAPES = ((5, 96), (4, 1030))
Z_CLASS = (0, 60, 61, 62, 250)                # at (60, 61 occur in the five-valued rows), just above (62), far above (250)
K_CLASS = (1, 12)                             # and k_sup itself


def _images(rows, cols):
    """3 images: uniform random | five-valued {0, 59, 60, 61, 255} | constant rows (0, 60, 255, 61, 59: the 0 row is empty
    at every threshold > 0, the 59 row at 60)."""
    const = np.repeat(np.array([0, 60, 255, 61, 59], np.uint8)[:rows, None], cols, axis=1)
    return np.stack([G.rows_of("uniform", rows, cols, 11 + cols), G.rows_of("five", rows, cols, 12 + cols), const])


def _min_distances(cols):
    return (0.0, 2.5, cols * RANGE_RES + 1.0)


@functools.lru_cache(maxsize=None)
def _device_images(shape):
    import torch
    return torch.from_numpy(_images(*shape)).cuda()


@functools.lru_cache(maxsize=None)
def _direct(shape, k, z_min, min_distance):
    """cfear_filter_kstrongest_rowkeys on the three images with one class's parameters (computed once, shared, read only)."""
    from tbv_slam_public_amd import api
    keys, cnt = api.filter_kstrongest_rowkeys(_device_images(shape), k, z_min, RANGE_RES, min_distance)
    api.default_context().synchronize()
    keys, cnt = keys.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    keys.setflags(write=False); cnt.setflags(write=False)
    return keys, cnt


def _tie_at_cut(row, k, z_min):
    """The k-th and the (k + 1)-th strongest candidate of the row have the same intensity: the cut runs through a tie."""
    cand = np.sort(row[row >= G.u8(z_min)])[::-1]
    return len(cand) > k and cand[k - 1] == cand[k]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("z_sup", [0, 60])
@pytest.mark.parametrize("k_sup", [1, 3, 64])
def test_derived_keys_equal_the_direct_sweep(k_sup, z_sup, shape):
    from tbv_slam_public_amd import api
    rows, cols = shape
    imgs = _images(rows, cols)
    sup = api.filter_kstrongest(_device_images(shape), k_sup, z_sup, RANGE_RES, 2.5)
    classes = [(image, k, z, RANGE_RES, md)
               for image, k, z, md in itertools.product(range(3), sorted({k for k in K_CLASS if k <= k_sup} | {k_sup}),
                                                        [z for z in Z_CLASS if z >= z_sup], _min_distances(cols))]
    keys, cnt = api.kstrong_rowkeys_derive(sup["sel_range"], sup["sel_intensity"], sup["sel_count"], classes, z_sup)
    api.default_context().synchronize()
    keys, cnt = keys.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    sup_count = sup["sel_count"].cpu().numpy()
    fewer = empty = ties = 0
    for c, (image, k, z, _, md) in enumerate(classes):
        dkeys, dcnt = _direct(shape, k, z, md)
        assert np.array_equal(cnt[c], dcnt[image]), (c, classes[c])           # {count, 0} of every row
        for r in range(rows):
            n = dcnt[image, r, 0]
            assert n <= k and np.array_equal(keys[c, r, :n], dkeys[image, r, :n]), (c, classes[c], r)
            fewer += n < sup_count[image, r]
            empty += n == 0
            ties += bool(_tie_at_cut(imgs[image, r], k, z))
    # against a vacuous pass, on the direct outputs: the classes do cut the superset down, to nothing in places, through ties
    assert 4 * fewer >= len(classes) * rows, (fewer, len(classes) * rows)
    assert empty >= 1 and ties >= 1


def test_numpy_rule_agrees_with_the_kernel():
    """The restatement the CPU tests pin to the oracle (tests/grid_cpu.py) is the rule the kernel applies."""
    from tbv_slam_public_amd import api
    shape = SHAPES[0]
    sup = api.filter_kstrongest(_device_images(shape), 64, 0, RANGE_RES, 2.5)
    classes = [(1, 12, 60, RANGE_RES, 2.5), (0, 64, 0, RANGE_RES, 0.0), (2, 3, 61, RANGE_RES, 0.5)]
    keys, cnt = api.kstrong_rowkeys_derive(sup["sel_range"], sup["sel_intensity"], sup["sel_count"], classes, 0)
    keys, cnt = keys.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    h = {n: v.cpu().numpy() for n, v in sup.items()}
    for c, (image, k, z, rr, md) in enumerate(classes):
        wk, wc = G.derive_rowkeys(h["sel_range"][image], h["sel_intensity"][image], h["sel_count"][image], k, z, rr, md)
        assert np.array_equal(cnt[c, :, 0], wc) and not cnt[c, :, 1].any()
        assert np.array_equal(keys[c], wk)                                    # (the outputs start zeroed: unwritten = 0)


def test_refusals():
    import ctypes as C
    import torch
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    shape = SHAPES[0]
    sup = api.filter_kstrongest(_device_images(shape), 3, 60, RANGE_RES, 2.5)
    args = (sup["sel_range"], sup["sel_intensity"], sup["sel_count"])
    good = (0, 3, 60, RANGE_RES, 2.5)
    api.kstrong_rowkeys_derive(*args, [good], 60)
    for bad in ((0, 4, 60, RANGE_RES, 2.5),          # k beyond k_sup
                (0, 0, 60, RANGE_RES, 2.5),          # k < 1
                (0, 3, 59, RANGE_RES, 2.5),          # threshold below the sweep's
                (0, 3, 256, RANGE_RES, 2.5),         # ... 256 wraps to 0
                (3, 3, 60, RANGE_RES, 2.5), (-1, 3, 60, RANGE_RES, 2.5),   # image outside [0, 3)
                (0, 3, 60, 0.0, 2.5)):               # range_res <= 0
        with pytest.raises(L.CfearError, match="class 1") as e:
            api.kstrong_rowkeys_derive(*args, [good, bad], 60)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
    # k_sup outside [1, 64]
    wide = torch.zeros((1, 5, 65), dtype=torch.int32, device="cuda")
    with pytest.raises(L.CfearError, match="k_sup"):
        api.kstrong_rowkeys_derive(wide, wide.to(torch.uint8), torch.zeros((1, 5), dtype=torch.int32, device="cuda"), [(0, 3, 60, RANGE_RES, 2.5)], 60)
    # null pointers, and host pointers where device memory is required
    lib = ctx._lib
    cls = (L.RowkeysClass * 1)(L.RowkeysClass(*[0, 3, 60.0, RANGE_RES, 2.5]))
    keys = torch.zeros((1, 5, 64), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1, 5, 2), dtype=torch.int32, device="cuda")
    dev = [a.data_ptr() for a in args] + [keys.data_ptr(), cnt.data_ptr()]
    host = [np.zeros(4096, np.uint8) for _ in dev]

    def call(ptrs, classes=cls, n_images=3, rows=5, n_classes=1):
        return lib.cfear_kstrong_rowkeys_derive(ctx.h, ptrs[0], ptrs[1], ptrs[2], n_images, rows, 3, 60.0, classes, n_classes, ptrs[3], ptrs[4])

    assert call(dev) == L.OK
    for i in range(5):
        assert call(dev[:i] + [None] + dev[i + 1:]) == L.ERR_INVALID_ARGUMENT
        assert call(dev[:i] + [host[i].ctypes.data] + dev[i + 1:]) == L.ERR_INVALID_ARGUMENT
    assert call(dev, classes=None) == L.ERR_INVALID_ARGUMENT
    assert call(dev, classes=C.cast(keys.data_ptr(), C.POINTER(L.RowkeysClass))) == L.ERR_INVALID_ARGUMENT
    assert call(dev, n_images=0) == call(dev, rows=0) == call(dev, n_classes=0) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_kstrong_rowkeys_derive(None, dev[0], dev[1], dev[2], 3, 5, 3, 60.0, cls, 1, dev[3], dev[4]) == L.ERR_INVALID_ARGUMENT
    ctx.synchronize()
