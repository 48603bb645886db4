"""GPU: cfear_filter_cen2018 on every route it has, against the NumPy float32 restatement (tests/cen2018_cpu.py) with the
comparison of tests/test_gpu_cen2018.py: the three row kernels (cen2018_rows_kernel<15>, <51>, <0>) at one, two, three, eight
and sixteen 512-bin passes and at 64 and 65 .. 128 bitmap words; runs of hundreds of bins, from bin 0, into the last bin and
over the whole row; odd row counts, 1 row, and rows beyond the cloud kernel's 256-row scan block; zq <= 0; the widest and the
narrowest filter; min_range_bins at the row's end; absent optional outputs; more than one chunk; more images than a grid
has rows; the refusals.  tests/test_cen2018_cpu.py proves, without a GPU, that every input holds what it is there for."""
import numpy as np
import pytest

from tests import cen2018_cpu as R
from tests.cen2018_gpu import compare, run

pytestmark = pytest.mark.gpu
NAMES = sorted(R.matrix_cases().keys())
# one case per row kernel, one above 4096 bins, the whole-row run
SUBSET = ["s5w1025", "s17w1025", "s9w1025", "s17w8192", "zq-1w8192m0"]
PER_KERNEL = ["s5w1025", "s17w1025", "s9w1025"]


def _ref(name):
    if not hasattr(_ref, "c"):
        _ref.c = {}
    if name not in _ref.c:
        imgs, par, _ = R.matrix_cases()[name]
        _ref.c[name] = [R.cen2018(img, **par) for img in imgs]
    return _ref.c[name]


def _cap(name):
    return max(len(r["targets"]) for r in _ref(name)) + 64


def _same_bits(h, d, batch):
    for k in ("n_points", "row_stats", "det_mask"):
        assert np.array_equal(h[k], d[k]), k
    for b in range(batch):
        n = int(h["n_points"][b])
        assert np.array_equal(h["targets"][b, :n], d["targets"][b, :n]), b
        assert np.array_equal(h["xyzi"][b, :n].view(np.uint32), d["xyzi"][b, :n].view(np.uint32)), b


@pytest.mark.parametrize("name", NAMES)
def test_matrix_case_equals_restatement(name):
    imgs, par, _ = R.matrix_cases()[name]
    compare(run(imgs, par, _cap(name)), _ref(name), imgs, name)


@pytest.mark.parametrize("name", SUBSET)
def test_matrix_device_pointers_equal_host_pointers(name):
    imgs, par, _ = R.matrix_cases()[name]
    h = run(imgs, par, _cap(name))
    d = run(imgs, par, _cap(name), device=True)
    compare(d, _ref(name), imgs, name)
    _same_bits(h, d, len(imgs))


@pytest.mark.parametrize("name", PER_KERNEL)
def test_absent_optional_outputs_leave_the_cloud_as_it_is(name):
    """targets, det_mask and row_stats all absent: n_points and xyzi are the bits of the call that asked for them"""
    import torch
    from tbv_slam_public_amd import api
    imgs, par, _ = R.matrix_cases()[name]
    full = run(imgs, par, _cap(name))
    compare(full, _ref(name), imgs, name)
    bare_h = api.filter_cen2018(imgs, cap_points=_cap(name), **par)
    bare_d = api.filter_cen2018(torch.from_numpy(imgs).cuda(), cap_points=_cap(name), **par)
    torch.cuda.synchronize()
    for bare in (bare_h, {k: v.cpu().numpy() for k, v in bare_d.items()}):
        assert sorted(bare.keys()) == ["n_points", "xyzi"]
        assert np.array_equal(bare["n_points"], full["n_points"])
        for b in range(len(imgs)):
            n = int(full["n_points"][b])
            assert n > 0 and np.array_equal(bare["xyzi"][b, :n].view(np.uint32), full["xyzi"][b, :n].view(np.uint32))


@pytest.mark.parametrize("offset", [0, 5])
@pytest.mark.parametrize("sigma_gauss", [5, 17])
def test_chunks_of_five_five_and_one(sigma_gauss, offset):
    """A chunk is 64 MiB of image bytes as the descriptor counts them, rows * stride.  With a row pitch of 4 MiB an image of
    3 x 100 bins counts 12 MiB, so 11 images go in chunks of 5, 5 and 1: the per-chunk offsets of every output, and the
    scratch bitmaps used three times.  The padding is 255 everywhere; the batch stride adds 13 bytes, so the images start at
    every byte alignment (offset 0: image 0, 4 and 8 take the dword loads; offset 5: a view that is itself unaligned)."""
    import torch
    imgs, par = R.chunk_case(sigma_gauss)
    refs = [R.cen2018(img, **par) for img in imgs]
    batch, rows, cols = imgs.shape
    pitch = 4 << 20
    bstride = rows * pitch + 13
    assert (64 << 20) // (rows * pitch) == 5 and batch == 11
    t = torch.full((batch * bstride + offset,), 255, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(t, (batch, rows, cols), (bstride, pitch, 1), offset)
    view.copy_(torch.from_numpy(imgs).cuda())
    got = run(view, par, 64, device=True)
    compare(got, refs, imgs, "chunks/s%d/o%d" % (sigma_gauss, offset))
    one = run(imgs, par, 64, device=True)                   # the same images contiguous: 3300 bytes, one chunk
    _same_bits(one, got, batch)


def _tiled_equals_sources(got, pick, rep, cap):
    """every image of the tiled batch has the bits of the first image made from the same source"""
    n = got["n_points"]
    assert np.array_equal(n, n[rep][pick])
    assert np.array_equal(got["row_stats"].view(np.uint32), got["row_stats"][rep][pick].view(np.uint32))
    assert np.array_equal(got["det_mask"], got["det_mask"][rep][pick])
    valid = np.arange(cap)[None, :] < n[:, None]
    assert np.array_equal(got["targets"][valid], got["targets"][rep][pick][valid])
    assert np.array_equal(got["xyzi"][valid].view(np.uint32), got["xyzi"][rep][pick][valid].view(np.uint32))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_more_images_than_a_grid_has_rows(device):
    """70000 sweeps of 4 x 48 bins: cen2018_rows_kernel has the image on gridDim.y, which ends at 65535, so a chunk holds at
    most that many images whatever their size.  Every image equals the restatement of its source."""
    src, pick, par = R.big_batch_case()
    refs = [R.cen2018(img, **par) for img in src]
    imgs = np.ascontiguousarray(src[pick])
    assert imgs.shape == (70000, 4, 48)
    got = run(imgs, par, 32, device=device)
    rep = np.array([int(np.nonzero(pick == s)[0][0]) for s in range(len(src))])
    compare({k: v[rep] for k, v in got.items()}, refs, src, "batch70000")
    _tiled_equals_sources(got, pick, rep, 32)
    want_n = np.array([len(r["targets"]) for r in refs], np.int32)
    assert np.array_equal(got["n_points"], want_n[pick])    # no source has an undecided row: the counts are complete
    assert int(pick[-1]) == 63 and int(got["n_points"][-1]) == want_n[63] and got["n_points"].shape == (70000,)


def test_refusals_and_recovery():
    from tbv_slam_public_amd import api, _lib as L
    name = "s5w511"
    imgs, par, _ = R.matrix_cases()[name]
    for bad, kw, status, word in ((np.zeros((33000, 15), np.uint8), dict(sigma_gauss=5), L.ERR_CAPACITY, "LDS"),
                                  (np.zeros((3, 8193), np.uint8), dict(sigma_gauss=5), L.ERR_INVALID_ARGUMENT, "8192")):
        with pytest.raises(L.CfearError) as e:
            api.filter_cen2018(bad, cap_points=16, **kw)
        assert e.value.status == status and word in str(e.value), (status, str(e.value))
        compare(run(imgs, par, _cap(name)), _ref(name), imgs, name)   # the same context, straight after


def test_legacy_filter_on_more_images_than_a_grid_has_rows():
    """cfear_filter_kstrongest_legacy: legacy_prepare_kernel has the image on gridDim.y too.  70000 images of 4 x 16 tiled
    from 64; each equals the oracle's legacy filter on its source, as test_legacy_k_strongest_filter_vs_oracle compares."""
    import torch
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    k, z, rr, md = 3, 60.0, 0.0438, 0.2
    src = np.stack([np.random.default_rng(9000 + s).integers(0, 256, (4, 16), dtype=np.uint8) for s in range(64)])
    pick = np.random.default_rng(9064).integers(0, 64, 70000)
    pick[:64] = np.arange(64)
    pick[-1] = 63
    exp = [O.kstrongest_legacy(img, k, z, rr, md) for img in src]
    assert max(e.shape[0] for e in exp) > 0
    imgs = np.ascontiguousarray(src[pick])
    h = api.k_strongest_filter(imgs, k, z, rr, md)
    d = api.k_strongest_filter(torch.from_numpy(imgs).cuda(), k, z, rr, md)
    torch.cuda.synchronize()
    api.default_context().synchronize()
    rep = np.arange(64)
    for r in (h, {kk: v.cpu().numpy() for kk, v in d.items()}):
        for s in range(64):
            assert r["n_points"][s] == exp[s].shape[0], (s, r["n_points"][s], exp[s].shape)
            np.testing.assert_array_equal(r["xyzi"][s, :exp[s].shape[0]], exp[s])
        n = r["n_points"]
        assert n.shape == (70000,) and np.array_equal(n, n[rep][pick])
        valid = np.arange(r["xyzi"].shape[1])[None, :] < n[:, None]
        assert np.array_equal(r["xyzi"][valid].view(np.uint32), r["xyzi"][rep][pick][valid].view(np.uint32))
