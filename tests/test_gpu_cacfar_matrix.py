"""GPU: every CA-CFAR kernel instantiation against the oracle, bit for bit, at the smallest shape that reaches it.

tests/cacfar_cases.py holds one case per entry of the two dispatch tables (cacfar_rows_kernel: chunk width D, chunk count,
shorter last chunk, bitmap or key output, pre-filter on / off; cacfar_cols_kernel, the fused decode: D, last chunk,
pre-filter); tests/test_cacfar_plan_cpu.py shows without a GPU that each case reaches the entry it names, and here the
plan is asked again with the device address.  Every image sits in a buffer of 255s with the case's offset, row pitch and
batch stride, so a kernel that reads padding sees returns that are not there.  Both outputs are compared: the bitmap route
(cfear_filter_cacfar: cloud, count, mask) and the key route the batched odometry uses (cfear_filter_cacfar_rowkeys: per-row
counts and keys, including rows beyond kcap), the fused decode also against the rows kernel on the rotated image.
The oracle's answer is computed once per case and shared (read-only)."""
import functools

import numpy as np
import pytest

from tests import cacfar_cases as K

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name, z=None):
    """(images [batch, azimuths, bins], [(cloud, (row, bin)) per image]) from the oracle."""
    from oracle import pyoracle as O
    case = K.CASES[name]
    img = K.images(case)
    img.setflags(write=False)
    return img, [O.cacfar(img[b], *K.params(case, z)) for b in range(case.batch)]


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared reference images are read-only)


def _device(case, src):
    """The source images on the device, laid out as the case says, inside a buffer of 255s."""
    import torch
    buf, offset, shape, strides = K.buffer(case, src)
    t = torch.from_numpy(buf).cuda()
    view = torch.as_strided(t, shape, strides, storage_offset=offset)
    assert view.data_ptr() % 16 == offset
    return view


def _check_bitmap(case, view, img, ref, z=None):
    from tbv_slam_public_amd import api
    r = api.filter_cacfar(view, *K.params(case, z), want_mask=True)
    api.default_context().synchronize()
    r = {k: v.cpu().numpy() for k, v in r.items()}
    for b in range(img.shape[0]):
        cloud, rc = ref[b]
        assert r["n_points"][b] == cloud.shape[0], (case.name, b, r["n_points"][b], cloud.shape[0])
        np.testing.assert_array_equal(r["xyzi"][b, :cloud.shape[0]], cloud, err_msg="%s image %d" % (case.name, b))
        mask = np.zeros(img[b].shape, np.uint8)
        mask[rc[:, 0], rc[:, 1]] = 1
        np.testing.assert_array_equal(r["det_mask"][b], mask, err_msg="%s image %d" % (case.name, b))
    return r


def _check_keys(case, view, img, ref, bins_major, z=None):
    from tbv_slam_public_amd import api
    keys, cnt = api.filter_cacfar_rowkeys(view, *K.params(case, z), kcap=case.kcap, bins_major=bins_major)
    api.default_context().synchronize()
    keys, cnt = keys.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    for b in range(img.shape[0]):
        counts, want = K.expected_rows(img[b], ref[b][1], case.kcap)
        np.testing.assert_array_equal(cnt[b, :, 0], counts, err_msg="%s image %d: per-row counts" % (case.name, b))
        np.testing.assert_array_equal(keys[b], want, err_msg="%s image %d: keys" % (case.name, b))     # (zero beyond min(count, kcap))
    assert not cnt[:, :, 1].any()
    return keys, cnt


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_bitmap_output_equals_the_oracle(name):
    """cfear_filter_cacfar: n_points, xyzi and det_mask.  A cols-route case has no bitmap output of its own: its rotated image
    goes through the rows kernel here, with 16 / 32 / 48 azimuths."""
    case = K.CASES[name]
    img, ref = _ref(name)
    assert all(r[0].shape[0] > 0 for r in ref)
    if case.route == "rows":
        view = _device(case, img)
        p = K.plan(case, keys=False, base=view.data_ptr())
        assert p["table_index"] == K.entries(case)["bitmap"] and (p["D"], p["DL"], p["nch"], p["pre_on"]) == case.geom, p
    else:
        view = _cuda(img)
    _check_bitmap(case, view, img, ref)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_key_output_equals_the_oracle(name):
    """cfear_filter_cacfar_rowkeys: per row the oracle's count and its (bin, intensity) pairs as keys in ascending bin order; a
    row beyond kcap keeps its count and its first kcap keys.  Fused decode: the same keys as the rows kernel on the rotated image."""
    case = K.CASES[name]
    img, ref = _ref(name)
    assert all(r[0].shape[0] > 0 for r in ref)
    view = _device(case, K.source(case, img))
    p = K.plan(case, keys=True, base=view.data_ptr())
    assert p["table_index"] == K.entries(case)["keys"] and (p["D"], p["DL"], p["nch"], p["pre_on"]) == case.geom, p
    keys, cnt = _check_keys(case, view, img, ref, bins_major=case.route == "cols")
    if case.route == "cols":
        assert p["cols_supported"] == 1
        np.testing.assert_array_equal(np.rot90(view.cpu().numpy(), 1, axes=(1, 2)), img)
        keys_r, cnt_r = _check_keys(case, _cuda(img), img, ref, bins_major=False)
        np.testing.assert_array_equal(keys, keys_r)
        np.testing.assert_array_equal(cnt, cnt_r)


@pytest.mark.parametrize("z", [127, 128, 255])
@pytest.mark.parametrize("name", K.THRESHOLD_CASES)
def test_static_thresholds_on_either_side_of_128(name, z):
    """The byte test has one form below 128 and one from 128 on; at 255 nothing passes (the range window is emptied on the host)."""
    case = K.CASES[name]
    img, ref = _ref(name, z)
    n = sum(r[0].shape[0] for r in ref)
    assert (n == 0) == (z == 255)
    if case.route == "rows":
        _check_bitmap(case, _device(case, img), img, ref, z)
    _check_keys(case, _device(case, K.source(case, img)), img, ref, case.route == "cols", z)


@pytest.mark.parametrize("name", K.BATCH_POSITION_CASES)
def test_an_image_alone_equals_the_image_inside_its_batch(name):
    case = K.CASES[name]
    assert case.batch == 3
    img, ref = _ref(name)
    keys, cnt = _check_keys(case, _device(case, K.source(case, img)), img, ref, case.route == "cols")
    for b in range(3):
        one, ref1 = img[b:b + 1], ref[b:b + 1]
        k1, c1 = _check_keys(case, _device(case, K.source(case, one)), one, ref1, case.route == "cols")
        np.testing.assert_array_equal(k1[0], keys[b])
        np.testing.assert_array_equal(c1[0], cnt[b])
        if case.route == "rows":
            _check_bitmap(case, _device(case, one), one, ref1)


def test_unsupported_fused_decode_and_bad_arguments_are_refused():
    import torch
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    args = (40, 10, 0.01, 0.175, 20, 2.5)
    for shape in [(3360, 40), (3352, 48)]:                 # azimuths % 16, bins % 16
        with pytest.raises(L.CfearError) as e:
            api.filter_cacfar_rowkeys(torch.zeros(shape, dtype=torch.uint8, device="cuda"), *args, bins_major=True)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(L.CfearError):
        api.filter_cacfar_rowkeys(torch.zeros((8, 64), dtype=torch.uint8, device="cuda"), *args, kcap=0)
    with pytest.raises(L.CfearError):
        api.filter_cacfar_rowkeys(torch.zeros((8, 64), dtype=torch.uint8, device="cuda"), 0, 10, 0.01, 0.175, 20, 2.5)


@pytest.mark.parametrize("pitch", [0, 1])
@pytest.mark.parametrize("cols", K.NARROW_COLS)
def test_rows_narrower_than_one_piece(cols, pitch):
    """Rows of 1 .. 15 bins at stride = cols and cols + 1, several rows and images: no 16-byte piece of such an image but the
    first few ends inside it, so the rows take the byte path (tbv_slam_public_amd/csrc/row_pieces.hpp) -- k-strongest and
    CA-CFAR, keys and bitmap, equal the oracle."""
    import torch
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    from tests import test_gpu_filters as F
    rng = np.random.default_rng(100 * cols + pitch)
    batch, rows, stride = 2, 7, cols + pitch
    img = rng.integers(0, 256, size=(batch, rows, cols)).astype(np.uint8)
    buf = np.full(batch * rows * stride, 255, np.uint8)      # not a byte beyond the last image
    np.lib.stride_tricks.as_strided(buf, (batch, rows, cols), (rows * stride, stride, 1))[...] = img
    view = torch.as_strided(torch.from_numpy(buf).cuda(), (batch, rows, cols), (rows * stride, stride, 1))
    k, z = 3, 100
    keys, cnt = api.filter_kstrongest_rowkeys(view, k, z, 0.0438, 0.0)
    api.default_context().synchronize()
    F._rowkeys_check(keys, cnt, img, k, z, 0.0438, 0.0)
    args = (1, 0, 0.5, 0.175, 10, 0.0)                       # one cell per side, no guard: bins 1 .. cols - 2 have both windows
    ref = [O.cacfar(img[b], *args) for b in range(batch)]
    r = api.filter_cacfar(view, *args, want_mask=True)
    kk, cc = api.filter_cacfar_rowkeys(view, *args, kcap=16)
    api.default_context().synchronize()
    for b in range(batch):
        cloud, rc = ref[b]
        assert int(r["n_points"][b]) == cloud.shape[0]
        np.testing.assert_array_equal(r["xyzi"][b, :cloud.shape[0]].cpu().numpy(), cloud)
        mask = np.zeros((rows, cols), np.uint8)
        mask[rc[:, 0], rc[:, 1]] = 1
        np.testing.assert_array_equal(r["det_mask"][b].cpu().numpy(), mask)
        counts, want = K.expected_rows(img[b], rc, 16)
        np.testing.assert_array_equal(cc[b, :, 0].cpu().numpy(), counts)
        np.testing.assert_array_equal(kk[b].cpu().numpy().view(np.uint32), want)
    if cols >= 3:
        assert sum(x[0].shape[0] for x in ref) > 0
    p = api.cacfar_plan(rows, cols, *args, stride=stride, batch=batch, batch_stride=rows * stride, base=view.data_ptr())
    # the pieces that end inside the image, counted by hand: row r of an image is read whole iff r * stride + 16 <= rows * stride
    whole = sum(1 for r in range(rows) if r * stride + 16 <= rows * stride)
    aligned = [b for b in range(batch) if stride % 4 == 0 and (b * rows * stride) % 4 == 0]
    assert p["piece_rows"] == whole * len(aligned) and (stride >= 16 or p["piece_rows"] < p["total_rows"])
