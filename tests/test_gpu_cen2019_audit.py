"""GPU: cfear_cen2019_order_audit against its NumPy definition (tests/cen2019_audit_cpu.py, which test_cen2019_audit_cpu.py
proves sound against the literal loops under shuffled tie orders).  Exact: every integer of the record, the two levels bit for
bit, targets, certain and marks.  Every input satisfies cen2019_cpu.mean_h_margin (asserted on the CPU, there and in
test_cen2019_cpu.py), so mean_h is the same float under any summation order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cen2019_audit_cpu as A
from tests import cen2019_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = A.RECORD_DTYPE.names[:14]


def _run(imgs, cap, device=False, marks=True, **par):
    from tbv_slam_public_amd import api
    kw = dict(cap_points=cap, want_targets=True, want_marks=marks, **par)
    if device:
        import torch
        x = imgs if hasattr(imgs, "data_ptr") else torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
        r = api.cen2019_order_audit(x, **kw)
        torch.cuda.synchronize()
        return {k: (v if k == "records" else v.cpu().numpy()) for k, v in r.items()}
    return api.cen2019_order_audit(imgs, **kw)


def _compare(got, b, ref, name):
    rec, want = got["records"][b], ref["record"][0]
    for f in INTS:
        assert int(rec[f]) == int(want[f]), (name, b, f, rec, want)
    for f in ("h_hi", "h_lo"):
        a, w = np.array(rec[f], np.float32), np.array(want[f], np.float32)
        assert (np.isnan(a) and np.isnan(w)) or a.view(np.uint32) == w.view(np.uint32), (name, b, f, rec, want)
    n = int(rec["n_targets"])
    assert np.array_equal(got["targets"][b, :n], ref["targets"]), (name, b, "targets")
    assert np.array_equal(got["certain"][b, :n], ref["certain"]), (name, b, "certain")
    if "marks" in got:
        assert np.array_equal(got["marks"][b], ref["marks"]), (name, b, "marks")


def _filter_agrees(got, b, img, mp, mr, name):
    from tbv_slam_public_amd import api
    f = api.filter_cen2019(img, max_points=mp, min_range_bins=mr, cap_points=got["targets"].shape[1], want_targets=True, want_counts=True)
    rec = got["records"][b]
    n = int(f["n_points"][0])
    assert n == int(rec["n_targets"]) and np.array_equal(f["targets"][0, :n], got["targets"][b, :n]), (name, "targets")
    assert f["counts"][0, :2].tolist() == [int(rec["n_candidates"]), int(rec["n_fresh"])], (name, "counts")


def _pre(name):
    if not hasattr(_pre, "c"):
        _pre.c = {}
    if name not in _pre.c:
        img = {**R.small_cases(), **R.facts_cases(), "straddle_tied": A.straddle_tied_case()}[name]
        _pre.c[name] = (img, A.prepare(img))
    return _pre.c[name]


def _max_points(pre):
    """the cut on, just before and just after both levels"""
    return sorted(set(R.max_points_of(int(pre["sure"].sum()))) | set(R.max_points_of(int(pre["possible"].sum()))))


@pytest.mark.parametrize("name", list(R.SHAPES) + list(R.facts_cases()) + ["straddle_tied"])
def test_kernels_equal_the_definition_at_every_max_points(name):
    img, pre = _pre(name)
    for mp in _max_points(pre):
        for mr in (0, 3) if mp == 8 else (0,):
            ref = A.audit(img, mp, mr, pre=pre)
            got = _run(img[None], len(ref["targets"]) + 8, max_points=mp, min_range_bins=mr)
            _compare(got, 0, ref, "%s/mp%d/mr%d" % (name, mp, mr))
            if mp in (8, 1000):
                _filter_agrees(got, 0, img, mp, mr, name)
    if name == "flat":
        assert np.isnan(got["records"][0]["h_hi"]) and int(got["records"][0]["n_candidates"]) == 0


@pytest.mark.parametrize("block", range(4))
def test_kernels_equal_the_definition_on_random_sweeps(block):
    """random_case(k), k < 200 (the four without a mean_h margin stay on the CPU), with the case's own max_points and
    min_range_bins and with the cut on and around both levels"""
    ks = [k for k in A.device_random_cases() if k // 50 == block]
    assert len(ks) >= 48
    for k in ks:
        img, mp0, mr0 = R.random_case(k)
        pre = A.prepare(img)
        for mp, mr in [(mp0, mr0)] + [(mp, 0) for mp in _max_points(pre)]:
            ref = A.audit(img, mp, mr, pre=pre)
            got = _run(img[None], len(ref["targets"]) + 4, max_points=mp, min_range_bins=mr)
            _compare(got, 0, ref, "random%d/mp%d/mr%d" % (k, mp, mr))
        _filter_agrees(got, 0, img, mp, 0, "random%d" % k)


def test_full_sweep_is_clear_at_1000_and_has_a_band_of_15_at_10000():
    img = R.synth_image(3, 3360)
    got = _run(img[None], 4096, marks=False, max_points=1000)["records"][0]
    assert got["n_marks_in"] == got["n_marks"] == got["n_marks_out"] == 1000 and got["n_targets"] == got["n_targets_certain"] == 123
    pre = A.prepare(img)
    ref = A.audit(img, 10000, 0, pre=pre)
    got = _run(img[None], 4096, device=True, max_points=10000)
    _compare(got, 0, ref, "synth/mp10000")
    assert got["records"][0]["n_band"] == 15 and got["records"][0]["n_targets_certain"] == 636


def test_batch_of_64_and_each_sweep_alone():
    imgs = R.batch64_case()
    whole = _run(imgs, 64, max_points=8)
    for b in range(64):
        _compare(whole, b, A.audit(imgs[b], 8, 0), "batch64")
        alone = _run(imgs[b:b + 1], 64, max_points=8)
        n = int(whole["records"][b]["n_targets"])
        assert alone["records"][0].tobytes() == whole["records"][b].tobytes(), b
        for k in ("targets", "certain"):                    # written up to n_targets
            assert np.array_equal(alone[k][0, :n], whole[k][b, :n]), (b, k)
        assert np.array_equal(alone["marks"][0], whole["marks"][b]), b
    three = _run(imgs[[5, 17, 9]], 64, max_points=8)
    assert three["records"][1].tobytes() == whole["records"][17].tobytes() and np.array_equal(three["marks"][1], whole["marks"][17])


@pytest.mark.parametrize("cols,pitch,batch_pad", list(R.pitch_cases()))
def test_row_pitch_odd_strides_and_batch_padding(cols, pitch, batch_pad):
    """the padding is 255 everywhere, so a kernel that read it would see returns that are not there"""
    import torch
    rows, batch = 9, 3
    imgs = R.pitch_cases()[(cols, pitch, batch_pad)]
    bstride = rows * pitch + batch_pad
    buf = np.full(batch * bstride + 5, 255, np.uint8)
    for b in range(batch):
        v = buf[5 + b * bstride: 5 + b * bstride + rows * pitch].reshape(rows, pitch)
        v[:, :cols] = imgs[b]
    t = torch.from_numpy(buf).cuda()
    view = torch.as_strided(t, (batch, rows, cols), (bstride, pitch, 1), 5)
    got = _run(view, 256, device=True, max_points=12, min_range_bins=1)
    for b in range(batch):
        _compare(got, b, A.audit(imgs[b], 12, 1), "pitch%d/%d" % (cols, pitch))


@pytest.mark.parametrize("name", ["8x40", "3x513", "7x4097", "tiled"])
def test_device_pointers(name):
    img, pre = _pre(name)
    for mp in (8, 15):
        ref = A.audit(img, mp, 0, pre=pre)
        _compare(_run(img[None], len(ref["targets"]) + 8, device=True, max_points=mp), 0, ref, name)


def test_records_alone_need_no_capacity():
    from tbv_slam_public_amd import api
    img, pre = _pre("6x64")
    r = api.cen2019_order_audit(img, max_points=8)
    assert sorted(r) == ["records"]
    assert r["records"][0].tobytes() == _run(img[None], 64, max_points=8)["records"][0].tobytes()
    assert int(r["records"][0]["n_targets"]) == int(A.audit(img, 8, 0, pre=pre)["record"][0]["n_targets"])


def test_capacity_comes_with_complete_records_and_a_good_call_follows():
    from tbv_slam_public_amd import api, _lib as L
    img, pre = _pre("7x4097")
    ref = A.audit(img, 1000, 0, pre=pre)
    n = len(ref["targets"])
    assert n > 4
    ctx = api.default_context()
    d = L.PolarDesc(rows=img.shape[0], cols=img.shape[1], stride=img.shape[1], batch=1, batch_stride=img.size)
    p = api.cen2019_params(max_points=1000)
    cap = n - 1
    rec = np.zeros(1, L.CEN2019_ORDER_RECORD_DTYPE)
    tg, ct = np.zeros((1, cap, 2), np.int32), np.zeros((1, cap), np.uint8)
    rc = ctx._lib.cfear_cen2019_order_audit(ctx.h, img.ctypes.data, C.byref(d), C.byref(p), rec.ctypes.data, tg.ctypes.data, ct.ctypes.data,
                                            cap, None)
    assert rc == L.ERR_CAPACITY
    for f in INTS:
        assert int(rec[0][f]) == int(ref["record"][0][f]), f
    assert np.array_equal(tg[0], ref["targets"][:cap]) and np.array_equal(ct[0], ref["certain"][:cap])
    # without the arrays the same sweep is no capacity error, whatever cap_points says
    rc = ctx._lib.cfear_cen2019_order_audit(ctx.h, img.ctypes.data, C.byref(d), C.byref(p), rec.ctypes.data, None, None, 0, None)
    assert rc == L.OK and int(rec[0]["n_targets"]) == n
    import torch
    with pytest.raises(L.CfearError) as e:
        api.cen2019_order_audit(torch.from_numpy(img).cuda(), max_points=1000, cap_points=cap, want_targets=True)
    assert e.value.status == L.ERR_CAPACITY
    _compare(_run(img[None], n, max_points=1000), 0, ref, "after capacity")


def test_every_refusal_is_followed_by_a_good_call():
    from tbv_slam_public_amd import api, _lib as L
    img, pre = _pre("8x40")
    ref = A.audit(img, 8, 0, pre=pre)

    def good():
        _compare(_run(img[None], 64, max_points=8), 0, ref, "after a refusal")

    for kw, word in ((dict(max_points=-1), "max_points"), (dict(min_range_bins=-1), "min_range")):
        with pytest.raises(L.CfearError) as e:
            api.cen2019_order_audit(img, **kw)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and word in str(e.value), (kw, str(e.value))
        good()
    for shape, word in (((4, 1), "cols"), ((1, 8193), "cols"), ((2049, 2048), "2^22"), ((40000, 64), "rows")):
        with pytest.raises(L.CfearError) as e:
            api.cen2019_order_audit(np.zeros(shape, np.uint8))
        assert e.value.status == L.ERR_INVALID_ARGUMENT and word in str(e.value), (shape, str(e.value))
        good()
    import torch
    ctx = api.default_context()
    d = L.PolarDesc(rows=8, cols=40, stride=40, batch=1, batch_stride=320)
    p = api.cen2019_params()
    rec = torch.zeros((1, 64), dtype=torch.uint8, device="cuda")
    tg = np.zeros((1, 16, 2), np.int32)
    f = ctx._lib.cfear_cen2019_order_audit
    assert f(ctx.h, img.ctypes.data, C.byref(d), C.byref(p), rec.data_ptr(), None, None, 0, None) == L.ERR_INVALID_ARGUMENT   # host image, device records
    good()
    hrec = np.zeros(1, L.CEN2019_ORDER_RECORD_DTYPE)
    assert f(ctx.h, img.ctypes.data, C.byref(d), C.byref(p), None, None, None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert f(ctx.h, img.ctypes.data, C.byref(d), C.byref(p), hrec.ctypes.data, tg.ctypes.data, None, 0, None) == L.ERR_INVALID_ARGUMENT
    assert f(ctx.h, img.ctypes.data, C.byref(d), C.byref(p), hrec.ctypes.data, None, None, -1, None) == L.ERR_INVALID_ARGUMENT
    good()


def test_cpp_mirror_runs(tmp_path):
    img, pre = _pre("tiled")
    ref = A.audit(img, 15, 0, pre=pre)
    exe = str(tmp_path / "cen2019_audit_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "cen2019_audit_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    raw = str(tmp_path / "sweep.bin")
    img.tofile(raw)
    out = subprocess.check_output([exe, raw, str(img.shape[0]), str(img.shape[1]), "15", "0"], timeout=120).decode().split("\n")
    rec = ref["record"][0]
    assert [int(v) for v in out[0].split()] == [int(rec[f]) for f in ("n_targets", "n_targets_certain", "n_band", "n_marks_in", "n_marks_out")] + \
        [int(rec["n_marks_in"] == rec["n_marks_out"])]
    rows = [[int(v) for v in line.split()] for line in out[1:1 + len(ref["targets"])]]
    assert rows == [t + [int(c)] for t, c in zip(ref["targets"].tolist(), ref["certain"].tolist())]
