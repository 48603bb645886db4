"""CPU: the Cen2018 restatement (tests/cen2018_cpu.py) against an independent float64 form, its defining properties, the
undecided-bin cap on every input the GPU tests use, what the matrix inputs claim to hold, and the C-ABI additions (symbols,
struct size, defaults, refusals)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cen2018_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_cen2018_params_default", "cfear_filter_cen2018"]
UNDECIDED_ROW_CAP = 0.005


def _cases():
    if not hasattr(_cases, "c"):
        _cases.c = R.gpu_cases()
    return _cases.c


@pytest.mark.parametrize("name", ["noise", "w51", "w257", "s5w100", "s9"])
def test_restatement_equals_float64_form_on_decided_bins(name):
    """Rows of up to 1000 bins.  On 3360-bin rows the two serial float32 sums move sigma by up to 5.2e-5 of its value against
    a float64 mean (measured on the synthetic scene: 3 of 1 344 000 bins outside the undecided band then fall on the other
    side of the threshold, the furthest 3.5e-5 of thres away) -- that is the order dependence the kernel has to reproduce,
    and the GPU tests pin it bit for bit; an order-free float64 form cannot."""
    imgs, par = _cases()[name]
    img = imgs[0]
    r = R.cen2018(img, **par)
    y64, t64 = R.float64_form(img, par["zq"], par["sigma_gauss"], par["min_range_bins"])
    in_range = np.arange(img.shape[1])[None, :] >= par["min_range_bins"]
    m64 = (y64 > t64) & in_range
    decided = ~r["undecided"]
    assert np.array_equal(r["mask"].astype(bool)[decided], m64[decided])
    assert r["mask"].any() and not r["mask"].all()
    assert np.max(np.abs(r["y"] - y64)) < 1e-5


def test_all_zero_row_has_default_sigma_and_no_target():
    img = R.speckle_image(3, 8, 120)
    img[5] = 0
    r = R.cen2018(img, min_range_bins=0)
    assert r["sigma"][5] == np.float32(0.034) and r["mean"][5] == 0
    assert not r["mask"][5].any() and not (r["targets"][:, 0] == 5).any()


def _flat_with(cols, spans, level=200, floor=10):
    img = np.full((4, cols), floor, np.uint8)
    for a, b in spans:
        img[1, a:b] = level
    return img


def test_isolated_strong_bin_gives_one_target_at_that_bin():
    img = _flat_with(200, [(90, 91)])
    r = R.cen2018(img, min_range_bins=2)
    t = r["targets"][r["targets"][:, 0] == 1]
    assert t.tolist() == [[1, 90]]


def test_even_run_emits_element_len_over_two_and_last_bin_run_is_emitted():
    img = _flat_with(200, [(60, 64), (197, 200)])
    r = R.cen2018(img, min_range_bins=2)
    m = r["mask"][1].astype(bool)
    assert m[60:64].all() and not m[59] and not m[64] and m[197:200].all()
    t = r["targets"][r["targets"][:, 0] == 1][:, 1].tolist()
    assert t == [62, 198]                                   # run[4 // 2] = 60 + 2; run[3 // 2] = 197 + 1, emitted after the loop
    assert R.runs_to_targets(np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], bool)).tolist() == [1, 5, 8]


def test_nothing_below_min_range_bins():
    img = _flat_with(200, [(0, 3), (30, 32)])
    r0 = R.cen2018(img, min_range_bins=0)
    assert r0["mask"][1, 0:3].all()
    r = R.cen2018(img, min_range_bins=40)
    assert not r["mask"][:, :40].any() and (r["targets"][:, 1] >= 40).all()
    r2 = R.cen2018(img, min_range_bins=2)                   # the run 0..2 is cut to bin 2: its only element
    assert r2["targets"][r2["targets"][:, 0] == 1][:, 1].tolist() == [2, 31]


def test_point_coordinates_follow_the_reference_loop():
    img = R.speckle_image(5, 16, 150)
    r = R.cen2018(img, range_res=0.0438)
    assert len(r["targets"]) > 4
    for (i, b), pt in zip(r["targets"], r["xyzi"]):
        theta = (float(i + 1) / 16) * 2.0 * math.pi
        rr = 0.0438 * int(b)                                # the bin edge: no half-bin offset
        assert pt[0] == np.float32(rr * math.cos(theta)) and pt[1] == np.float32(rr * math.sin(theta))
        assert pt[2] == 0 and pt[3] == float(img[i, b])
    key = r["targets"][:, 0].astype(np.int64) * 1000 + r["targets"][:, 1]
    assert (np.diff(key) > 0).all()                         # rows ascending, bins ascending within a row


def test_taps_are_normalised_and_symmetric():
    for s in (1, 5, 17):
        w, mu = R.taps(s)
        assert w.size == 3 * s and mu == (3 * s) // 2 and w.dtype == np.float32
        assert np.array_equal(w, w[::-1]) and abs(float(w.sum()) - 1) < 1e-6


@pytest.mark.parametrize("name", ["synth3360", "synth3768", "noise", "noise_lo", "w51", "w52", "w64", "w100", "w257", "s5w15", "s5w16",
                          "s5w100", "s5w257", "s9", "batch64", "compose"])
def test_undecided_rows_stay_under_the_cap_on_every_gpu_input(name):
    """A bin is undecided when |y - thres| <= 8 * 2^-23 * max(|y|, thres): y is four float operations on values that may
    differ by one ulp of exp, about six half-ulps, rounded up to 8.  Rows holding such a bin may be at most 0.5 % of a
    test's rows; the seeds of cen2018_cpu.gpu_cases() are chosen so that this holds."""
    imgs, par = _cases()[name]
    bad = total = 0
    for img in imgs:
        r = R.cen2018(img, **par)
        bad += int(r["undecided"].any(axis=1).sum())
        total += img.shape[0]
    print("undecided rows %s: %d of %d" % (name, bad, total))
    assert bad <= UNDECIDED_ROW_CAP * total, (name, bad, total)


def test_undecided_rows_of_the_strided_parameter_and_mirror_inputs():
    groups = [("pitch", list(R.pitch_cases().values())), ("parameters", R.parameter_cases()),
              ("mirror", [(R.mirror_case()[0][None], R.mirror_case()[1])])]
    for name, group in groups:
        bad = total = 0
        for imgs, par in group:
            for img in imgs:
                bad += int(R.cen2018(img, **par)["undecided"].any(axis=1).sum())
                total += img.shape[0]
        print("undecided rows %s: %d of %d" % (name, bad, total))
        assert bad <= UNDECIDED_ROW_CAP * total, (name, bad, total)


def _matrix():
    if not hasattr(_matrix, "c"):
        _matrix.c = R.matrix_cases()
    return _matrix.c


def _word_span(a, b):
    """64-bin words the run [a, b) touches"""
    return (b - 1) // 64 - a // 64 + 1


@pytest.mark.parametrize("name", sorted(R.matrix_cases().keys()))
def test_matrix_inputs_meet_the_cap_and_are_what_they_claim(name):
    """Every input of tests/test_gpu_cen2018_matrix.py: the undecided-row cap (zero rows for a case of fewer than 200), and
    the facts the case is there for, read off the restatement's mask."""
    imgs, par, facts = _matrix()[name]
    cols = imgs.shape[2]
    bad = total = 0
    runs, targets = [], []
    for img in imgs:
        r = R.cen2018(img, **par)
        bad += int(r["undecided"].any(axis=1).sum())
        total += img.shape[0]
        runs += [ab for i in range(img.shape[0]) for ab in R.runs_of(r["mask"][i])]
        targets += r["targets"][:, 1].tolist()
    print("undecided rows %s: %d of %d" % (name, bad, total))
    assert bad <= UNDECIDED_ROW_CAP * total, (name, bad, total)
    assert set(facts) <= {"long", "long_hi", "whole", "hi", "last_word"}
    assert ("hi" in facts) == (cols > 4096)                 # every case above 4096 bins holds a target up there
    if "long" in facts:
        assert any(_word_span(a, b) >= 3 for a, b in runs) and any(a == 0 for a, b in runs) and any(b == cols for a, b in runs)
    if "long_hi" in facts:
        assert any(_word_span(a, b) >= 3 and b > 4096 for a, b in runs)
    if "whole" in facts:
        assert sum(1 for a, b in runs if (a, b) == (par["min_range_bins"], cols)) >= len(R.CONSTANT_ROWS)
    if "hi" in facts:
        assert any(t >= 4096 for t in targets)
    if "last_word" in facts:
        assert par["min_range_bins"] >= (cols - 1) // 64 * 64 and len(targets) > 0
    if par["min_range_bins"] >= cols:
        assert not runs


def test_matrix_holds_every_width_filter_row_count_and_parameter_edge():
    m = _matrix()
    for sg in R.MATRIX_FILTERS:
        for cols in R.MATRIX_WIDTHS:
            imgs, par, facts = m["s%dw%d" % (sg, cols)]
            assert imgs.shape[0] == 2 and imgs.shape[1] % 2 == 1 and imgs.shape[2] == cols and par["sigma_gauss"] == sg
            assert "long" in facts and (cols <= 4096 or "hi" in facts)
    assert [m["rows%d" % r][0].shape[1:] for r in R.MATRIX_ROW_COUNTS] == [(r, 48) for r in R.MATRIX_ROW_COUNTS]
    for cols in (200, 4097, 8192):
        for mr in (0, 2):
            imgs, par, facts = m["zq-1w%dm%d" % (cols, mr)]
            assert par["zq"] == -1.0 and [int(row[0]) for row in imgs[0][:6]] == list(R.CONSTANT_ROWS) and "whole" in facts
            assert (imgs[0][:6] == imgs[0][:6, :1]).all() and m["zq0w%dm%d" % (cols, mr)][1]["zq"] == 0.0
    assert m["s341w8192"][1]["sigma_gauss"] == 341 and m["s341w1023"][0].shape[2] == 3 * 341 and m["s1w3"][1]["sigma_gauss"] == 1
    assert [m["w200m%d" % mr][1]["min_range_bins"] for mr in (195, 199, 200, 205)] == [195, 199, 200, 205]


def test_constants_left_out_under_zq_zero_are_the_undecidable_ones():
    """zq == 0: a row of one value whose float mean is that value has q == p == y == 0 == thres in every bin, which the
    restatement cannot decide; the matrix keeps exactly the constants for which that is not so."""
    for cols, sg in ((200, 5), (4097, 17), (8192, 9)):
        img = np.concatenate([np.full((1, cols), v, np.uint8) for v in R.CONSTANT_ROWS])
        r = R.cen2018(img, zq=0.0, sigma_gauss=sg, min_range_bins=0)
        und = r["undecided"].any(axis=1)
        assert tuple(v for v, u in zip(R.CONSTANT_ROWS, und) if not u) == R.ZERO_ZQ_CONSTANTS[cols]
        assert (r["y"][und] == 0).all() and (r["thres"][und] == 0).all()


def test_undecided_rows_of_the_chunk_and_large_batch_inputs():
    src, pick, par = R.big_batch_case()
    refs = [R.cen2018(img, **par) for img in src]
    assert not any(r["undecided"].any() for r in refs) and max(len(r["targets"]) for r in refs) <= 32
    assert pick.shape == (70000,) and set(pick.tolist()) == set(range(64))
    for sg in (5, 17):
        imgs, par = R.chunk_case(sg)
        assert imgs.shape == (11, 3, 100)
        assert not any(R.cen2018(img, **par)["undecided"].any() for img in imgs)


def test_case_list_is_complete():
    assert sorted(_cases().keys()) == sorted(["synth3360", "synth3768", "noise", "noise_lo", "w51", "w52", "w64", "w100", "w257",
                                              "s5w15", "s5w16", "s5w100", "s5w257", "s9", "batch64", "compose"])


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_built_and_struct_size():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(L.Cen2018Params) == 24 and C.sizeof(L.PolarDesc) == 24
    assert L.Cen2018Params.range_res.offset == 16
    assert lib.cfear_abi_version() == 1


def test_defaults_are_the_reference_settings():
    from tbv_slam_public_amd import _lib as L, api
    p = L.Cen2018Params(zq=9.0, sigma_gauss=9, min_range_bins=9, pad=9, range_res=9.0)
    L.lib().cfear_cen2018_params_default(C.byref(p))
    assert (p.zq, p.sigma_gauss, p.min_range_bins, p.pad, p.range_res) == (3.0, 17, 2, 0, 0.04328)
    assert api.cen2018_params(sigma_gauss=5).sigma_gauss == 5
    with pytest.raises(KeyError):
        api.cen2018_params(nonsense=1)


def test_refusals_need_no_device():
    """Arguments are checked before the context is touched, so the refusals can be provoked without a GPU (with no
    context the status is all there is; tests/test_gpu_cen2018.py reads the messages)."""
    from tbv_slam_public_amd import _lib as L
    lib = L.lib()
    img = np.zeros((4, 64), np.uint8)
    xyzi = np.zeros((1, 16, 4), np.float32)
    n = np.zeros(1, np.int32)

    def call(cols=64, n_ptr=n.ctypes.data, **kw):
        d = L.PolarDesc(rows=4, cols=cols, stride=64, batch=1, batch_stride=256)
        p = L.Cen2018Params()
        lib.cfear_cen2018_params_default(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.cfear_filter_cen2018(None, img.ctypes.data, C.byref(d), C.byref(p), xyzi.ctypes.data, n_ptr, 16, None, None, None)

    assert call(sigma_gauss=16) == L.ERR_INVALID_ARGUMENT            # even
    assert call(sigma_gauss=0) == L.ERR_INVALID_ARGUMENT
    assert call(cols=50, sigma_gauss=17) == L.ERR_INVALID_ARGUMENT   # cols < 3 * sigma_gauss
    assert call(n_ptr=None, sigma_gauss=5) == L.ERR_INVALID_ARGUMENT
    assert call(sigma_gauss=5, min_range_bins=-1) == L.ERR_INVALID_ARGUMENT
    assert call(sigma_gauss=5, zq=float("nan")) == L.ERR_INVALID_ARGUMENT


def test_cpp_mirror_compiles_against_the_cv_bridge_standin(tmp_path):
    exe = str(tmp_path / "cen2018_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "cen2018_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)
