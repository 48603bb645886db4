"""CPU: the NumPy definition of CartesianRadar / CorAlCartQuality (tests/cart_cpu.py) against an independent scalar loop in
double, its exact properties, the reference's quirks it keeps, and the C-ABI additions (struct sizes, defaults, symbols, the C++
mirror compiled against the stand-in headers)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import cart_cpu as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_cart_params_default", "cfear_polar_to_cartesian", "cfear_cart_quality_batch"]
TOL = 4 * 2.0 ** -24                    # four float roundings on values <= 1


def _sweep(rows=12, cols=64, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def _scalar_bilinear(src, ix, iy, fx, fy):
    """double precision, plain weights, taps outside read 0: nothing shared with R.bilinear"""
    H, Wd = src.shape
    out = np.zeros(ix.shape, np.float64)
    for i in range(ix.shape[0]):
        for j in range(ix.shape[1]):
            acc = 0.0
            for dy, wy in ((0, 1.0 - fy[i, j] / 32.0), (1, fy[i, j] / 32.0)):
                for dx, wx in ((0, 1.0 - fx[i, j] / 32.0), (1, fx[i, j] / 32.0)):
                    yy, xx = int(iy[i, j]) + dy, int(ix[i, j]) + dx
                    if 0 <= yy < H and 0 <= xx < Wd:
                        acc += float(src[yy, xx]) * wy * wx
            out[i, j] = acc
    return out


@pytest.mark.parametrize("W", [9, 10])
def test_definition_equals_scalar_loop(W):
    pol = _sweep()
    maps = R.fixed_maps(12, W, 0.04328, 0.5)
    cart = R.polar_to_cartesian(pol, 0.04328, 0.5, W, maps)
    assert cart.dtype == F and cart.shape == (W, W) and cart.max() <= 1.0 and cart.max() > 0.5
    want = _scalar_bilinear(R.to_float(pol), *maps)                         # the same converted input: convertTo is its own step
    assert np.abs(cart.astype(np.float64) - want).max() <= TOL
    # each warp of RotoTranslation, on its own input
    for M in (R.rotation_matrix(W, 0.7), [1.0, 0.0, float(F(0.37) / F(0.5)), 0.0, 1.0, float(F(-1.21) / F(0.5))], R.rotation_matrix(W, -40.0)):
        got = R.warp_affine(cart, M)
        want = _scalar_bilinear(cart, *R.warp_coords(R.invert(M), W))
        assert np.abs(got.astype(np.float64) - want).max() <= TOL
    out, rotated = R.roto_translation(cart, 0.37, -1.21, 0.7, 0.5, want_rotated=True)
    assert np.array_equal(rotated.view(np.uint32), R.warp_affine(cart, R.rotation_matrix(W, 0.7)).view(np.uint32))
    want = _scalar_bilinear(rotated, *R.warp_coords(R.invert([1.0, 0.0, float(F(0.37) / F(0.5)), 0.0, 1.0, float(F(-1.21) / F(0.5))]), W))
    assert np.abs(out.astype(np.float64) - want).max() <= TOL


def test_identity_translation_and_far_translation_are_exact():
    for W in (9, 10):
        cart = R.polar_to_cartesian(_sweep(), 0.04328, 0.5, W)
        q, warped = R.quality(cart, cart, 0.0, 0.0, 0.0, 0.5)
        assert np.array_equal(warped.view(np.uint32), cart.view(np.uint32)) and q == 0.0
        # 3 pixels right, 2 pixels up: an exact shift, zeros shifted in
        _, moved = R.quality(cart, cart, 3 * 0.5, -2 * 0.5, 0.0, 0.5)
        want = np.zeros_like(cart)
        want[:W - 2, 3:] = cart[2:, :W - 3]
        assert np.array_equal(moved.view(np.uint32), want.view(np.uint32))
        # further than the image is wide: nothing of the source is left, the score is the sum of the reference
        ref = R.polar_to_cartesian(_sweep(seed=4), 0.04328, 0.5, W)
        q, gone = R.quality(ref, cart, (W + 1) * 0.5, 0.0, 0.0, 0.5)
        assert not gone.any() and q == R.abs_diff(np.zeros_like(ref), ref) == float(np.cumsum(ref.astype(np.float64).ravel())[-1])


def test_quirk_darkened_seam():
    """angle lies in [-1, rows - 1): below 0 the upper row is row -1, which reads zeros (the cross-over interpolation is
    commented out, Utils.cpp:316-319), so the pixel is the row-0 value weighted by fy / 32 only."""
    rows, W = 12, 33
    ix, iy, fx, fy = R.fixed_maps(rows, W, 0.04328, 0.05)
    _, angle = R.float_maps(rows, W, 0.04328, 0.05)
    assert angle.min() >= -1.0 and angle.max() < rows - 1
    seam = (angle < 0) & (iy == -1) & (ix + 1 < 64)
    assert seam.sum() > 10 and np.array_equal(iy == -1, (angle < 0) & (iy < 0)) and iy.min() == -1
    white = R.polar_to_cartesian(np.full((rows, 64), 255, np.uint8), 0.04328, 0.05, W)
    assert np.array_equal(white[seam], fy[seam].astype(F) / F(32)) and white[seam].max() < 1.0     # elsewhere inside: 1.0
    inside = (iy >= 0) & (ix + 1 < 64)
    assert np.all(white[inside] == 1.0)
    pol = _sweep(rows, 64, 9)
    cart = R.polar_to_cartesian(pol, 0.04328, 0.05, W)
    f = R.to_float(pol)
    ax, ay = fx.astype(F) / F(32), fy.astype(F) / F(32)
    want = f[0][ix[seam]] * (ay[seam] * (F(1) - ax[seam])) + f[0][ix[seam] + 1] * (ay[seam] * ax[seam])
    assert np.array_equal(cart[seam].view(np.uint32), want.astype(F).view(np.uint32))


def test_quirk_yaw_in_radians_read_as_degrees():
    W = 33
    M = R.rotation_matrix(W, 0.5)
    assert M[0] == math.cos(math.radians(0.5)) and M[1] == math.sin(math.radians(0.5))
    cart = R.polar_to_cartesian(_sweep(), 0.04328, 0.12, W)
    got = R.roto_translation(cart, 0.0, 0.0, 0.5, 0.2384)
    half_degree = R.warp_affine(cart, [math.cos(math.radians(0.5)), math.sin(math.radians(0.5)), M[2], -math.sin(math.radians(0.5)),
                                       math.cos(math.radians(0.5)), M[5]])
    assert np.array_equal(got.view(np.uint32), half_degree.view(np.uint32))
    half_radian = R.warp_affine(cart, R.rotation_matrix(W, math.degrees(0.5)))
    assert np.abs(got - cart).mean() < 0.2 * np.abs(half_radian - cart).mean()          # half a degree barely moves the image


def test_quirk_reference_pose_is_ignored():
    src, off = (4.0, -3.0, 0.6), (0.5, -0.25, 0.01)
    a = R.pose_offset(src, off, ref_pose=(0.0, 0.0, 0.0))
    assert a == R.pose_offset(src, off, ref_pose=(100.0, 50.0, -2.0)) == R.pose_offset(src, off)
    np.testing.assert_allclose(a, off, rtol=0, atol=1e-14)                              # Tsrc^-1 Tsrc Toffset = Toffset
    from tbv_slam_public_amd import api
    assert api.cart_pose_offset(src, off, (100.0, 50.0, -2.0)) == a
    scans = [dict(R.cartesian_radar(_sweep(seed=s), T, W=9, cart_resolution=0.5)) for s, T in ((1, (0, 0, 0)), (2, (1.0, 0.5, 0.1)))]
    moved = [dict(scans[0], T=(30.0, -7.0, 1.0)), scans[1]]
    assert [d["score"] for d in R.evaluate(scans, 0.5)] == [d["score"] for d in R.evaluate(moved, 0.5)]


def test_quirk_two_rounding_rules():
    k = 5
    i, f = R.quantise_map(np.array([k + 1 / 64, k + 3 / 64, k + 5 / 64], F))            # cvRound: half to even
    assert i.tolist() == [k, k, k] and f.tolist() == [0, 2, 2]
    W = 9
    ix, iy, fx, fy = R.warp_coords(R.invert([1.0, 0.0, -(k + 1 / 64), 0.0, 1.0, 0.0]), W)   # (v * 1024 + 16) >> 5: half up
    assert np.array_equal(ix, np.broadcast_to(np.arange(W) + k, (W, W))) and np.all(fx == 1) and np.all(fy == 0)
    assert np.array_equal(iy, np.broadcast_to(np.arange(W)[:, None], (W, W)))
    ix, _, fx, _ = R.warp_coords(R.invert([1.0, 0.0, -(k + 3 / 64), 0.0, 1.0, 0.0]), W)
    assert np.all(fx == 2) and np.array_equal(ix[0], np.arange(W) + k)


def test_quirk_centre_pixel_and_min_range():
    cr = 0.2384
    assert R.cart_min_range(9, cr) == F(4) * F(cr)
    assert R.cart_min_range(10, cr) == F((5 - 0.5) * float(F(cr))) != F(5) * F(cr)
    r, angle = R.float_maps(12, 9, 0.04328, cr)
    assert r[4, 4] == 0.0 and (r >= 0).all()                                            # x = y = 0: (0 - res / 2) / res < 0, clamped
    ix, iy, fx, fy = R.fixed_maps(12, 9, 0.04328, cr)
    assert (ix[4, 4], fx[4, 4]) == (0, 0)
    r10, _ = R.float_maps(12, 10, 0.04328, cr)
    assert r10.min() > 0                                                                # no pixel at the origin


def test_struct_sizes_and_defaults():
    from tbv_slam_public_amd import _lib as L
    assert C.sizeof(L.CartParams) == 16 and C.sizeof(L.CartJob) == 40 and L.CART_RESULT_DTYPE.itemsize == 16
    assert L.CART_RESULT_DTYPE.fields["status"][1] == 8
    assert L.lib().cfear_abi_version() == 1
    p = L.CartParams(radar_resolution=1.0, cart_resolution=2.0, cart_pixel_width=7, pad=7)
    L.lib().cfear_cart_params_default(C.byref(p))
    assert (p.radar_resolution, p.cart_resolution, p.cart_pixel_width, p.pad) == (float(F(0.04328)), float(F(0.2384)), 300, 0)
    from tbv_slam_public_amd import api
    q = api.cart_params(cart_pixel_width=33)
    assert q.cart_pixel_width == 33 and q.cart_resolution == float(F(0.2384))
    with pytest.raises(KeyError):
        api.cart_params(nonsense=1)
    assert (R.RADAR_RESOLUTION, R.CART_RESOLUTION, R.CART_PIXEL_WIDTH) == (0.04328, 0.2384, 300)


def test_new_symbols_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared, s
        assert s in L.EXPORTS, s
        assert hasattr(lib, s), s
    assert "#define CFEAR_ABI_VERSION 1" in hdr and "#define CFEAR_CART_MAX_WIDTH 4096" in hdr


def test_quality_kind_of_cartesian_radar():
    from tbv_slam_public_amd import api
    for m in ("P2P", "P2L", "Coral", "keypoint_repetability", "anything"):
        assert api._quality_kind("CartesianRadar", m) == "CorAlCart"
    with pytest.raises(NotImplementedError):
        api._quality_kind("RawLidar", "Coral")
    with pytest.raises(NotImplementedError):
        api._quality_kind("RawLidar", "P2D")


def test_cpp_mirror_compiles_against_the_standins(tmp_path):
    exe = str(tmp_path / "cart_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "cart_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)
