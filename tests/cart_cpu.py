"""NumPy restatement of CartesianRadar and CorAlCartQuality (coral_alignment_quality/src/alignment_checker/ScanType.cpp:
191-209, Utils.cpp:255-339, AlignmentQuality.cpp:356-386).  It is the DEFINITION cfear_polar_to_cartesian and
cfear_cart_quality_batch are compared against: every float operation is its own rounding, in the reference's order (built
for baseline x86-64: no FMA).

  convertTo(CV_32F, 1 / 255.0)     f = float(u8) * float(1 / 255.0): a table of 256 floats
  radar_polar_to_cartesian         float maps (range bin, azimuth index) per Cartesian pixel, then cv::remap
  remap, float maps                cvRound(v * 32): 1/32-pixel coordinates rounded HALF TO EVEN, bilinear, constant border 0
  getRotationMatrix2D              about ((W - 1) / 2, (W - 1) / 2); the caller hands the yaw over in RADIANS as degrees
  warpAffine                       the matrix inverted in double, 1/1024-pixel integer maps, + 16 then >> 5: 1/32-pixel
                                   coordinates rounded HALF UP, bilinear, constant border 0
  RotoTranslation                  the rotation warp, then a translation warp of its OUTPUT by (x, y) / image_res pixels
  quality_                         {sum |warped - ref| over the floats, added in double, 0, 0}

UNPINNED: OpenCV is not available to this repository.  The arithmetic of remap, warpAffine, getRotationMatrix2D and convertTo
is restated from knowledge of OpenCV 4.2's imgproc; nothing here was compared with an OpenCV build.  The float maps use the
host libm's atan2f (through ctypes, not NumPy's arctan2, which may be a vector implementation of its own), as the library's
host code does.  cv::sum's own order of additions is not restated: the sum here is serial."""
import ctypes
import ctypes.util
import math

import numpy as np

from tests import p2p_cpu

F = np.float32
D = np.float64
RADAR_RESOLUTION, CART_RESOLUTION, CART_PIXEL_WIDTH = 0.04328, 0.2384, 300      # Utils.h: radar_polar_to_cartesian's defaults

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.restype = ctypes.c_float
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]


def to_float(polar_u8):
    """polar.convertTo(CV_32F, 1 / 255.0)"""
    table = np.arange(256).astype(F) * F(1 / 255.0)
    return table[np.asarray(polar_u8, np.uint8)]


def cart_min_range(W, cart_resolution):
    cr = F(cart_resolution)
    if W % 2 == 0:
        return F((W // 2 - 0.5) * float(cr))                      # a double product, stored in a float
    return F(F(W // 2) * cr)                                      # int * float: a float product


def float_maps(rows, W, radar_resolution=RADAR_RESOLUTION, cart_resolution=CART_RESOLUTION):
    """(range, angle) float32 [W, W]: the two maps radar_polar_to_cartesian hands to cv::remap (Utils.cpp:258-308)."""
    rr, cr = F(radar_resolution), F(cart_resolution)
    cmr = cart_min_range(W, cart_resolution)
    idx = np.arange(W).astype(F)
    y = np.broadcast_to((F(-1) * cmr + idx * cr)[None, :], (W, W))           # map_y[i][j]: a function of the column
    x = np.broadcast_to((cmr - idx * cr)[:, None], (W, W))                   # map_x[i][j]: a function of the row
    assert x.dtype == F and y.dtype == F
    xd, yd = x.astype(D), y.astype(D)
    r = ((np.sqrt(xd * xd + yd * yd) - float(F(rr / F(2)))) / float(rr)).astype(F)
    r = np.where(r < 0, F(0), r)
    theta = np.array([[_libm.atan2f(float(y[i, j]), float(x[i, j])) for j in range(W)] for i in range(W)], F)
    theta = np.where(theta < 0, (theta.astype(D) + 2 * math.pi).astype(F), theta)
    az0 = (1.0 / rows) * 2 * math.pi
    az_last = (float(rows) / rows) * 2 * math.pi
    step = (az_last - az0) / float(rows - 1)
    angle = ((theta.astype(D) - az0) / step).astype(F)
    return r, angle


def quantise_map(v):
    """cvRound(v * 32) of a float map (half to even) -> (integer part saturated to short, 5-bit fraction).  A coordinate
    whose product leaves the int range lands outside every image on either side of the saturation: 32767 here."""
    v = np.asarray(v, F)
    big = ~(np.abs(v) < F(2.0 ** 24))
    s = np.rint(np.where(big, F(0), v) * F(32)).astype(np.int64)
    i = np.where(big, 32767, np.clip(s >> 5, -32768, 32767))
    return i.astype(np.int32), (s & 31).astype(np.int32)


def _tap(src, iy, ix):
    H, Wd = src.shape
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < Wd)
    return np.where(ok, src[np.clip(iy, 0, H - 1), np.clip(ix, 0, Wd - 1)], F(0))


def bilinear(src, ix, iy, fx, fy):
    """remapBilinear on a float image with BORDER_CONSTANT 0: ((S00 w0 + S01 w1) + S10 w2) + S11 w3 in float."""
    src = np.asarray(src, F)
    ax, ay = fx.astype(F) * F(1 / 32), fy.astype(F) * F(1 / 32)
    w0, w1, w2, w3 = (F(1) - ay) * (F(1) - ax), (F(1) - ay) * ax, ay * (F(1) - ax), ay * ax
    out = ((_tap(src, iy, ix) * w0 + _tap(src, iy, ix + 1) * w1) + _tap(src, iy + 1, ix) * w2) + _tap(src, iy + 1, ix + 1) * w3
    assert out.dtype == F
    return out


def fixed_maps(rows, W, radar_resolution=RADAR_RESOLUTION, cart_resolution=CART_RESOLUTION):
    """(ix, iy, fx, fy) int32 [W, W]: x is the range bin, y the azimuth row."""
    r, angle = float_maps(rows, W, radar_resolution, cart_resolution)
    ix, fx = quantise_map(r)
    iy, fy = quantise_map(angle)
    return ix, iy, fx, fy


def polar_to_cartesian(polar_u8, radar_resolution=RADAR_RESOLUTION, cart_resolution=CART_RESOLUTION, W=CART_PIXEL_WIDTH, maps=None):
    """uint8 [rows, cols] -> float32 [W, W] (CartesianRadar's cart_ image).  maps: fixed_maps() of the geometry, to share."""
    polar_u8 = np.asarray(polar_u8, np.uint8)
    ix, iy, fx, fy = maps or fixed_maps(polar_u8.shape[0], W, radar_resolution, cart_resolution)
    return bilinear(to_float(polar_u8), ix, iy, fx, fy)


def rotation_matrix(W, angle_deg):
    """getRotationMatrix2D(Point2f((W - 1) / 2.0, (W - 1) / 2.0), angle_deg, 1.0) -> float64 [6]"""
    c = float(F((W - 1) / 2.0))
    a = float(angle_deg) * (math.pi / 180.0)
    alpha, beta = math.cos(a), math.sin(a)
    return np.array([alpha, beta, (1 - alpha) * c - beta * c, -beta, alpha, beta * c + (1 - alpha) * c], D)


def invert(M):
    """warpAffine's inversion of a forward matrix (no WARP_INVERSE_MAP), in double."""
    M = [float(v) for v in M]
    Dt = M[0] * M[4] - M[1] * M[3]
    Dt = 1.0 / Dt if Dt != 0 else 0.0
    A11, A22 = M[4] * Dt, M[0] * Dt
    M[0] = A11
    M[1] *= -Dt
    M[3] *= -Dt
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, D)


def warp_coords(Minv, W):
    """(ix, iy, fx, fy) int32 [W, W] of warpAffine's INTER_LINEAR maps: 10 fraction bits, + 16, >> 5 (half up)."""
    k = np.arange(W).astype(D)
    adelta = np.rint(Minv[0] * k * 1024.0).astype(np.int64)
    bdelta = np.rint(Minv[3] * k * 1024.0).astype(np.int64)
    X0 = np.rint((Minv[1] * k + Minv[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((Minv[4] * k + Minv[5]) * 1024.0).astype(np.int64) + 16
    X = X0[:, None] + adelta[None, :]
    Y = Y0[:, None] + bdelta[None, :]
    assert max(np.abs(X).max(), np.abs(Y).max()) < 2 ** 31            # signed 32-bit arithmetic in the reference
    X, Y = X >> 5, Y >> 5
    return (X >> 5).astype(np.int32), (Y >> 5).astype(np.int32), (X & 31).astype(np.int32), (Y & 31).astype(np.int32)


def warp_affine(src, M):
    src = np.asarray(src, F)
    assert src.shape[0] == src.shape[1]
    return bilinear(src, *warp_coords(invert(M), src.shape[0]))


def roto_translation(src, x, y, yaw, image_res, want_rotated=False):
    """RotoTranslation (Utils.cpp:325-339) of a float32 [W, W] image by the pose (x, y, yaw)."""
    src = np.asarray(src, F)
    rotated = warp_affine(src, rotation_matrix(src.shape[0], yaw))               # the yaw, in radians, as degrees
    tx, ty = F(F(x) / F(image_res)), F(F(y) / F(image_res))
    out = warp_affine(rotated, [1.0, 0.0, float(tx), 0.0, 1.0, float(ty)])
    return (out, rotated) if want_rotated else out


def abs_diff(a, b):
    d = np.abs(np.asarray(a, F) - np.asarray(b, F))
    assert d.dtype == F
    return float(np.cumsum(d.astype(D).ravel())[-1])                            # a serial sum in double


def quality(ref, src, x, y, yaw, image_res):
    """-> (abs_diff, warped): CorAlCartQuality's quality_[0] and the image it was taken from."""
    warped = roto_translation(src, x, y, yaw, image_res)
    return abs_diff(warped, ref), warped


def pose_offset(src_pose, Toffset=(0.0, 0.0, 0.0), ref_pose=None):
    """(x, y, yaw) of Tchange as Affine3dToEigVectorXYeZ reads it.  CorAlCartQuality takes BOTH Tsrc and Tref from the
    source scan (AlignmentQuality.cpp:363-364): Tchange = Tsrc^-1 Tsrc Toffset and ref_pose is ignored (it is accepted so
    that a test can say so).  Planar poses: eulerAngles(0, 1, 2)[2] = atan2(m10, m11)."""
    T = p2p_cpu.tchange(src_pose, src_pose, Toffset)
    return float(T[2]), float(T[5]), math.atan2(float(T[3]), float(T[4]))


def cartesian_radar(polar_u8, T, pose_id=0, radar_resolution=RADAR_RESOLUTION, cart_resolution=CART_RESOLUTION, W=CART_PIXEL_WIDTH, maps=None):
    """A CartesianRadar scan.  The reference's constructor calls radar_polar_to_cartesian with its DEFAULT arguments whatever
    pars says; the keywords exist so that tests can use small images."""
    return {"type": "CartesianRadar", "T": tuple(float(v) for v in T), "pose_id": pose_id,
            "cart": polar_to_cartesian(polar_u8, radar_resolution, cart_resolution, W, maps)}


def evaluate(scans, image_res=CART_RESOLUTION, scan_spacing=1, **pert):
    """scanEvaluator's pair loop (ScanEvaluator.cpp:65-109) with CorAlCartQuality as the measure."""
    vek = p2p_cpu.create_perturbations(**pert)
    out, index = [], 0
    for k in range(scan_spacing, len(scans)):
        ref, src = scans[k - 1], scans[k]
        index += 1
        dx, dy = float(ref["T"][0]) - float(src["T"][0]), float(ref["T"][1]) - float(src["T"][1])
        for verr in vek:
            score = quality(ref["cart"], src["cart"], *pose_offset(src["T"], verr, ref["T"]), image_res)[0]
            out.append(dict(index=index, ref_id=int(ref.get("pose_id", k - 1)), src_id=int(src.get("pose_id", k)),
                            distance=math.sqrt(dx * dx + dy * dy), score=[score, 0.0, 0.0], aligned=p2p_cpu.aligned(verr),
                            perturbation=list(verr), residuals=[0.0, 0.0, 0.0]))
    return out
