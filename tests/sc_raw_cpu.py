"""NumPy restatement of RSCManager::MakeRadarContext (place_recognition_radar RadarScancontext.cpp:41-57) with TBV's
reachable settings: cv::threshold(THRESH_TOZERO) of the 8-bit sweep, then cv::resize(..., INTER_AREA) to
num_ring x num_sector, as OpenCV 4.2 computes them (imgproc/src/thresh.cpp, imgproc/src/resize.cpp:
computeResizeAreaTab, resizeArea_<uchar, float>, resizeAreaFast_<uchar, int>).  It is the CPU checker of
cfear_sc_raw_descriptors; it is not pinned against OpenCV (OpenCV is not a dependency of this project).

Every float operation is an explicit np.float32 multiply or add in the order OpenCV performs it, and results are
rounded half to even (cvRound)."""
import math

import numpy as np

DBL_EPSILON = np.finfo(np.float64).eps
INTER_AREA = 3


class Refused(ValueError):
    """What the library refuses with CFEAR_ERR_INVALID_ARGUMENT."""


def area_tab(ssize, dsize):
    """computeResizeAreaTab for one axis: per output index d the list of (source index, float32 weight) in table
    order."""
    scale = 1.0 / (float(dsize) / float(ssize))
    tab = []
    for d in range(dsize):
        fs1 = d * scale
        fs2 = fs1 + scale
        cell = min(scale, ssize - fs1)
        s1, s2 = math.ceil(fs1), math.floor(fs2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        e = []
        if s1 - fs1 > 1e-3:
            e.append((s1 - 1, np.float32((s1 - fs1) / cell)))
        for s in range(s1, s2):
            e.append((s, np.float32(1.0 / cell)))
        if fs2 - s2 > 1e-3:
            e.append((s2, np.float32(min(min(fs2 - s2, 1.0), cell) / cell)))
        tab.append(e)
    return tab


def resize_path(H, W, R, S):
    """'fast' or 'general' as cv::resize picks for INTER_AREA from [H, W] to [R, S]; raises Refused otherwise."""
    sx, sy = 1.0 / (float(S) / W), 1.0 / (float(R) / H)
    if sx < 1 or sy < 1:
        raise Refused("INTER_AREA with a scale below 1 (upsampling) is not supported")
    ix, iy = int(np.rint(sx)), int(np.rint(sy))
    if abs(sx - ix) < DBL_EPSILON and abs(sy - iy) < DBL_EPSILON:
        if ix == 2 and iy == 2:
            raise Refused("INTER_AREA at exactly 2 x 2 is not supported")
        return "fast"
    return "general"


def threshold(img, radar_threshold):
    """cv::threshold(img, img, t, 255, THRESH_TOZERO) on 8U, as a copy: keep v where v > cvFloor(t)."""
    if not np.isfinite(radar_threshold):
        raise Refused("radar_threshold must be finite")
    t = math.floor(radar_threshold)
    if t < 0:
        return img.copy()
    if t >= 255:
        return np.zeros_like(img)
    return np.where(img > t, img, 0).astype(np.uint8)


def _round_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)            # saturate_cast<uchar>: cvRound, half to even


def resize_area(img, R, S):
    """cv::resize(img, Size(S, R), INTER_AREA) of a uint8 image [H, W] -> uint8 [R, S]."""
    H, W = img.shape
    if resize_path(H, W, R, S) == "fast":
        ix, iy = W // S, H // R
        box = img.astype(np.int64).reshape(R, iy, S, ix).sum(axis=(1, 3))
        return _round_u8(box.astype(np.float32) * np.float32(np.float32(1.0) / np.float32(ix * iy)))
    xt, yt = area_tab(W, S), area_tab(H, R)
    out = np.zeros((R, S), np.uint8)
    src = img.astype(np.float32)
    for dy in range(R):
        acc = None
        for sy, beta in yt[dy]:
            buf = np.zeros(S, np.float32)
            row = src[sy]
            for dx in range(S):
                b = np.float32(0.0)
                for sx, alpha in xt[dx]:
                    b = np.float32(b + np.float32(row[sx] * alpha))
                buf[dx] = b
            term = (beta * buf).astype(np.float32)
            acc = term if acc is None else (acc + term).astype(np.float32)
        out[dy] = _round_u8(acc)
    return out


def resize_area_fast_vec(img, R, S):
    """resize_area's general path, vectorised over the output columns (same operations, same order)."""
    H, W = img.shape
    if resize_path(H, W, R, S) == "fast":
        return resize_area(img, R, S)
    xt, yt = area_tab(W, S), area_tab(H, R)
    n = max(len(e) for e in xt)
    idx = np.zeros((S, n), np.int64)
    alp = np.zeros((S, n), np.float32)
    cnt = np.zeros(S, np.int64)
    for dx, e in enumerate(xt):
        cnt[dx] = len(e)
        for k, (sx, a) in enumerate(e):
            idx[dx, k], alp[dx, k] = sx, a
    src = img.astype(np.float32)
    buf = np.zeros((H, S), np.float32)                               # buf for every source row
    for k in range(n):
        live = cnt > k
        term = (src[:, idx[:, k]] * alp[None, :, k]).astype(np.float32)
        buf = np.where(live[None, :], (buf + term).astype(np.float32), buf)
    out = np.zeros((R, S), np.uint8)
    for dy in range(R):
        acc = None
        for sy, beta in yt[dy]:
            term = (beta * buf[sy]).astype(np.float32)
            acc = term if acc is None else (acc + term).astype(np.float32)
        out[dy] = _round_u8(acc)
    return out


def keys(desc):
    """makeRingkeyFromScancontext / makeSectorkeyFromScancontext (Scancontext.cpp:239-268): row and column means.
    The entries are integers, so every summation order gives the same double."""
    return desc.sum(axis=1) / desc.shape[1], desc.sum(axis=0) / desc.shape[0]


def raw_descriptor(img, num_ring=40, num_sector=120, radar_threshold=0.0, transpose=None, normalize=False,
                   interpolation=INTER_AREA):
    """MakeRadarContext of one stored sweep -> (desc float64 [R, S], ring key [R], sector key [S]).
    transpose: the stored sweep is azimuth-major and is read transposed (PNGReaderInterface::Get, tbv_slam utils.cpp:
    4-19, transposes when rows < cols); None follows that rule."""
    if normalize:
        raise Refused("normalize = true is not supported")
    if interpolation != INTER_AREA:
        raise Refused("only INTER_AREA is supported")
    img = np.asarray(img, np.uint8)
    if transpose is None:
        transpose = img.shape[0] < img.shape[1]
    im = img.T if transpose else img
    t = threshold(im, radar_threshold)
    d = resize_area_fast_vec(np.ascontiguousarray(t), num_ring, num_sector).astype(np.float64)
    rk, sk = keys(d)
    return d, rk, sk
