"""Host-side mirror of the reference's `cfear_radarodometry` class API over the C-ABI.

Names, argument meaning and error behaviour follow namespace CFEAR_Radarodometry:
  radarDriver            radar_driver.h:32-118        (filters: radar_filters.h / cfar.h)
  MapPointNormal         pointnormal.h:110-243
  n_scan_normal_reg      n_scan_normal.h:27-85 (+ Registration, registration.h:68-133)
  OdometryKeyframeFuser  odometrykeyframefuser.h:72-249  (batched over independent streams here)
with ROS / PCL / Eigen types replaced by NumPy arrays (host) or torch CUDA tensors (device):
  pcl::PointCloud<PointXYZI>  ->  float32 [n,4] (x, y, z, intensity)
  Eigen::Affine3d (planar)    ->  float64 (x, y, theta)  [Affine3dToVectorXYeZ, utils.cpp:115-122]
Everything computes in libcfear_hip.so on the GPU; there is no CPU path in this package.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _lib as L


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ptr(x):
    """(address, keepalive) of a NumPy array (host) or torch tensor (device)."""
    if x is None:
        return None, None
    if _is_torch(x):
        assert x.is_contiguous()
        return x.data_ptr(), x
    assert x.flags["C_CONTIGUOUS"]
    return x.ctypes.data, x


def _torch_ready(ctx, *arrays):
    """Waits until the work torch has queued on its current stream -- the fill of a fresh tensor, the copy behind a
    torch.stack -- is finished, when one of `arrays` is a torch tensor and `ctx` enqueues on a stream of its own.  A private
    stream is non-blocking: without the wait a kernel of the context may read such a tensor before torch has written it, or
    have its output overwritten by a fill that was queued first.  Nothing to do where the context shares torch's stream
    (default_context()): there the stream orders the two."""
    if not any(_is_torch(a) for a in arrays):
        return
    import torch
    ts = int(torch.cuda.current_stream(ctx.device).cuda_stream) or 1      # torch's null stream: hipStreamLegacy
    if ctx.stream_handle() != ts:
        torch.cuda.current_stream(ctx.device).synchronize()


class Context:
    """cfear_ctx: one per host thread / HIP stream.  `stream` = a hipStream_t handle to enqueue on; None or 0 (which is
    also what torch reports for its default stream) gives the context a PRIVATE non-blocking stream: work torch has queued
    that produces this context's inputs must then be synchronised by the caller (default_context() passes hipStreamLegacy
    for torch's default stream instead, which orders the two)."""

    default_options = {}      # {L.OPT_*: value} applied to every new context (measurement scripts: bench.py --ctx-option)

    def __init__(self, device=0, stream=None):
        self._lib = L.lib()
        h = C.c_void_p()
        rc = self._lib.cfear_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != L.OK:
            raise L.CfearError(rc, self._lib.cfear_status_string(rc).decode() +
                               " (libcfear_hip needs an MI355X; there is no CPU fallback)")
        self.h = h
        self.device = device
        for opt, val in Context.default_options.items():
            self.set_option(opt, val)

    def check(self, rc, allowed=()):
        if rc != L.OK and rc not in allowed:
            raise L.CfearError(rc, self._lib.cfear_last_error(self.h).decode())
        return rc

    def synchronize(self):
        self.check(self._lib.cfear_ctx_synchronize(self.h))

    def stream_handle(self):
        """The hipStream_t this context enqueues on, as an int (the caller's stream, or the private one)."""
        s = C.c_void_p()
        self.check(self._lib.cfear_ctx_get_stream(self.h, C.byref(s)))
        return int(s.value or 0)

    def shares_torch_stream(self):
        """True when work enqueued on torch's CURRENT stream is ordered with this context's kernels without a host
        synchronisation: the two are the same HIP stream (torch's default stream reports 0 -- a context given 0 made a
        private stream, so 0 never counts as shared)."""
        import torch
        ts = int(torch.cuda.current_stream().cuda_stream)
        return ts != 0 and ts == self.stream_handle()

    def set_option(self, option, value):
        """cfear_ctx_set_option: the test / measurement hooks of include/cfear_hip.h (L.OPT_*)."""
        self.check(self._lib.cfear_ctx_set_option(self.h, int(option), int(value)))

    def get_option(self, option):
        v = C.c_int64()
        self.check(self._lib.cfear_ctx_get_option(self.h, int(option), C.byref(v)))
        return int(v.value)

    def profile_enable(self, on=True):
        """True / 1: every kernel family; 2: only the polar filter's row kernels; False / 0: off."""
        self.check(self._lib.cfear_ctx_profile_enable(self.h, int(on)))

    def profile_read(self, reset=True):
        """{kernel family: (total_ms, launches)} measured with hipEvents on the context's stream."""
        cap = 32
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        cnt = (C.c_int64 * cap)()
        n = self._lib.cfear_ctx_profile_read(self.h, names, ms, cnt, cap, int(reset))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(n, cap))}

    def close(self):
        if getattr(self, "h", None):
            self._lib.cfear_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT_CTX = None


def default_context():
    """The process-wide context on device 0.  It enqueues on torch's current stream, so kernels launched through
    the mirror are ordered with torch work on the tensors they read and write (device-pointer calls are
    asynchronous, include/cfear_hip.h)."""
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        stream = None
        try:
            import torch
            if torch.cuda.is_available():
                # torch's default stream is the null stream (handle 0): address it as hipStreamLegacy (1)
                stream = torch.cuda.current_stream(0).cuda_stream or 1
        except ImportError:
            pass
        _DEFAULT_CTX = Context(0, stream)
    return _DEFAULT_CTX


# ------------------------------------------------------------------------------------------------
# radarDriver
# ------------------------------------------------------------------------------------------------
class radarDriverParameters:
    """radarDriver::Parameters (radar_driver.h:35-84); float members are float32 like the reference."""

    def __init__(self, z_min=60.0, range_res=0.0438, azimuths=400, k_strongest=12, nb_guard_cells=20,
                 window_size=10, false_alarm_rate=0.01, min_distance=2.5, max_distance=200.0,
                 dataset="oxford", filter_type="kstrong"):
        self.z_min, self.range_res, self.azimuths, self.k_strongest = z_min, range_res, azimuths, k_strongest
        self.nb_guard_cells, self.window_size, self.false_alarm_rate = nb_guard_cells, window_size, false_alarm_rate
        self.min_distance, self.max_distance = min_distance, max_distance
        self.dataset, self.filter_type = dataset, filter_type


def _desc(img):
    if img.ndim == 2:
        rows, cols = img.shape
        batch = 1
    else:
        batch, rows, cols = img.shape
    d = L.PolarDesc()
    d.rows, d.cols, d.stride, d.batch = rows, cols, cols, batch
    d.batch_stride = rows * cols
    return d, batch, rows, cols


def polar_rotate_ccw(img, ctx=None):
    """cv::rotate(ROTATE_90_COUNTERCLOCKWISE) of radarDriver::Callback (radar_driver.cpp:74-90) for a uint8 image
    [bins, azimuths] or a batch [b, bins, azimuths] -> [azimuths, bins] / [b, azimuths, bins] (NumPy -> NumPy,
    torch CUDA -> torch CUDA); out[i, j] = img[j, azimuths - 1 - i]."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    shape = (cols, rows) if img.ndim == 2 else (batch, cols, rows)
    if _is_torch(img):
        import torch
        img = img.contiguous()
        out = torch.empty(shape, dtype=torch.uint8, device=img.device)
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        out = np.empty(shape, np.uint8)
    ctx.check(ctx._lib.cfear_polar_rotate_ccw(ctx.h, _ptr(img)[0], C.byref(d), _ptr(out)[0], rows, rows * cols))
    return out


def filter_kstrongest(img, k, z_min, range_res, min_distance, want_peaks=False, ctx=None):
    """StructuredKStrongest (radar_filters.cpp:198-337) for a uint8 image [rows, cols] or a batch
    [b, rows, cols] (NumPy -> NumPy results, torch CUDA tensor -> torch CUDA results; a torch view with a row pitch or a
    batch stride is used in place).
    Returns dict(sel_range, sel_intensity, sel_count, is_peak, xyzi, n_points, xyzi_peaks, n_peaks)."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    par = L.KStrongParams(int(k), float(z_min), float(range_res), float(min_distance), int(bool(want_peaks)))
    if _is_torch(img):
        import torch
        assert img.dtype == torch.uint8 and img.stride(-1) == 1
        d.stride = img.stride(-2)
        d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
        dev = img.device
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        res = dict(sel_range=mk((batch, rows, k), torch.int32), sel_intensity=mk((batch, rows, k), torch.uint8),
                   sel_count=mk((batch, rows), torch.int32), xyzi=mk((batch, rows * k, 4), torch.float32),
                   n_points=mk((batch,), torch.int32))
        if want_peaks:
            res.update(is_peak=mk((batch, rows, k), torch.uint8), xyzi_peaks=mk((batch, rows * k, 4), torch.float32),
                       n_peaks=mk((batch,), torch.int32))
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        res = dict(sel_range=np.empty((batch, rows, k), np.int32), sel_intensity=np.empty((batch, rows, k), np.uint8),
                   sel_count=np.empty((batch, rows), np.int32), xyzi=np.empty((batch, rows * k, 4), np.float32),
                   n_points=np.empty((batch,), np.int32))
        if want_peaks:
            res.update(is_peak=np.empty((batch, rows, k), np.uint8),
                       xyzi_peaks=np.empty((batch, rows * k, 4), np.float32), n_peaks=np.empty((batch,), np.int32))
    out = L.KStrongOut()
    for name in ("sel_range", "sel_intensity", "sel_count", "is_peak", "xyzi", "n_points", "xyzi_peaks", "n_peaks"):
        setattr(out, name, _ptr(res.get(name))[0])
    p = img.data_ptr() if _is_torch(img) else _ptr(img)[0]
    ctx.check(ctx._lib.cfear_filter_kstrongest(ctx.h, p, C.byref(d), C.byref(par), C.byref(out)))
    return res


def filter_kstrongest_rowkeys(img, k, z_min, range_res, min_distance, bins_major=False, two_pass=False, tile_sweep=False, route=0, ctx=None):
    """cfear_filter_kstrongest_rowkeys: the batched odometry's filter stage on its own, for a torch CUDA uint8 image
    [rows, cols] or batch [b, rows, cols]; bins_major: the images are [range bins][azimuths] and are decoded (rotated
    counter-clockwise, radar_driver.cpp:74-90) by the sweep itself (two_pass: by the rotation kernel first; tile_sweep:
    every 16-column tile through the LDS transposition instead of the candidate lists; route 1 / 2: the lists in global
    memory / one workgroup per image whatever the batch size).
    Returns (row_keys uint32-as-int32 [b, azimuths, k], row_counts int32 [b, azimuths, 2]) as CUDA tensors."""
    import torch
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    assert img.dtype == torch.uint8 and img.stride(-1) == 1      # a view with a row pitch / batch stride is fine
    d.stride = img.stride(-2)
    d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
    az = cols if bins_major else rows
    par = L.KStrongParams(int(k), float(z_min), float(range_res), float(min_distance), 0)
    keys = torch.zeros((batch, az, k), dtype=torch.int32, device=img.device)
    cnt = torch.zeros((batch, az, 2), dtype=torch.int32, device=img.device)
    p = img.data_ptr()
    flags = (1 if bins_major else 0) | (2 if two_pass else 0) | (4 if tile_sweep else 0) | (int(route) << 4)
    ctx.check(ctx._lib.cfear_filter_kstrongest_rowkeys(ctx.h, p, C.byref(d), C.byref(par), flags, _ptr(keys)[0], _ptr(cnt)[0]))
    return keys, cnt


def filter_cacfar(img, window_size, nb_guard_cells, false_alarm_rate, range_res, z_min, min_distance,
                  max_distance=400.0, cap_points=None, want_mask=False, ctx=None):
    """AzimuthCACFAR::getFilteredPointCloud (cfar.cpp:35-71).  Returns dict(xyzi, n_points[, det_mask]).  A torch CUDA view
    with a row pitch or a batch stride is used in place."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    cap = int(cap_points or rows * cols)
    par = L.CacfarParams(int(window_size), int(nb_guard_cells), float(false_alarm_rate), float(range_res),
                         float(z_min), float(min_distance), float(max_distance))
    if _is_torch(img):
        import torch
        assert img.dtype == torch.uint8 and img.stride(-1) == 1
        d.stride = img.stride(-2)
        d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
        xyzi = torch.empty((batch, cap, 4), dtype=torch.float32, device=img.device)
        npts = torch.empty((batch,), dtype=torch.int32, device=img.device)
        mask = torch.empty((batch, rows, cols), dtype=torch.uint8, device=img.device) if want_mask else None
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        xyzi = np.empty((batch, cap, 4), np.float32)
        npts = np.empty((batch,), np.int32)
        mask = np.empty((batch, rows, cols), np.uint8) if want_mask else None
    ctx.check(ctx._lib.cfear_filter_cacfar(ctx.h, img.data_ptr() if _is_torch(img) else _ptr(img)[0], C.byref(d), C.byref(par), _ptr(xyzi)[0],
                                           _ptr(npts)[0], cap, _ptr(mask)[0]))
    res = dict(xyzi=xyzi, n_points=npts)
    if want_mask:
        res["det_mask"] = mask
    return res


def cacfar_plan(rows, cols, window_size, nb_guard_cells, false_alarm_rate, range_res, z_min, min_distance, max_distance=400.0,
                keys=False, bins_major=False, stride=None, batch=1, batch_stride=None, base=0):
    """cfear_cacfar_plan: which CA-CFAR kernel instantiation a call launches and with which geometry, as a dict of the
    struct's fields (include/cfear_hip.h).  Host code only: needs no GPU and no context.  rows, cols (, stride, batch,
    batch_stride): the images as the filter call gets them (bins_major: [range bins][azimuths]); keys: the key output
    (filter_cacfar_rowkeys, the batched odometry) instead of the bitmap of filter_cacfar; base: the image address."""
    d = L.PolarDesc()
    d.rows, d.cols, d.batch = int(rows), int(cols), int(batch)
    d.stride = int(cols if stride is None else stride)
    d.batch_stride = int(d.rows * d.stride if batch_stride is None else batch_stride)
    par = L.CacfarParams(int(window_size), int(nb_guard_cells), float(false_alarm_rate), float(range_res),
                         float(z_min), float(min_distance), float(max_distance))
    flags = (L.ROWKEYS_BINS_MAJOR if bins_major else 0) | (L.CACFAR_PLAN_KEYS if keys else 0) | ((int(base) & 15) << 12)
    out = L.CacfarPlan()
    rc = L.lib().cfear_cacfar_plan(C.byref(d), C.byref(par), flags, C.byref(out))
    if rc != 0:
        raise L.CfearError(rc, "cfear_cacfar_plan: bad descriptor or parameters")
    return {name: int(getattr(out, name)) for name, _ in L.CacfarPlan._fields_}


def kstrong_plan(rows, cols, k, z_min, range_res=0.0438, min_distance=2.5, stride=None, batch=1, batch_stride=None, base=0):
    """cfear_kstrong_plan: which kstrongest_rows_kernel<NCHUNK, VEC, MASK> a call launches, as a dict of the struct's fields
    (include/cfear_hip.h) with "refused" None or the reason the filter call refuses the arguments.  Host code only: needs no
    GPU and no context.  rows, cols (, stride, batch, batch_stride): the images as the row sweep gets them; base: the address
    of the first image (or that address modulo 16)."""
    d = L.PolarDesc()
    d.rows, d.cols, d.batch = int(rows), int(cols), int(batch)
    d.stride = int(cols if stride is None else stride)
    d.batch_stride = int(d.rows * d.stride if batch_stride is None else batch_stride)
    par = L.KStrongParams(int(k), float(z_min), float(range_res), float(min_distance), 0)
    out = L.KStrongPlan()
    rc = L.lib().cfear_kstrong_plan(C.byref(d), C.byref(par), int(base) & 0xFFFFFFFFFFFFFFFF, C.byref(out))
    if rc != 0:
        raise L.CfearError(rc, "cfear_kstrong_plan: null argument")
    res = {name: int(getattr(out, name)) for name, _ in L.KStrongPlan._fields_ if name != "pad"}
    res["refused"] = L.KSTRONG_REFUSED[res["refused"]]
    return res


def filter_cacfar_rowkeys(img, window_size, nb_guard_cells, false_alarm_rate, range_res, z_min, min_distance,
                          max_distance=400.0, kcap=1024, bins_major=False, ctx=None):
    """cfear_filter_cacfar_rowkeys: the batched odometry's CA-CFAR stage on its own, for a torch CUDA uint8 image
    [rows, cols] or batch [b, rows, cols] (a view with a row pitch / batch stride is used in place); bins_major: the
    images are [range bins][azimuths] and are decoded by the filter itself.
    Returns (row_keys uint32-as-int32 [b, azimuths, kcap] (intensity << 24 | bin, ascending bins; zero beyond a row's
    min(count, kcap)), row_counts int32 [b, azimuths, 2] ({detections, 0})) as CUDA tensors."""
    import torch
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    assert img.dtype == torch.uint8 and img.stride(-1) == 1
    d.stride = img.stride(-2)
    d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
    az = cols if bins_major else rows
    par = L.CacfarParams(int(window_size), int(nb_guard_cells), float(false_alarm_rate), float(range_res),
                         float(z_min), float(min_distance), float(max_distance))
    keys = torch.zeros((batch, az, int(kcap)), dtype=torch.int32, device=img.device)
    cnt = torch.zeros((batch, az, 2), dtype=torch.int32, device=img.device)
    ctx.check(ctx._lib.cfear_filter_cacfar_rowkeys(ctx.h, img.data_ptr(), C.byref(d), C.byref(par), 1 if bins_major else 0,
                                                   _ptr(keys)[0], _ptr(cnt)[0], int(kcap)))
    return keys, cnt


def cen2018_params(**kw):
    """cfear_cen2018_params with the reference's settings (zq 3.0, sigma_gauss 17, min_range_bins 2, range_res 0.04328),
    overridden by keyword."""
    p = L.Cen2018Params()
    L.lib().cfear_cen2018_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in ("zq", "sigma_gauss", "min_range_bins", "range_res"):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def filter_cen2018(img, zq=3.0, sigma_gauss=17, min_range_bins=2, range_res=0.04328, cap_points=None, want_targets=False,
                   want_mask=False, want_stats=False, ctx=None):
    """Cen2018Radar's detector (cen2018features, Utils.cpp:348-434, and the cloud loop of ScanType.cpp:68-88) for a uint8
    image [rows, cols] or a batch [b, rows, cols] (NumPy -> NumPy results, torch CUDA tensor -> torch CUDA results; a torch
    view with a row pitch or a batch stride is used in place).  Returns dict(xyzi [b, cap, 4], n_points [b][, targets
    [b, cap, 2] (azimuth, bin)][, det_mask [b, rows, cols]][, row_stats [b, rows, 2] (mean, sigma)])."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    cap = int(cap_points or rows * ((cols + 1) // 2))      # a row of n bins holds at most ceil(n / 2) runs
    par = cen2018_params(zq=float(zq), sigma_gauss=int(sigma_gauss), min_range_bins=int(min_range_bins), range_res=float(range_res))
    if _is_torch(img):
        import torch
        assert img.dtype == torch.uint8 and img.stride(-1) == 1
        d.stride = img.stride(-2)
        d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=img.device)
        i32, u8, f32 = torch.int32, torch.uint8, torch.float32
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        mk = lambda shape, dt: np.empty(shape, dt)
        i32, u8, f32 = np.int32, np.uint8, np.float32
    res = dict(xyzi=mk((batch, cap, 4), f32), n_points=mk((batch,), i32))
    if want_targets:
        res["targets"] = mk((batch, cap, 2), i32)
    if want_mask:
        res["det_mask"] = mk((batch, rows, cols), u8)
    if want_stats:
        res["row_stats"] = mk((batch, rows, 2), f32)
    p = img.data_ptr() if _is_torch(img) else _ptr(img)[0]
    ctx.check(ctx._lib.cfear_filter_cen2018(ctx.h, p, C.byref(d), C.byref(par), _ptr(res["xyzi"])[0], _ptr(res["n_points"])[0],
                                            cap, _ptr(res.get("targets"))[0], _ptr(res.get("det_mask"))[0],
                                            _ptr(res.get("row_stats"))[0]))
    return res


def cen2019_params(**kw):
    """cfear_cen2019_params with the reference's settings (max_points 1000, min_range_bins 0, range_res 0.04328), overridden
    by keyword."""
    p = L.Cen2019Params()
    L.lib().cfear_cen2019_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in ("max_points", "min_range_bins", "range_res"):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def filter_cen2019(img, max_points=1000, min_range_bins=0, range_res=0.04328, cap_points=None, want_targets=False,
                   want_mask=False, want_stats=False, want_counts=False, ctx=None):
    """The Cen2019 detector (cen2019features, Utils.cpp:436-594; the cloud as Cen2018Radar's, ScanType.cpp:68-88) for a uint8
    image [rows, cols] or a batch [b, rows, cols] (NumPy -> NumPy results, torch CUDA tensor -> torch CUDA results; a torch
    view with a row pitch or a batch stride is used in place).  Returns dict(xyzi [b, cap, 4], n_points [b][, targets
    [b, cap, 2] (azimuth, bin)][, region_mask [b, rows, cols]][, image_stats [b, 4] (mean, max g, mean_h, h of the last
    candidate gone through)][, counts [b, 3] (candidates, fresh, gone through)])."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    cap = int(cap_points or rows * ((cols + 1) // 2))      # a row of n bins holds at most ceil(n / 2) runs
    par = cen2019_params(max_points=int(max_points), min_range_bins=int(min_range_bins), range_res=float(range_res))
    if _is_torch(img):
        import torch
        assert img.dtype == torch.uint8 and img.stride(-1) == 1
        d.stride = img.stride(-2)
        d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=img.device)
        i32, u8, f32 = torch.int32, torch.uint8, torch.float32
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        mk = lambda shape, dt: np.empty(shape, dt)
        i32, u8, f32 = np.int32, np.uint8, np.float32
    res = dict(xyzi=mk((batch, cap, 4), f32), n_points=mk((batch,), i32))
    if want_targets:
        res["targets"] = mk((batch, cap, 2), i32)
    if want_mask:
        res["region_mask"] = mk((batch, rows, cols), u8)
    if want_stats:
        res["image_stats"] = mk((batch, 4), f32)
    if want_counts:
        res["counts"] = mk((batch, 3), i32)
    p = img.data_ptr() if _is_torch(img) else _ptr(img)[0]
    ctx.check(ctx._lib.cfear_filter_cen2019(ctx.h, p, C.byref(d), C.byref(par), _ptr(res["xyzi"])[0], _ptr(res["n_points"])[0],
                                            cap, _ptr(res.get("targets"))[0], _ptr(res.get("region_mask"))[0],
                                            _ptr(res.get("image_stats"))[0], _ptr(res.get("counts"))[0]))
    return res


def cen2019_order_audit(img, max_points=1000, min_range_bins=0, cap_points=None, want_targets=False, want_marks=False, ctx=None):
    """cfear_cen2019_order_audit: which landmarks of filter_cen2019 hang on the order among equal h that the reference's
    std::sort leaves open, for a uint8 image [rows, cols] or a batch [b, rows, cols] (NumPy, or a torch
    CUDA tensor -- a view with a row pitch or a batch stride is used in place).  Returns dict(records: a
    CEN2019_ORDER_RECORD_DTYPE array [b] (NumPy on either side)[, targets [b, cap, 2] and certain uint8 [b, cap]: the filter's
    targets and whether every order emits each][, marks uint8 [b, rows, cols]: bit 0 R_in, bit 1 R, bit 2 R_out, bit 3 the
    reversed order's R]).  records["n_marks_in"] == records["n_marks_out"]: no order changes that sweep."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    cap = int(cap_points or rows * ((cols + 1) // 2)) if want_targets else 0
    par = cen2019_params(max_points=int(max_points), min_range_bins=int(min_range_bins))
    dev = _is_torch(img)
    if dev:
        import torch
        assert img.dtype == torch.uint8 and img.stride(-1) == 1
        d.stride = img.stride(-2)
        d.batch_stride = img.stride(0) if img.ndim == 3 else rows * d.stride
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=img.device)
        i32, u8 = torch.int32, torch.uint8
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        mk = lambda shape, dt: np.empty(shape, dt)
        i32, u8 = np.int32, np.uint8
    rec = mk((batch, L.CEN2019_ORDER_RECORD_DTYPE.itemsize), u8)
    res = {}
    if want_targets:
        res["targets"] = mk((batch, cap, 2), i32)
        res["certain"] = mk((batch, cap), u8)
    if want_marks:
        res["marks"] = mk((batch, rows, cols), u8)
    _torch_ready(ctx, img, rec, *res.values())
    p = img.data_ptr() if dev else _ptr(img)[0]
    rc = ctx._lib.cfear_cen2019_order_audit(ctx.h, p, C.byref(d), C.byref(par), _ptr(rec)[0], _ptr(res.get("targets"))[0],
                                            _ptr(res.get("certain"))[0], cap, _ptr(res.get("marks"))[0])
    ctx.check(rc)
    res["records"] = (rec.cpu().numpy() if dev else rec).view(L.CEN2019_ORDER_RECORD_DTYPE).reshape(batch)
    return res


def k_strongest_filter(img, k_strongest, z_min, range_res, min_distance, ctx=None):
    """The legacy k_strongest_filter / InsertStrongestK (radar_filters.cpp:25-78; CorAl's kstrongRadar).  img: uint8
    [rows, cols] or [batch, rows, cols] (NumPy or torch CUDA).  Returns dict(xyzi [batch, rows * k, 4], n_points)."""
    ctx = ctx or default_context()
    d, batch, rows, cols = _desc(img)
    cap = rows * int(k_strongest)
    if _is_torch(img):
        import torch
        xyzi = torch.empty((batch, cap, 4), dtype=torch.float32, device=img.device)
        npts = torch.empty((batch,), dtype=torch.int32, device=img.device)
    else:
        img = np.ascontiguousarray(img, dtype=np.uint8)
        xyzi = np.empty((batch, cap, 4), np.float32)
        npts = np.empty((batch,), np.int32)
    ctx.check(ctx._lib.cfear_filter_kstrongest_legacy(ctx.h, _ptr(img)[0], C.byref(d), int(k_strongest), float(z_min), float(range_res),
                                                      float(min_distance), _ptr(xyzi)[0], _ptr(npts)[0], cap))
    return dict(xyzi=xyzi, n_points=npts)


class radarDriver:
    """radarDriver (radar_driver.cpp): CallbackOffline(image) -> (cloud, cloud_peaks)."""

    def __init__(self, pars=None, ctx=None):
        self.par = pars or radarDriverParameters()
        self.ctx = ctx or default_context()
        self.cv_polar_image = None

    def CallbackOffline(self, radar_image_polar):
        img = radar_image_polar
        if self.par.dataset != "oxford":
            # Callback (radar_driver.cpp:74-90): MONO8 + rotate 90 deg CCW so rows = azimuth
            img = polar_rotate_ccw(img, self.ctx)
        self.cv_polar_image = img
        p = self.par
        if p.filter_type == "CA-CFAR":                                      # radar_driver.cpp:52-56
            r = filter_cacfar(img, p.window_size, p.nb_guard_cells, p.false_alarm_rate, p.range_res, p.z_min,
                              p.min_distance, 400.0, ctx=self.ctx)
            n = int(r["n_points"][0])
            return r["xyzi"][0, :n], r["xyzi"][0, :0]
        r = filter_kstrongest(img, p.k_strongest, p.z_min, p.range_res, p.min_distance, True, ctx=self.ctx)
        n, m = int(r["n_points"][0]), int(r["n_peaks"][0])
        return r["xyzi"][0, :n], r["xyzi_peaks"][0, :m]


# ------------------------------------------------------------------------------------------------
# Compensate / MapPointNormal
# ------------------------------------------------------------------------------------------------
def Compensate(cloud, mot, ccw, ctx=None):
    """Compensate(cloud, mot, ccw) (utils.cpp:96-107): in place on `cloud` (float32 [n,4])."""
    ctx = ctx or default_context()
    m = (C.c_double * 3)(*[float(v) for v in mot])
    ctx.check(ctx._lib.cfear_compensate(ctx.h, _ptr(cloud)[0], int(cloud.shape[0]), m, int(bool(ccw))))
    return cloud


class MapPointNormal:
    """MapPointNormal (pointnormal.h:110): device-resident oriented surface points of one scan."""

    downsample_factor = 1.0      # static member, pointnormal.cpp:5

    def __init__(self, cld=None, radius=3.0, origin=(0.0, 0.0), weight_intensity=False, raw=False, ctx=None,
                 cells=None, compensate=None, ccw=False):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        lib = self.ctx._lib
        if cells is not None:
            cells = np.ascontiguousarray(cells, dtype=L.CELL_DTYPE)
            self.ctx.check(lib.cfear_scan_from_cells(self.ctx.h, cells.ctypes.data, int(cells.shape[0]), C.byref(self._h)))
            return
        if raw:
            # GetIdentityCell per point (pointnormal.cpp:76-82, pointnormal.h:56,78-80)
            pts = np.asarray(cld if not _is_torch(cld) else cld.cpu().numpy())
            c = np.zeros(pts.shape[0], L.CELL_DTYPE)
            c["mean"] = pts[:, :2]
            c["normal"] = (1.0, 0.0)
            c["cov"] = (0.1, 0.0, 0.0, 0.1)
            c["scale"], c["avg_intensity"], c["lambda_min"], c["lambda_max"], c["nsamples"] = 1.0, 1.0, 1.0, 1.0, 1
            self.ctx.check(lib.cfear_scan_from_cells(self.ctx.h, c.ctypes.data, int(c.shape[0]), C.byref(self._h)))
            return
        fp = L.FeatureParams()
        fp.radius = float(radius)
        fp.downsample_factor = float(MapPointNormal.downsample_factor)
        fp.origin[0], fp.origin[1] = float(origin[0]), float(origin[1])
        fp.weight_intensity = int(bool(weight_intensity))
        fp.compensate = int(compensate is not None)
        if compensate is not None:
            fp.mot[0], fp.mot[1], fp.mot[2] = [float(v) for v in compensate]
        fp.ccw = int(bool(ccw))
        n = int(cld.shape[0])
        self.ctx.check(lib.cfear_scan_create(self.ctx.h, _ptr(cld)[0], n, C.byref(fp), C.byref(self._h)))

    @classmethod
    def _from_handle(cls, h, ctx):
        """Wraps a cfear_scan* the library handed out (cfear_odometry_get_scan); the wrapper owns it."""
        m = cls.__new__(cls)
        m.ctx, m._h = ctx, h
        return m

    def GetSize(self):
        return self.ctx._lib.cfear_scan_size(self._h)

    @property
    def path(self):
        """The route the surface-point kernels served this scan on (L.SURF_PATH_*; 0 for a map made from cells)."""
        p = C.c_uint32()
        self.ctx.check(self.ctx._lib.cfear_scan_surface_path(self._h, C.byref(p)))
        return int(p.value)

    def GetClosestIdx(self, p, d):
        """GetClosestIdx(p, d) (pointnormal.cpp:238-254): [index of the nearest cell mean] or [] beyond d.
        p may also be an array [n, 2] of points (NumPy or torch CUDA float64): -> int32 [n], -1 where none."""
        single = not _is_torch(p) and np.ndim(p) == 1
        q = p if _is_torch(p) else np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
        n = int(q.shape[0])
        if _is_torch(q):
            import torch
            q = q.contiguous()
            out = torch.empty(n, dtype=torch.int32, device=q.device)
        else:
            out = np.empty(n, np.int32)
        self.ctx.check(self.ctx._lib.cfear_scan_closest_idx(self._h, _ptr(q)[0], n, float(d), _ptr(out)[0]))
        if single:
            return [int(out[0])] if out[0] >= 0 else []
        return out

    def GetClosestTies(self, p, d):
        """The tie-aware GetClosestIdx (cfear_scan_closest_ties): ALL cells at the minimum float distance of p, which FLANN's
        1-NN search returns one of.  -> (lo, hi, count): lo is GetClosestIdx's answer (the lowest index), hi the highest
        cell at the same distance, count how many there are; (-1, -1, 0) beyond d.  p: one point or an array [n, 2]
        (NumPy or torch CUDA float64) -> ints or int32 [n] arrays."""
        single = not _is_torch(p) and np.ndim(p) == 1
        q = p if _is_torch(p) else np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
        n = int(q.shape[0])
        if _is_torch(q):
            import torch
            q = q.contiguous()
            lo, hi, cnt = (torch.empty(n, dtype=torch.int32, device=q.device) for _ in range(3))
        else:
            lo, hi, cnt = (np.empty(n, np.int32) for _ in range(3))
        self.ctx.check(self.ctx._lib.cfear_scan_closest_ties(self._h, _ptr(q)[0], n, float(d), _ptr(lo)[0], _ptr(hi)[0], _ptr(cnt)[0]))
        if single:
            return int(lo[0]), int(hi[0]), int(cnt[0])
        return lo, hi, cnt

    def GetCells(self):
        n = self.GetSize()
        out = np.zeros(max(n, 1), L.CELL_DTYPE)
        rc = self.ctx._lib.cfear_scan_get_cells(self._h, out.ctypes.data, out.shape[0])
        if rc < 0:
            self.ctx.check(rc)
        return out[:n]

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_batch", None) is not None:  # borrowed from a ScanBatch: the batch owns the cells
                self._batch = None
            elif getattr(self.ctx, "h", None):            # the context may already be gone at interpreter exit: its
                self.ctx._lib.cfear_scan_destroy(self._h)   # objects died with it, destroying them again would be a use after free
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScanBatch:
    """cfear_scan_batch: N scans in one arena, made by one call (scan_create_batch).  batch[i] is a MapPointNormal that
    BORROWS scan i -- usable wherever a MapPointNormal is (Register*, ScanTable, GetCells, GetClosestIdx, path, the audits)
    and keeping the batch alive -- or None where the scan failed; batch.status is the int32 [n] array of per-scan statuses
    (L.OK, L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY)."""

    def __init__(self, h, status, ctx):
        self.ctx, self._h, self.status = ctx, h, status
        self._scans = []
        for i in range(int(ctx._lib.cfear_scan_batch_size(h))):
            s = C.c_void_p()
            ctx.check(ctx._lib.cfear_scan_batch_get(h, i, C.byref(s)))
            m = None
            if s.value:
                m = MapPointNormal._from_handle(s, ctx)
                m._batch = self
            self._scans.append(m)

    def __len__(self):
        return len(self._scans)

    def __getitem__(self, i):
        return self._scans[i]

    def __iter__(self):
        return iter(self._scans)

    def close(self):
        """Destroys the batch; the MapPointNormals it handed out must not be used afterwards."""
        if getattr(self, "_h", None):
            for m in self._scans:
                if m is not None:
                    m._h, m._batch = None, None
            if getattr(self.ctx, "h", None):
                self.ctx._lib.cfear_scan_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scan_create_batch(clouds, radius=3.0, origin=(0.0, 0.0), weight_intensity=False, compensate=None, ccw=False, max_cells=None,
                      downsample_factor=None, ctx=None):
    """cfear_scan_create_batch: one MapPointNormal per cloud in one call -> a ScanBatch.  clouds: a list of [n, 4] float32
    arrays, all NumPy or all torch CUDA tensors (they are concatenated), or a tuple (xyzi [total, 4], offsets, lengths) that
    is used in place.  compensate: None, or the [N, 3] motions the clouds are compensated by (in a copy: the clouds stay as
    they are).  max_cells: the cells a scan may hold (default: the longest cloud's points, at most 16 384).  A cloud that is
    empty or exceeds max_cells gives None in the batch and its status in batch.status; nothing is raised for it."""
    ctx = ctx or default_context()
    if isinstance(clouds, tuple):
        xyzi, offsets, lengths = clouds
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    else:
        clouds = list(clouds)
        lengths = np.array([int(c.shape[0]) for c in clouds], np.int32)
        offsets = (np.cumsum(lengths, dtype=np.int64) - lengths).astype(np.int64)
        if clouds and _is_torch(clouds[0]):
            import torch
            xyzi = torch.cat([c.reshape(-1, 4) for c in clouds]).float().contiguous()
        else:
            xyzi = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 4) for c in clouds]) if clouds
                                        else np.zeros((0, 4), np.float32))
    n = int(lengths.shape[0])
    if not _is_torch(xyzi):
        xyzi = np.ascontiguousarray(xyzi, dtype=np.float32)
    fp = L.FeatureParams()
    fp.radius = float(radius)
    fp.downsample_factor = float(MapPointNormal.downsample_factor if downsample_factor is None else downsample_factor)
    fp.origin[0], fp.origin[1] = float(origin[0]), float(origin[1])
    fp.weight_intensity = int(bool(weight_intensity))
    fp.compensate = int(compensate is not None)
    fp.ccw = int(bool(ccw))
    mots = None if compensate is None else np.ascontiguousarray(compensate, dtype=np.float64).reshape(n, 3)
    if max_cells is None:
        max_cells = max(1, min(16384, int(lengths.max()) if n else 1))
    status = np.zeros(n, np.int32)
    h = C.c_void_p()
    _torch_ready(ctx, xyzi)
    rc = ctx._lib.cfear_scan_create_batch(ctx.h, _ptr(xyzi)[0] if xyzi.shape[0] else None, offsets.ctypes.data, lengths.ctypes.data, n,
                                          C.byref(fp), None if mots is None else mots.ctypes.data, int(max_cells), C.byref(h),
                                          status.ctypes.data)
    if not h.value:
        ctx.check(rc)
    return ScanBatch(h, status, ctx)


# ------------------------------------------------------------------------------------------------
# n_scan_normal_reg
# ------------------------------------------------------------------------------------------------
class ScanTable:
    """The device views of a set of scans, uploaded once (cfear_scan_table_create): what a loop-closure thread keeps for the
    graph nodes' cloud_normal_ (types.h:119-122) so that a candidate is two indices and two poses."""

    def __init__(self, scans, ctx=None):
        self.ctx = ctx or scans[0].ctx
        self._scans = list(scans)                                  # (the table holds its own reference on every scan too)
        hs = (C.c_void_p * len(scans))(*[s._h for s in scans])
        self._h = C.c_void_p()
        self.ctx.check(self.ctx._lib.cfear_scan_table_create(self.ctx.h, hs, len(scans), C.byref(self._h)))

    def __len__(self):
        return int(self.ctx._lib.cfear_scan_table_size(self._h))

    @staticmethod
    def candidates(targets, sources, source_xyt, target_xyt=None):
        """CANDIDATE_DTYPE array from index arrays and [n][3] poses (target pose: the origin unless given)."""
        n = len(targets)
        c = np.zeros(n, L.CANDIDATE_DTYPE)
        c["target"], c["source"] = targets, sources
        c["source_xyt"] = np.asarray(source_xyt, dtype=np.float64).reshape(n, 3)
        if target_xyt is not None:
            c["target_xyt"] = np.asarray(target_xyt, dtype=np.float64).reshape(n, 3)
        return c

    def close(self):
        if self._h:
            self.ctx._lib.cfear_scan_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RcclComm:
    """cfear_rccl_comm made by the library itself (cfear_rccl_unique_id / cfear_rccl_comm_init): `exchange(b)` hands rank 0's
    128-byte id to every rank -- any broadcast will do (bench.py uses torch.distributed); world 1 needs none."""

    def __init__(self, ctx, world=1, rank=0, exchange=None):
        self.ctx = ctx
        lib = ctx._lib
        uid = C.create_string_buffer(128)
        if rank == 0:
            rc = lib.cfear_rccl_unique_id(uid)
            if rc != L.OK:
                raise L.CfearError(rc, "librccl.so / ncclGetUniqueId not available")
        if world > 1:
            raw = exchange(bytes(uid.raw))
            assert len(raw) == 128
            uid = C.create_string_buffer(raw, 128)
        self.c = L.RcclComm()
        ctx.check(lib.cfear_rccl_comm_init(ctx.h, uid, int(world), int(rank), C.byref(self.c)))
        self.world, self.rank = int(world), int(rank)

    def close(self):
        if getattr(self, "c", None) is not None and self.c.nccl_comm:
            self.ctx._lib.cfear_rccl_comm_destroy(C.byref(self.c))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CandidatePipe:
    """cfear_candidate_pipe: up to `depth` sharded candidate steps in flight (submit never waits, collect waits on one event);
    every rank hands in the FULL candidate list and gets all n records back in candidate order."""

    def __init__(self, reg, table, max_candidates, comm=None, rank=0, world=1, depth=2, graph=False, timing=False):
        self.reg, self.table, self.ctx, self.comm = reg, table, reg.ctx, comm
        self._h = C.c_void_p()
        self.ctx.check(self.ctx._lib.cfear_candidate_pipe_create(self.ctx.h, table._h, int(max_candidates), int(rank), int(world),
                                                                 C.byref(comm.c) if comm is not None else None, int(depth),
                                                                 (L.PIPE_GRAPH if graph else 0) | (L.PIPE_TIMING if timing else 0),
                                                                 C.byref(self._h)))
        self.depth = int(depth)

    def stats(self):
        """{exchange_ms: all_gather + read-back summed over the collected steps (timing=True), steps, graph_slots}"""
        ms, n, g = C.c_double(), C.c_int64(), C.c_int32()
        self.ctx.check(self.ctx._lib.cfear_candidate_pipe_stats(self._h, C.byref(ms), C.byref(n), C.byref(g)))
        return {"exchange_ms": float(ms.value), "steps": int(n.value), "graph_slots": int(g.value)}

    def submit(self, cands):
        cands = np.ascontiguousarray(cands, dtype=L.CANDIDATE_DTYPE)
        t = C.c_int64()
        self.ctx.check(self.ctx._lib.cfear_candidate_pipe_submit(self._h, C.c_void_p(cands.ctypes.data), cands.shape[0],
                                                                 C.byref(self.reg.par), C.byref(t)))
        return (int(t.value), cands.shape[0])

    def collect(self, ticket, out=None):
        t, n = ticket
        out = np.empty(n, L.RESULT_DTYPE) if out is None else out
        self.ctx.check(self.ctx._lib.cfear_candidate_pipe_collect(self._h, t, C.c_void_p(out.ctypes.data)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.ctx._lib.cfear_candidate_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class n_scan_normal_reg:
    """n_scan_normal_reg(cost, loss=Huber, loss_limit=0.1, opt=Uniform) (n_scan_normal.h:35)."""

    def __init__(self, cost="P2L", loss="Huber", loss_limit=0.1, opt=0, ctx=None):
        self.ctx = ctx or default_context()
        self.par = L.RegParams()
        self.ctx._lib.cfear_reg_params_default(C.byref(self.par))
        self.par.cost = L.COST[cost] if isinstance(cost, str) else int(cost)
        self.par.loss = L.LOSS[loss] if isinstance(loss, str) else int(loss)
        self.par.loss_limit = float(loss_limit)
        self.par.weight_opt = int(opt)
        self.summary_ = None
        self.score_ = 0.0

    def SetParameters(self, max_itr_association, max_itr_solver):          # n_scan_normal.cpp:15-19
        self.par.max_itr_association = int(max_itr_association)
        self.par.max_itr_solver = int(max_itr_solver)

    def SetD2dPar(self, cov_scale, regularization):                        # n_scan_normal.h:59
        self.par.cov_scale, self.par.regularization = float(cov_scale), float(regularization)

    def _handles(self, scans):
        return (C.c_void_p * len(scans))(*[s._h for s in scans])

    def Register(self, scans, Tsrc):
        """Register(scans, Tsrc, reg_cov) (n_scan_normal.cpp:82-185): Tsrc float64 [n,3] (x,y,theta);
        returns (success, Tsrc_out, reg_cov) with reg_cov the reference's constant diagonal."""
        p = np.ascontiguousarray(Tsrc, dtype=np.float64).copy()
        res = L.RegResult()
        rc = self.ctx._lib.cfear_register(self.ctx.h, self._handles(scans), len(scans),
                                          p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self.par), C.byref(res))
        self.ctx.check(rc, allowed=(L.ERR_TOO_FEW_RESIDUALS, L.ERR_SOLVER))
        self.summary_ = res
        self.score_ = res.score
        self.par.itr = res.outer_iters                                     # itr_ is left behind for GetCost
        cov = np.diag([0.1 * 0.1, 0.1 * 0.1, 0, 0, 0, 0.01 * 0.01])        # n_scan_normal.cpp:171-175
        return rc == L.OK, p, cov

    def PrepareBatch(self, jobs):
        """Marshals a list of (scans, Tsrc) once; the result can be passed to RegisterBatch repeatedly."""
        n = len(jobs)
        arr = (L.RegJob * n)()
        keep = []
        for i, (scans, T) in enumerate(jobs):
            hs = self._handles(scans)
            p = np.ascontiguousarray(T, dtype=np.float64)
            keep.append((hs, p, scans))
            arr[i].scans = C.cast(hs, C.POINTER(C.c_void_p))
            arr[i].n_scans = len(scans)
            arr[i].poses_xyt = p.ctypes.data_as(C.POINTER(C.c_double))
        return (arr, n, keep)

    def RegisterBatch(self, jobs):
        """jobs: list of (scans, Tsrc) or a PrepareBatch result.  One launch; returns a RESULT_DTYPE array
        (loop-closure candidate batches, tbv_slam/src/tbv_slam/loopclosure.cpp:35-97 per candidate)."""
        arr, n, _keep = jobs if isinstance(jobs, tuple) else self.PrepareBatch(jobs)
        out = np.zeros(n, L.RESULT_DTYPE)
        if n:
            self.ctx.check(self.ctx._lib.cfear_register_batch(self.ctx.h, arr, n, C.byref(self.par), out.ctypes.data))
        return out

    def RegisterBatchInto(self, jobs, device_ptr):
        """As RegisterBatch, but the records stay on the GPU: device_ptr = a device buffer of n * 72 bytes; the launch is
        enqueued on the context's stream and NOT synchronised (cfear_register_batch with a device pointer for results).
        Returns n."""
        arr, n, _keep = jobs if isinstance(jobs, tuple) else self.PrepareBatch(jobs)
        if n:
            self.ctx.check(self.ctx._lib.cfear_register_batch(self.ctx.h, arr, n, C.byref(self.par), C.c_void_p(int(device_ptr))))
        return n

    def RegisterCandidates(self, table, cands, device_ptr=None):
        """Candidate pairs among the scans of a ScanTable (cfear_register_candidates): cands = a CANDIDATE_DTYPE array
        (ScanTable.candidates builds one) -- 56 bytes per candidate cross PCIe instead of a marshalled job record.  Returns a
        RESULT_DTYPE array, or, with device_ptr (a device buffer of n * 72 bytes), leaves the records there without
        synchronising and returns n."""
        cands = np.ascontiguousarray(cands, dtype=L.CANDIDATE_DTYPE)
        n = cands.shape[0]
        out = None if device_ptr is not None else np.zeros(n, L.RESULT_DTYPE)
        if n:
            dst = C.c_void_p(int(device_ptr)) if device_ptr is not None else C.c_void_p(out.ctypes.data)
            self.ctx.check(self.ctx._lib.cfear_register_candidates(self.ctx.h, table._h, C.c_void_p(cands.ctypes.data), n,
                                                                   C.byref(self.par), dst))
        return n if device_ptr is not None else out

    def GetCost(self, scans, Tsrc):
        """GetCost (n_scan_normal.cpp:186-211) -> (success, score(cost), residuals)."""
        p = np.ascontiguousarray(Tsrc, dtype=np.float64)
        cap = 2 * sum(s.GetSize() for s in scans) + 2
        r = np.empty(cap, np.float64)
        cost, score, nres = C.c_double(), C.c_double(), C.c_int32()
        rc = self.ctx._lib.cfear_get_cost(self.ctx.h, self._handles(scans), len(scans),
                                          p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self.par), C.byref(cost),
                                          r.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(nres), C.byref(score))
        self.ctx.check(rc, allowed=(L.ERR_TOO_FEW_RESIDUALS,))
        self.score_ = score.value
        return rc == L.OK, cost.value, r[:nres.value].copy()

    def getScore(self):
        return self.score_

    def GetCostBatch(self, jobs):
        """GetCost for a list of (scans, Tsrc) in one launch -> RESULT_DTYPE array (final_cost = robust cost,
        score, num_residuals, status).  The radius follows self.par.itr like GetCost."""
        arr, n, _keep = jobs if isinstance(jobs, tuple) else self.PrepareBatch(jobs)
        out = np.zeros(n, L.RESULT_DTYPE)
        if n:
            self.ctx.check(self.ctx._lib.cfear_get_cost_batch(self.ctx.h, arr, n, C.byref(self.par), out.ctypes.data))
        return out

    def GetCovarianceScaler(self):
        """GetCovarianceScaler (n_scan_normal.cpp:433-439) of the last Register -> (ok, scale)."""
        r = self.summary_
        if r is None or r.num_residuals - 3 == 0:
            return False, 1.0
        return True, r.final_cost / (r.num_residuals - 3)

    @staticmethod
    def sampling_params(xy_range=0.4, yaw_range=0.0043625, samples_per_axis=3, covariance_scaler=4.0):
        """OdometryKeyframeFuser::Parameters cov_sampling_* (odometrykeyframefuser.h:107-110); the loop-closure
        copy uses xy_range=0.4, yaw_range=0.0044 (loopclosure.cpp:108-112)."""
        sp = L.CovSamplingParams()
        sp.xy_range, sp.yaw_range = float(xy_range), float(yaw_range)
        sp.samples_per_axis, sp.covariance_scaler = int(samples_per_axis), float(covariance_scaler)
        return sp

    def approximateCovarianceBySampling(self, scans, T_vek, reg_result=None, sampling=None, want_samples=False):
        """OdometryKeyframeFuser::approximateCovarianceBySampling (odometrykeyframefuser.cpp:261-380) /
        loopclosure::approximateCovarianceBySampling (loopclosure.cpp:99-208).  T_vek: poses after Register;
        reg_result: that Register's summary (defaults to this object's last one).
        Returns (success, cov 6x6[, samples [n^3,4]])."""
        res = reg_result if reg_result is not None else self.summary_
        if res is None:
            raise ValueError("approximateCovarianceBySampling needs the result of a Register call")
        if not isinstance(res, L.RegResult):
            r = L.RegResult()
            for k in ("score", "final_cost", "num_residuals", "outer_iters", "lm_iters", "status"):
                setattr(r, k, res[k].item() if hasattr(res[k], "item") else res[k])
            res = r
        sp = sampling or self.sampling_params()
        p = np.ascontiguousarray(T_vek, dtype=np.float64)
        cov = np.zeros((6, 6), np.float64)
        m = sp.samples_per_axis ** 3
        smp = np.zeros((m, 4), np.float64)
        ok = C.c_int32()
        rc = self.ctx._lib.cfear_covariance_by_sampling(
            self.ctx.h, self._handles(scans), len(scans), p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self.par),
            C.byref(res), C.byref(sp), cov.ctypes.data_as(C.POINTER(C.c_double)),
            smp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ok))
        self.ctx.check(rc)
        return (bool(ok.value), cov, smp) if want_samples else (bool(ok.value), cov)

    def approximateCovarianceBySamplingBatch(self, jobs, reg_results, sampling=None):
        """Batch form: jobs as for RegisterBatch (poses AFTER registration), reg_results the RESULT_DTYPE array
        RegisterBatch returned.  -> (success [n] bool, cov [n,6,6])."""
        arr, n, _keep = jobs if isinstance(jobs, tuple) else self.PrepareBatch(jobs)
        sp = sampling or self.sampling_params()
        regs = np.ascontiguousarray(reg_results, dtype=L.RESULT_DTYPE)
        cov = np.zeros((n, 6, 6), np.float64)
        ok = np.zeros(n, np.int32)
        if n:
            self.ctx.check(self.ctx._lib.cfear_covariance_by_sampling_batch(
                self.ctx.h, arr, n, C.byref(self.par), regs.ctypes.data, C.byref(sp), cov.ctypes.data, None,
                ok.ctypes.data))
        return ok.astype(bool), cov


# ------------------------------------------------------------------------------------------------
# Which registrations hang on a nearest-neighbour tie
# ------------------------------------------------------------------------------------------------
def _tie_reg(par, ctx):
    """An n_scan_normal_reg that carries `par`: None (the defaults), a RegParams, or an n_scan_normal_reg."""
    reg = n_scan_normal_reg(ctx=ctx)
    if par is not None:
        reg.par = par.par if isinstance(par, n_scan_normal_reg) else par
    return reg


def association_ties(jobs, par=None, itr=1, want_queries=False, ctx=None, device_out=False):
    """cfear_association_ties_batch: the association step of every job -- a list of (scans, Tsrc) as for RegisterBatch, or
    a PrepareBatch result -- replayed at the poses given, with ALL nearest target cells of every query kept.  itr selects
    the radius as in AddScanPairCost (2 * radius when itr == 1).  One launch for the batch.
    -> a TIE_RECORD_DTYPE array [n]; with want_queries (records, per_query int32 [total, 3] = (lo, hi, count), offsets
    int64 [n + 1]): job j's queries are per_query[offsets[j]:offsets[j + 1]], the entry of fixed scan t and source cell s
    is t * n_src + s, (-1, -1, 0) outside the radius.  With device_out the records (uint8 [n, 32], to view on the host) and
    per_query are torch CUDA tensors and nothing is synchronised."""
    ctx = ctx or default_context()
    reg = _tie_reg(par, ctx)
    arr, n, keep = jobs if isinstance(jobs, tuple) else reg.PrepareBatch(jobs)
    sizes = [int(k[2][-1].GetSize()) * (len(k[2]) - 1) for k in keep]
    offsets = np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
    total = int(offsets[-1])
    if device_out:
        import torch
        rec = torch.zeros((n, L.TIE_RECORD_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        pq = torch.zeros((max(total, 1), 3), dtype=torch.int32, device="cuda") if want_queries else None
        _torch_ready(ctx, rec)
    else:
        rec = np.zeros(n, L.TIE_RECORD_DTYPE)
        pq = np.zeros((max(total, 1), 3), np.int32) if want_queries else None
    if n:
        ctx.check(ctx._lib.cfear_association_ties_batch(ctx.h, arr, n, C.byref(reg.par), int(itr), _ptr(rec)[0], _ptr(pq)[0], total))
    return (rec, pq[:total], offsets) if want_queries else rec


def flip_ties(scan):
    """A MapPointNormal with the cells of `scan` in reverse order.  The matcher takes the lowest index among all minimisers, so
    against the flipped scan every tie is decided the other way -- ties among distinct equidistant cells included; the
    residual blocks keep their order (keyframe, source cell) as long as only TARGETS are flipped.  Through GetCells / cells=:
    not a hot path."""
    return MapPointNormal(cells=scan.GetCells()[::-1].copy(), ctx=scan.ctx)


def tie_sensitivity(jobs, par=None, ctx=None):
    """The legal spread of THESE registrations under the tie rule, as numbers: every job -- (scans, Tsrc) -- is audited at
    its start poses (itr = 1), registered as given, registered again with every target scan flipped (flip_ties), and audited
    at the registered poses (itr = 2).  Four batched calls.
    -> dict of arrays over the jobs: ties_start, ties_end (TIE_RECORD_DTYPE), result, result_flipped (RESULT_DTYPE) and delta
    [n, 3] = |dx|, |dy|, |dtheta| between the two registered poses.  Nothing here says which way FLANN decides: the spread
    is between this library's rule and its opposite."""
    ctx = ctx or default_context()
    reg = _tie_reg(par, ctx)
    jobs = [(list(scans), np.ascontiguousarray(T, dtype=np.float64).reshape(len(scans), 3)) for scans, T in jobs]
    flipped = {}
    for scans, _ in jobs:
        for s in scans[:-1]:
            if id(s) not in flipped:
                flipped[id(s)] = flip_ties(s)
    ties_start = association_ties(jobs, reg, 1, ctx=ctx)
    result = reg.RegisterBatch(jobs)
    result_flipped = reg.RegisterBatch([([flipped[id(s)] for s in scans[:-1]] + [scans[-1]], T) for scans, T in jobs])
    end = []
    for (scans, T), r in zip(jobs, result):
        Te = T.copy()
        Te[-1] = r["pose"]
        end.append((scans, Te))
    ties_end = association_ties(end, reg, 2, ctx=ctx)
    return {"ties_start": ties_start, "ties_end": ties_end, "result": result, "result_flipped": result_flipped,
            "delta": np.abs(result["pose"] - result_flipped["pose"]).reshape(len(jobs), 3)}


# ------------------------------------------------------------------------------------------------
# Which scans hang on the in-voxel summation order of pcl::VoxelGrid
# ------------------------------------------------------------------------------------------------
def voxel_order_audit(clouds, radius=3.0, downsample_factor=1.0, voxels=False, ctx=None, device_out=False):
    """cfear_voxel_order_audit_batch: per scan -- clouds is a list of [n, 4] float32 arrays, all NumPy or all torch CUDA tensors,
    the clouds MapPointNormal would hand to VoxelGrid -- whether a reference build can differ from this library through the
    order in which a voxel's points are summed.  n_voxels_exposed == 0: it cannot; n_voxels_changed_reversed > 0: the
    reversed order does; the truth lies between the two.  One call for the batch.
    -> a VOXEL_AUDIT_RECORD_DTYPE array [n]; with voxels (records, table VOXEL_AUDIT_VOXEL_DTYPE [total], offsets int64
    [n + 1]): scan s's voxels, in ascending key, are table[offsets[s]:offsets[s + 1]].  A scan that is empty, holds a
    coordinate that is not finite or is too large carries its status in its record and has no rows; nothing is raised for
    it.  With device_out the records (uint8 [n, 48]) and the table (uint8 [total, 56]) are torch CUDA tensors."""
    ctx = ctx or default_context()
    clouds = list(clouds)
    n = len(clouds)
    dev = n > 0 and _is_torch(clouds[0])
    lengths = np.array([int(c.shape[0]) for c in clouds], np.int32)
    total = int(lengths.sum())
    if dev:
        import torch
        xyzi = torch.cat([c.reshape(-1, 4).float() for c in clouds]).contiguous() if total else torch.zeros((1, 4), device="cuda")
    else:
        xyzi = np.concatenate([np.asarray(c, np.float32).reshape(-1, 4) for c in clouds] + [np.zeros((1, 4), np.float32)])
    par = L.VoxelAuditParams(float(radius), 0.0, float(downsample_factor))
    cap = max(total, 1)
    if device_out:
        import torch
        rec = torch.zeros((n, L.VOXEL_AUDIT_RECORD_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        tab = torch.zeros((cap, L.VOXEL_AUDIT_VOXEL_DTYPE.itemsize), dtype=torch.uint8, device="cuda") if voxels else None
    else:
        rec = np.zeros(n, L.VOXEL_AUDIT_RECORD_DTYPE)
        tab = np.zeros(cap, L.VOXEL_AUDIT_VOXEL_DTYPE) if voxels else None
    _torch_ready(ctx, xyzi, rec)
    rows = C.c_int64(0)
    rc = ctx._lib.cfear_voxel_order_audit_batch(ctx.h, _ptr(xyzi)[0], None, lengths.ctypes.data, n, C.byref(par), _ptr(rec)[0], _ptr(tab)[0],
                                                cap, C.byref(rows))
    status = (rec.cpu().numpy().view(L.VOXEL_AUDIT_RECORD_DTYPE).reshape(-1) if device_out else rec)["status"]
    if rc != L.OK and not (status == rc).any():            # a refusal of the call, not a scan's own status
        ctx.check(rc)
    if not voxels:
        return rec
    counts = (rec.cpu().numpy().view(L.VOXEL_AUDIT_RECORD_DTYPE).reshape(-1) if device_out else rec)["n_voxels"]
    return rec, tab[:rows.value], np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)


def voxel_order_spread(job, par=None, radius=3.0, origin=(0.0, 0.0), weight_intensity=True, ctx=None):
    """The legal spread of THIS registration under the in-voxel order, as numbers: job = (clouds, Tsrc), the clouds of the
    job's scans ([n, 4] float32, the free source last).  The scans are built from the clouds as given and from the clouds
    reversed -- this library sums a voxel in input order, so the reversed cloud is the opposite order in every voxel -- and
    both jobs are registered in one batch.  Existing calls only.
    -> dict: audit (VOXEL_AUDIT_RECORD_DTYPE, one per cloud), result, result_reversed (RESULT_DTYPE records) and delta [3] =
    |dx|, |dy|, |dtheta| between the two registered poses.  Nothing here says which order libstdc++'s sort leaves: the
    spread is between this library's order and its opposite."""
    ctx = ctx or default_context()
    reg = _tie_reg(par, ctx)
    clouds, T = job
    clouds = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 4) for c in clouds]
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(len(clouds), 3)
    fwd = [MapPointNormal(c, radius, origin, weight_intensity, ctx=ctx) for c in clouds]
    rev = [MapPointNormal(np.ascontiguousarray(c[::-1]), radius, origin, weight_intensity, ctx=ctx) for c in clouds]
    res = reg.RegisterBatch([(fwd, T), (rev, T)])
    return {"audit": voxel_order_audit(clouds, radius, MapPointNormal.downsample_factor, ctx=ctx), "result": res[0],
            "result_reversed": res[1], "delta": np.abs(res[0]["pose"] - res[1]["pose"]).reshape(3)}


class CeresCost:
    """cfear_cost: Ceres-compatible evaluation of one association set (n_scan_normal.cpp:264-318)."""

    def __init__(self, reg, scans, Tsrc, itr=1):
        self.ctx = reg.ctx
        p = np.ascontiguousarray(Tsrc, dtype=np.float64)
        self._h = C.c_void_p()
        self.rpb = 1 if reg.par.cost == L.P2L else 2
        self.ctx.check(self.ctx._lib.cfear_cost_prepare(self.ctx.h, reg._handles(scans), len(scans),
                                                        p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(reg.par),
                                                        int(itr), C.byref(self._h)))

    def blocks(self):
        n = self.ctx._lib.cfear_cost_num_blocks(self._h)
        pairs = np.empty((max(n, 1), 3), np.int32)
        w = np.empty(max(n, 1), np.float64)
        self.ctx._lib.cfear_cost_get_blocks(self._h, pairs.ctypes.data, w.ctypes.data)
        return pairs[:n], w[:n]

    def evaluate(self, x):
        n = self.ctx._lib.cfear_cost_num_residuals(self._h)
        r = np.empty(max(n, 1), np.float64)
        J = np.empty((max(n, 1), 3), np.float64)
        xx = (C.c_double * 3)(*[float(v) for v in x])
        self.ctx.check(self.ctx._lib.cfear_cost_evaluate(self._h, xx, r.ctypes.data, J.ctypes.data))
        return r[:n], J[:n]

    def normal_eq(self, x):
        xx = (C.c_double * 3)(*[float(v) for v in x])
        H = (C.c_double * 9)()
        g = (C.c_double * 3)()
        cost = C.c_double()
        self.ctx.check(self.ctx._lib.cfear_cost_normal_eq(self._h, xx, H, g, C.byref(cost)))
        return np.array(H).reshape(3, 3), np.array(g), cost.value

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "h", None):              # the context may already be gone at interpreter exit: its
                self.ctx._lib.cfear_cost_destroy(self._h)   # objects died with it, destroying them again would be a use after free
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# batched radarDriver + OdometryKeyframeFuser
# ------------------------------------------------------------------------------------------------
# ------------------------------------------------------------------------------------------------
# CorAl alignment quality
# ------------------------------------------------------------------------------------------------
class CorAlRadarQuality:
    """CorAlRadarQuality(ref, src, par, Toffset) (coral_alignment_quality AlignmentQuality.cpp:99-230) over
    peak clouds, as ScanLearningInterface::getCorAlQualityMeasure builds it (alignmentinterface.cpp:437-456).

    ref / src: float32 [n, 4] clouds (NumPy or torch CUDA) in their sensor frames; poses (x, y, theta).
    GetQualityMeasure() -> [joint, sep, overlap]; .valid_ as in the reference."""

    def __init__(self, ref_cloud, ref_pose, src_cloud, src_pose, Toffset=(0.0, 0.0, 0.0), radius=1.0,
                 weight_res_intensity=False, want_per_point=False, ctx=None):
        out, pp = coral_quality_batch([(ref_cloud, ref_pose, src_cloud, src_pose, Toffset)], radius,
                                      weight_res_intensity, want_per_point, ctx)
        r = out[0]
        self.quality_ = [float(r["joint"]), float(r["sep"]), float(r["overlap"])]
        self.valid_ = bool(r["valid"])
        self.count_valid = int(r["count_valid"])
        self.path = int(r["pad"])                     # CFEAR_CORAL_PATH_* (diagnostic)
        self.per_point = pp[0] if want_per_point else None
        self.residuals_ = [0.0, 0.0, 0.0]                    # the base constructor's; CorAlRadarQuality adds none

    def GetQualityMeasure(self):
        return list(self.quality_)

    def GetResiduals(self):
        return list(self.residuals_)


def _compose_xyt(a, b):
    """Eigen Affine3d product of two planar poses (x, y, theta): a * b."""
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([c * b[0] - s * b[1] + a[0], s * b[0] + c * b[1] + a[1], a[2] + b[2]], np.float64)


def cfear_quality_batch(jobs, method="P2L", ctx=None):
    """CFEARQuality (AlignmentQuality.cpp:330-354) for a list of (ref_scan, ref_pose, src_scan, src_pose, Toffset):
    a fresh n_scan_normal_reg(method, Huber, 0.3).GetCost on {ref, src} at {T_ref, T_src * Toffset}, one launch.
    -> float64 [n, 3] quality_ = {cost, #residuals, (N_src + N_ref) / 2} ({0, 0, 0} where GetCost fails)."""
    reg = n_scan_normal_reg(method, "Huber", 0.3, 0, ctx=ctx)
    gj = [([rs, ss], np.stack([np.asarray(rp, np.float64), _compose_xyt(np.asarray(sp, np.float64), np.asarray(off, np.float64))]))
          for rs, rp, ss, sp, off in jobs]
    out = reg.GetCostBatch(gj)
    q = np.zeros((len(jobs), 3), np.float64)
    for i, ((rs, _rp, ss, _sp, _off), r) in enumerate(zip(jobs, out)):
        if r["status"] == L.OK:
            q[i] = [r["final_cost"], r["num_residuals"], (ss.GetSize() + rs.GetSize()) / 2.0]
    return q


def coral_quality_batch(jobs, radius=1.0, weight_res_intensity=False, want_per_point=False, ctx=None):
    """jobs: list of (ref_cloud, ref_pose, src_cloud, src_pose, Toffset).  One launch.
    -> (CORAL_RESULT_DTYPE array, per-point list or None)."""
    ctx = ctx or default_context()
    n = len(jobs)
    arr = (L.CoralJob * n)()
    keep, sizes = [], []
    for i, (rc, rp, sc, sp, off) in enumerate(jobs):
        pr, nr, kr = _cloud_ptr(rc)
        ps, ns, ks = _cloud_ptr(sc)
        keep += [kr, ks]
        arr[i].ref_xyzi, arr[i].src_xyzi, arr[i].n_ref, arr[i].n_src = pr, ps, nr, ns
        for k in range(3):
            arr[i].ref_pose[k], arr[i].src_pose[k], arr[i].offset[k] = float(rp[k]), float(sp[k]), float(off[k])
        sizes.append(nr + ns)
    par = L.CoralParams()
    ctx._lib.cfear_coral_params_default(C.byref(par))
    par.radius, par.weight_res_intensity = float(radius), int(weight_res_intensity)
    out = np.zeros(n, L.CORAL_RESULT_DTYPE)
    pp = np.zeros((sum(sizes), 3), np.float64) if want_per_point else None
    if n:
        ctx.check(ctx._lib.cfear_coral_quality_batch(ctx.h, arr, n, C.byref(par), out.ctypes.data,
                                                     pp.ctypes.data if want_per_point else None))
    if not want_per_point:
        return out, None
    offs = np.cumsum([0] + sizes)
    return out, [pp[offs[i]:offs[i + 1]] for i in range(n)]


# ------------------------------------------------------------------------------------------------
# P2P quality, keypoint repeatability, the quality factory and evaluate_scans (coral_alignment_quality)
# ------------------------------------------------------------------------------------------------
def _aff(p):
    c, s = math.cos(float(p[2])), math.sin(float(p[2]))
    return (c, -s, s, c, float(p[0]), float(p[1]))


def _aff_mul(a, b):
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3],
            a[0] * b[4] + a[1] * b[5] + a[4], a[2] * b[4] + a[3] * b[5] + a[5])


def p2p_tchange(ref_pose, src_pose, Toffset=(0.0, 0.0, 0.0)):
    """Tchange = Tref.inverse() * Tsrc * Toffset (AlignmentQuality.cpp:260-264) of planar poses (x, y, theta) as the
    row-major 2x3 float64 [6] a cfear_p2p_job carries.  The inverse is (R^T, -R^T t); every product is a plain fp64
    multiply and add, left to right -- include/cfear_hip.hpp composes with the same formula."""
    return np.array(_tchange(ref_pose, src_pose, Toffset), np.float64)


def _tchange(ref_pose, src_pose, Toffset):
    l0, l1, l2, l3, t0, t1 = _aff(ref_pose)
    inv = (l0, l2, l1, l3, -(l0 * t0 + l2 * t1), -(l1 * t0 + l3 * t1))
    m = _aff_mul(_aff_mul(inv, _aff(src_pose)), _aff(Toffset))
    return (m[0], m[1], m[4], m[2], m[3], m[5])


def p2p_quality_batch(jobs, radius=3.0, want_per_point=False, ctx=None, device_out=False):
    """cfear_p2p_quality_batch: one launch; jobs that share a reference cloud share its sort.  jobs: list of (ref_cloud,
    ref_pose, src_cloud, src_pose, Toffset), or of (ref_cloud, src_cloud, T) with T the composed float64 [6].  Clouds:
    float32 [n, 4], NumPy or torch CUDA (used in place).
    -> (P2P_RESULT_DTYPE array, list of float32 [n_src] rows or None); with device_out torch CUDA tensors instead (uint8
    [n, 32] records to view on the host, one flat float32 tensor) and nothing is synchronised when the clouds are on the
    device too."""
    ctx = ctx or default_context()
    n = len(jobs)
    arr = (L.P2pJob * max(n, 1))()
    keep, sizes = [], []
    for i, job in enumerate(jobs):
        if len(job) == 3:
            rc, sc, T = job
            T = np.asarray(T, np.float64).reshape(6)
        else:
            rc, rp, sc, sp, off = job
            T = _tchange(rp, sp, off)
        pr, nr, kr = _cloud_ptr(rc)
        ps, ns, ks = _cloud_ptr(sc)
        keep += [kr, ks]
        arr[i].ref_xyzi, arr[i].src_xyzi, arr[i].n_ref, arr[i].n_src = pr, ps, nr, ns
        arr[i].T[:] = [float(v) for v in T]
        sizes.append(ns)
    total = int(sum(sizes))
    if device_out:
        import torch
        out = torch.zeros((n, L.P2P_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        pp = torch.zeros(max(total, 1), dtype=torch.float32, device="cuda") if want_per_point else None
    else:
        out = np.zeros(n, L.P2P_RESULT_DTYPE)
        pp = np.zeros(max(total, 1), np.float32) if want_per_point else None
    if n:
        ctx.check(ctx._lib.cfear_p2p_quality_batch(ctx.h, arr, n, float(radius), _ptr(out)[0], _ptr(pp)[0]))
    if not want_per_point:
        return out, None
    if device_out:
        return out, pp[:total]
    offs = np.cumsum([0] + sizes)
    return out, [pp[offs[i]:offs[i + 1]] for i in range(n)]


class AlignmentQualityParameters:
    """AlignmentQuality::parameters (AlignmentQuality.h:53-86)."""

    def __init__(self, method="P2L", radius=3.0, ent_cfg="any", weight_res_intensity=False, output_overlap=True, visualize=False):
        self.method, self.radius, self.ent_cfg = method, float(radius), ent_cfg
        self.weight_res_intensity, self.output_overlap, self.visualize = weight_res_intensity, output_overlap, visualize


def _scan_cloud(scan):
    return scan["cloud"] if "cloud" in scan else scan["cldPeaks"]


class p2pQuality:
    """p2pQuality(ref, src, par, Toffset) (AlignmentQuality.cpp:235-290).  A scan is a dict {"T": (x, y, theta), "cloud":
    float32 [n, 4] (NumPy or torch CUDA)[, "type", "pose_id", "CFEAR"]}.  residuals_ keeps the base constructor's three
    leading zeros (AlignmentQuality.h:92), so quality_[0] = sum / (matched + 3)."""

    def __init__(self, ref, src, par=None, Toffset=(0.0, 0.0, 0.0), ctx=None, _record=None):
        self.par_ = par or AlignmentQualityParameters(method="P2P")
        if _record is None:
            out, pp = p2p_quality_batch([(_scan_cloud(ref), ref["T"], _scan_cloud(src), src["T"], Toffset)], self.par_.radius, True, ctx)
            _record = (out[0], pp[0])
        r, pp = _record
        self.record = r
        self.residuals_ = [0.0, 0.0, 0.0] + [float(v) for v in pp[pp >= 0]]
        self.quality_ = [float(r["mean"]), 0.0, 0.0]
        self.valid_ = False                                   # never set by the reference

    def GetResiduals(self):
        return list(self.residuals_)

    def GetQualityMeasure(self):
        return list(self.quality_)


class keypointRepetability:
    """keypointRepetability(ref, src, par, Toffset) (AlignmentQuality.cpp:293-328): quality_ = {matched / n_src, matched,
    n_src}; NaN for an empty source cloud, as 0.0 / 0.0 is there."""

    def __init__(self, ref, src, par=None, Toffset=(0.0, 0.0, 0.0), ctx=None, _record=None):
        self.par_ = par or AlignmentQualityParameters(method="keypoint_repetability")
        if _record is None:
            out, _ = p2p_quality_batch([(_scan_cloud(ref), ref["T"], _scan_cloud(src), src["T"], Toffset)], self.par_.radius, False, ctx)
            _record = (out[0], None)
        r = _record[0]
        self.record = r
        self.residuals_ = [0.0, 0.0, 0.0]
        self.quality_ = _repeatability(r)
        self.valid_ = False

    def GetResiduals(self):
        return list(self.residuals_)

    def GetQualityMeasure(self):
        return list(self.quality_)


def _repeatability(r):
    with np.errstate(invalid="ignore", divide="ignore"):
        return [float(np.float64(r["matched"]) / np.float64(r["n_src"])), float(r["matched"]), float(r["n_src"])]


class CFEARQuality:
    """CFEARQuality(ref, src, par, Toffset) (AlignmentQuality.cpp:330-354) over scans that carry "CFEAR": MapPointNormal."""

    def __init__(self, ref, src, par, Toffset=(0.0, 0.0, 0.0), ctx=None):
        if par.method not in L.COST:
            raise ValueError("CFEARQuality: unknown cost %r" % (par.method,))
        self.par_ = par
        self.quality_ = [float(v) for v in cfear_quality_batch([(ref["CFEAR"], ref["T"], src["CFEAR"], src["T"], Toffset)], par.method, ctx)[0]]
        self.residuals_ = [0.0, 0.0, 0.0]                      # the matcher's residual vector is not returned by the batched call
        self.valid_ = True

    def GetResiduals(self):
        return list(self.residuals_)

    def GetQualityMeasure(self):
        return list(self.quality_)


# ------------------------------------------------------------------------------------------------
# The Cartesian radar image and CorAlCartQuality (ScanType.cpp:191-209, Utils.cpp:255-339, AlignmentQuality.cpp:356-386)
# ------------------------------------------------------------------------------------------------
def cart_params(**kw):
    """cfear_cart_params with radar_polar_to_cartesian's default arguments (radar_resolution 0.04328, cart_resolution 0.2384,
    cart_pixel_width 300), overridden by keyword."""
    p = L.CartParams()
    L.lib().cfear_cart_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in ("radar_resolution", "cart_resolution", "cart_pixel_width"):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def polar_to_cartesian(images, params=None, ctx=None):
    """convertTo(CV_32F, 1 / 255.0) + radar_polar_to_cartesian for a uint8 sweep [rows, cols] or a batch [b, rows, cols]
    (rows = azimuths) -> float32 [W, W] / [b, W, W]; NumPy -> NumPy, torch CUDA -> torch CUDA (a torch view with a row pitch
    or a batch stride is used in place, and the call is only enqueued).  The fixed-point map of the geometry is built on the
    host once and kept in the context."""
    ctx = ctx or default_context()
    par = params or cart_params()
    d, batch, rows, cols = _desc(images)
    W = int(par.cart_pixel_width)
    shape = (W, W) if images.ndim == 2 else (batch, W, W)
    if _is_torch(images):
        import torch
        assert images.dtype == torch.uint8 and images.stride(-1) == 1
        d.stride = images.stride(-2)
        d.batch_stride = images.stride(0) if images.ndim == 3 else rows * d.stride
        out = torch.empty(tuple(max(v, 0) for v in shape), dtype=torch.float32, device=images.device)
        p = images.data_ptr()
    else:
        images = np.ascontiguousarray(images, dtype=np.uint8)
        out = np.empty(tuple(max(v, 0) for v in shape), np.float32)
        p = _ptr(images)[0]
    ctx.check(ctx._lib.cfear_polar_to_cartesian(ctx.h, p, C.byref(d), C.byref(par), _ptr(out)[0]))
    return out


def _image_ptr(img):
    if _is_torch(img):
        import torch
        assert img.dtype == torch.float32 and img.is_contiguous() and img.ndim == 2 and img.shape[0] == img.shape[1]
        return img.data_ptr(), int(img.shape[0]), img
    a = np.ascontiguousarray(img, dtype=np.float32)
    assert a.ndim == 2 and a.shape[0] == a.shape[1]
    return a.ctypes.data, int(a.shape[0]), a


def cart_quality_batch(jobs, image_res, want_warped=False, ctx=None, device_out=False):
    """cfear_cart_quality_batch: one launch.  jobs: list of (src_image, ref_image, (x, y, yaw)); images float32 [W, W], NumPy
    or torch CUDA (used in place; an image object named by several jobs is uploaded once).  The yaw is handed to
    getRotationMatrix2D as the reference does: radians, read as degrees.
    -> (CART_RESULT_DTYPE array, float32 [n, W, W] warped source images or None); a job with a non-finite pose or an offset
    beyond 2^20 pixels has status ERR_INVALID_ARGUMENT and zeros.  device_out: torch CUDA tensors (uint8 [n, 16] records)."""
    ctx = ctx or default_context()
    n = len(jobs)
    arr = (L.CartJob * max(n, 1))()
    keep, W, seen = [], None, {}
    for i, (src, ref, pose) in enumerate(jobs):
        for name, img in (("src", src), ("ref", ref)):
            if id(img) not in seen:                             # np.ascontiguousarray may copy: one copy per object
                seen[id(img)] = _image_ptr(img)
                keep.append(img)
            ptr, w, _k = seen[id(img)]
            if W is None:
                W = w
            if w != W:
                raise ValueError("cart_quality_batch: images of different widths")
            setattr(arr[i], name, ptr)
        arr[i].x, arr[i].y, arr[i].yaw = float(pose[0]), float(pose[1]), float(pose[2])
    W = W or 1
    if device_out:
        import torch
        out = torch.zeros((n, L.CART_RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        warped = torch.zeros((n, W, W), dtype=torch.float32, device="cuda") if want_warped else None
    else:
        out = np.zeros(n, L.CART_RESULT_DTYPE)
        warped = np.zeros((n, W, W), np.float32) if want_warped else None
    if n:
        ctx.check(ctx._lib.cfear_cart_quality_batch(ctx.h, arr, n, W, float(image_res), _ptr(out)[0], _ptr(warped)[0]))
    return out, warped


class PoseScanParameters:
    """PoseScan::Parameters (ScanType.h:55-91), the members CartesianRadar reads."""

    def __init__(self, scan_type="kstrongCart", sensor_min_distance=2.5, range_res=0.04328, cart_resolution=0.2384, cart_pixel_width=300):
        self.scan_type, self.sensor_min_distance, self.range_res = scan_type, float(sensor_min_distance), float(range_res)
        self.cart_resolution, self.cart_pixel_width = float(np.float32(cart_resolution)), int(cart_pixel_width)


def CartesianRadar(pars, polar, T, pose_id=0, ctx=None, image_params=None):
    """CartesianRadar(pars, polar, T) (ScanType.cpp:191-209) -> a scan dict {"type": "CartesianRadar", "T", "pose_id", "cart":
    float32 [W, W], "cart_resolution", "cart_pixel_width"}.  The reference's constructor calls radar_polar_to_cartesian with
    its DEFAULT arguments (0.04328, 0.2384, 300) whatever pars says, and only stores pars.cart_resolution / cart_pixel_width
    for CorAlCartQuality to read; so does this.  image_params (a cart_params()) overrides the geometry of the image."""
    pars = pars or PoseScanParameters()
    return {"type": "CartesianRadar", "T": tuple(float(v) for v in T), "pose_id": int(pose_id),
            "cart": polar_to_cartesian(polar, image_params, ctx), "cart_resolution": pars.cart_resolution,
            "cart_pixel_width": pars.cart_pixel_width}


def cart_pose_offset(src_pose, Toffset=(0.0, 0.0, 0.0), ref_pose=None):
    """(x, y, yaw) of CorAlCartQuality's Tchange.  The reference takes Tsrc AND Tref from the source scan
    (AlignmentQuality.cpp:363-364): Tchange = Tsrc^-1 Tsrc Toffset, ref_pose is not read.  Composed like p2p_tchange; the
    yaw is eulerAngles(0, 1, 2)[2] of a planar rotation, atan2(m10, m11)."""
    T = _tchange(src_pose, src_pose, Toffset)
    return float(T[2]), float(T[5]), math.atan2(T[3], T[4])


def _cart_job(ref, src, Toffset):
    return (src["cart"], ref["cart"], cart_pose_offset(src["T"], Toffset, ref["T"]))


class CorAlCartQuality:
    """CorAlCartQuality(ref, src, par, Toffset) (AlignmentQuality.cpp:356-386) over two CartesianRadar scans: quality_ =
    {sum |RotoTranslation(src.cart, Tchange, ref.cart_resolution) - ref.cart|, 0, 0}; residuals_ stays {0, 0, 0}."""

    def __init__(self, ref, src, par=None, Toffset=(0.0, 0.0, 0.0), ctx=None, _record=None):
        self.par_ = par or AlignmentQualityParameters()
        if _record is None:
            _record = cart_quality_batch([_cart_job(ref, src, Toffset)], ref.get("cart_resolution", 0.2384), False, ctx)[0][0]
        if int(_record["status"]) != L.OK:
            raise L.CfearError(int(_record["status"]), "CorAlCartQuality: the pose offset is not finite or beyond 2^20 pixels")
        self.record = _record
        self.residuals_ = [0.0, 0.0, 0.0]
        self.quality_ = [float(_record["abs_diff"]), 0.0, 0.0]
        self.valid_ = False                                   # never set by the reference

    def GetResiduals(self):
        return list(self.residuals_)

    def GetQualityMeasure(self):
        return list(self.quality_)


_CFEAR_TYPE, _P2P_TYPES, _CORAL_TYPES = "CFEARFeatures", ("BFARScan", "RawLidar", "kstrongStructuredRadar", "Cen2018Radar"), \
    ("kstrongRadar", "kstrongStructuredRadar")


def _quality_kind(scan_type, method):
    """The measure AlignmentQualityFactory::CreateQualityType (AlignmentQuality.h:260-312) builds for a scan type and
    pars.method: "CFEAR", "P2P", "keypoint_repetability", "Coral" or "CorAlCart" (CartesianRadar scans, whatever the method);
    raises where the reference prints "no quality metric for scan typee" and exits, and for the two measures that are empty
    stubs in the reference."""
    if scan_type == "CartesianRadar":
        return "CorAlCart"
    if scan_type == _CFEAR_TYPE:
        if method not in L.COST:
            raise ValueError("CFEARFeatures: unknown cost %r" % (method,))
        return "CFEAR"
    if method == "P2P" and scan_type in _P2P_TYPES:
        return "P2P"
    if method == "keypoint_repetability" and scan_type == "BFARScan":
        return "keypoint_repetability"
    if method == "Coral" and scan_type in _CORAL_TYPES:
        return "Coral"
    if scan_type == "RawLidar" and method in ("Coral", "P2D"):
        raise NotImplementedError("%s / %s: CorAl (lidar) and p2dQuality are not built" % (scan_type, method))
    raise ValueError("no quality metric for scan type %r with method %r" % (scan_type, method))


def _scan_type(ref, src):
    tr, ts = ref.get("type"), src.get("type")
    if tr is None or tr != ts:
        raise ValueError("no quality metric for scan types %r / %r" % (tr, ts))
    return tr


class AlignmentQualityFactory:
    """AlignmentQualityFactory (AlignmentQuality.h:260-312): dispatch on the scans' "type" tag (the reference's PoseScan
    subclass name) and pars.method."""

    @staticmethod
    def CreateQualityType(ref, src, pars, Toffset=(0.0, 0.0, 0.0), ctx=None):
        kind = _quality_kind(_scan_type(ref, src), pars.method)
        if kind == "CFEAR":
            return CFEARQuality(ref, src, pars, Toffset, ctx)
        if kind == "P2P":
            return p2pQuality(ref, src, pars, Toffset, ctx)
        if kind == "keypoint_repetability":
            return keypointRepetability(ref, src, pars, Toffset, ctx)
        if kind == "CorAlCart":
            return CorAlCartQuality(ref, src, pars, Toffset, ctx)
        if pars.ent_cfg not in ("any", 0):
            raise NotImplementedError("CorAlRadarQuality: only ent_cfg = any is built")
        return CorAlRadarQuality(_scan_cloud(ref), ref["T"], _scan_cloud(src), src["T"], Toffset, pars.radius,
                                 pars.weight_res_intensity, False, ctx)


class scanEvaluatorParameters:
    """scanEvaluator::parameters (ScanEvaluator.h:58-113), the fields that reach the scores and eval.txt."""

    def __init__(self, scan_spacing=1, range_error=0.5, theta_range=2 * math.pi / 4.0, offset_rotation_steps=2,
                 theta_error=0.57 * math.pi / 180.0, output_directory="", output_eval_file="eval.txt"):
        self.scan_spacing, self.range_error, self.theta_range = int(scan_spacing), float(range_error), float(theta_range)
        self.offset_rotation_steps, self.theta_error = int(offset_rotation_steps), float(theta_error)
        self.output_directory, self.output_eval_file = output_directory, output_eval_file


class scanEvaluator:
    """scanEvaluator (ScanEvaluator.cpp:4-114), the body of evaluate_scans: every pair (scan[k - 1], scan[k]), k >=
    scan_spacing, is scored at the aligned offset and at offset_rotation_steps misaligned ones.  All (N - scan_spacing) x
    (steps + 1) jobs go through ONE batched call of the measure the factory picks for the scans' type and quality_par.method
    (p2p_quality_batch, coral_quality_batch, cart_quality_batch or cfear_quality_batch); there is no loop over pairs.
    datapoints_: dicts(index, ref_id, src_id, distance, score, aligned, perturbation, residuals)."""

    HEADER = ["index", "ref_id", "src_id", "distance", " score1", "score2", "score3", "aligned", "error x", "error y", "error theta"]

    def __init__(self, scans, eval_par=None, quality_par=None, ctx=None):
        self.par_ = eval_par or scanEvaluatorParameters()
        self.quality_par_ = quality_par or AlignmentQualityParameters()
        p = self.par_
        if not (p.range_error > 0.0 and p.theta_range >= -2.220446049250313e-16 and p.theta_error >= 0.0 and p.scan_spacing >= 1):
            raise ValueError("scanEvaluator: InputSanityCheck")         # ScanEvaluator.cpp:47-56
        self.vek_perturbation_ = []
        self.CreatePerturbations()
        self.datapoints_ = []
        pairs = [(k, scans[k - 1], scans[k]) for k in range(p.scan_spacing, len(scans))]
        if not pairs:
            return
        kind = _quality_kind(_scan_type(pairs[0][1], pairs[0][2]), self.quality_par_.method)
        for _k, r, s in pairs:
            if _scan_type(r, s) != pairs[0][1]["type"]:
                raise ValueError("scanEvaluator: scans of different types")
        vek, q = self.vek_perturbation_, self.quality_par_
        nres = [[0.0, 0.0, 0.0]] * (len(pairs) * len(vek))
        if kind in ("P2P", "keypoint_repetability"):
            want_pp = kind == "P2P"
            out, pp = p2p_quality_batch([(_scan_cloud(r), r["T"], _scan_cloud(s), s["T"], o) for _k, r, s in pairs for o in vek],
                                        q.radius, want_pp, ctx)
            if want_pp:
                scores = [[float(v["mean"]), 0.0, 0.0] for v in out]
                nres = [[0.0, 0.0, 0.0] + [float(x) for x in row[row >= 0]] for row in pp]
            else:
                scores = [_repeatability(v) for v in out]
        elif kind == "CorAlCart":
            res = {float(np.float32(r.get("cart_resolution", 0.2384))) for _k, r, _s in pairs}
            if len(res) != 1:
                raise ValueError("scanEvaluator: CartesianRadar scans of different cart_resolution")
            out, _ = cart_quality_batch([_cart_job(r, s, o) for _k, r, s in pairs for o in vek], res.pop(), False, ctx)
            for v in out:
                if int(v["status"]) != L.OK:
                    raise L.CfearError(int(v["status"]), "CorAlCartQuality: the pose offset is not finite or beyond 2^20 pixels")
            scores = [[float(v["abs_diff"]), 0.0, 0.0] for v in out]
        elif kind == "Coral":
            if q.ent_cfg not in ("any", 0):
                raise NotImplementedError("CorAlRadarQuality: only ent_cfg = any is built")
            out, _ = coral_quality_batch([(_scan_cloud(r), r["T"], _scan_cloud(s), s["T"], o) for _k, r, s in pairs for o in vek],
                                         q.radius, q.weight_res_intensity, False, ctx)
            scores = [[float(v["joint"]), float(v["sep"]), float(v["overlap"])] for v in out]
        else:
            X = cfear_quality_batch([(r["CFEAR"], r["T"], s["CFEAR"], s["T"], o) for _k, r, s in pairs for o in vek], q.method, ctx)
            scores = [[float(x) for x in row] for row in X]
        i = 0
        for index, (k, r, s) in enumerate(pairs, 1):
            dx, dy = float(r["T"][0]) - float(s["T"][0]), float(r["T"][1]) - float(s["T"][1])
            for verr in vek:
                self.datapoints_.append(dict(index=index, ref_id=int(r.get("pose_id", k - 1)), src_id=int(s.get("pose_id", k)),
                                             distance=math.sqrt(dx * dx + dy * dy), score=scores[i], aligned=self.aligned(verr),
                                             perturbation=list(verr), residuals=nres[i]))
                i += 1

    @staticmethod
    def aligned(perturbation):                                           # datapoint::aligned (:4-10)
        total = 0.0
        for e in perturbation:
            total += abs(e)
        return total < 0.0001

    def CreatePerturbations(self):                                       # :11-25
        p = self.par_
        steps = p.offset_rotation_steps
        angles = [float(i) / float(steps) * p.theta_range for i in range(steps)]
        self.vek_perturbation_ += [[0.0, 0.0, 0.0]] + [[p.range_error * math.cos(a), p.range_error * math.sin(a), p.theta_error]
                                                       for a in angles]

    @staticmethod
    def ValsToString(d):                                                 # datapoint::ValsToString: std::to_string
        return ["%d" % d["index"], "%d" % d["ref_id"], "%d" % d["src_id"], "%f" % d["distance"], "%f" % d["score"][0],
                "%f" % d["score"][1], "%f" % d["score"][2], "%d" % int(d["aligned"]), "%f" % d["perturbation"][0],
                "%f" % d["perturbation"][1], "%f" % d["perturbation"][2]]

    def EvaluationText(self):
        """eval.txt: datapoint::HeaderToString(), then one row per datapoint, joined by Vec2String (Utils.cpp:596-604)."""
        return "".join(",".join(v) + "\n" for v in [self.HEADER] + [self.ValsToString(d) for d in self.datapoints_])

    def SaveEvaluation(self, path=None):                                 # :26-46
        assert self.datapoints_
        path = path or os.path.join(self.par_.output_directory, self.par_.output_eval_file)
        with open(path, "w") as f:
            f.write(self.EvaluationText())
        return path


# ------------------------------------------------------------------------------------------------
# loop-candidate verification (tbv_slam loopclosure + alignment_checker ScanLearningInterface)
# ------------------------------------------------------------------------------------------------
ODOM_BOUNDS, SC_SIM, CFEAR_COST, CORAL_COST, COMBINED_COST = "odom-bounds", "sc-sim", "CFEAR", "coral", "alignment_quality"


def verify_params(ctx=None, **kw):
    """cfear_verify_params with loopclosure::BaseParameters' defaults (tbv_slam/include/tbv_slam/loopclosure.h:117-138);
    align_coef / loop_coef accept sequences (6 and 3 values)."""
    ctx = ctx or default_context()
    p = L.VerifyParams()
    ctx._lib.cfear_verify_params_default(C.byref(p))
    for k, v in kw.items():
        if k in ("align_coef", "loop_coef"):
            arr = getattr(p, k)
            assert len(v) == len(arr), k
            for i, x in enumerate(v):
                arr[i] = float(x)
        elif k in ("coral_radius",):
            p.coral.radius = float(v)
        else:
            assert hasattr(p, k), k
            setattr(p, k, type(getattr(p, k))(v))
    return p


def VerifyByOdometry(rel_xyt, odom_sigma_error=0.03, verify_via_odometry=True, ctx=None):
    """loopclosure::VerifyByOdometry (loopclosure.cpp:776-808): rel_xyt [n, 3] = RelativeMotion(i, i+1) for
    i = to .. from-1 -> similarity (quality["odom-bounds"])."""
    r = np.ascontiguousarray(rel_xyt, dtype=np.float64).reshape(-1, 3)          # (host arithmetic: no context is made for it)
    out = C.c_double()
    rc = L.lib().cfear_verify_by_odometry(r.ctypes.data, int(r.shape[0]), float(odom_sigma_error),
                                          int(bool(verify_via_odometry)), C.byref(out))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_verify_by_odometry")
    return out.value


def verify_loop_candidates(cands, par=None, ctx=None, device_ptr=None):
    """RegisterLoopCandidate + VerifyLoopCandidate + ApplyConstratins (loopclosure.cpp:320-384, 261-274) for a batch.
    cands: list of dicts with keys from_scan, to_scan (MapPointNormal), from_peaks, to_peaks (float32 [n, 4], NumPy
    or torch CUDA), from_pose (x, y, theta), t_be_guess, sc_sim, odom_bounds, group -- or a prepare_verify_batch
    result.  -> VERIFY_RESULT_DTYPE array; with device_ptr (a device buffer of n * 480 bytes) the records stay there
    WITHOUT the selection (accepted = rank = 0: verify_apply_constraints over the gathered list) and n is returned."""
    ctx = ctx or default_context()
    par = par or verify_params(ctx)
    arr, n, _keep = cands if isinstance(cands, tuple) else prepare_verify_batch(cands)
    out = None if device_ptr is not None else np.zeros(n, L.VERIFY_RESULT_DTYPE)
    if n:
        dst = C.c_void_p(int(device_ptr)) if device_ptr is not None else C.c_void_p(out.ctypes.data)
        ctx.check(ctx._lib.cfear_verify_loop_candidates(ctx.h, arr, n, C.byref(par), dst))
    return n if device_ptr is not None else out


def verify_apply_constraints(results, groups, par):
    """cfear_verify_apply_constraints: ApplyConstratins (loopclosure.cpp:261-274) over gathered records, in place."""
    g = np.ascontiguousarray(groups, dtype=np.int32)
    assert results.flags["C_CONTIGUOUS"] and results.dtype == L.VERIFY_RESULT_DTYPE and g.shape[0] == results.shape[0]
    rc = L.lib().cfear_verify_apply_constraints(C.c_void_p(g.ctypes.data), int(g.shape[0]), C.byref(par), C.c_void_p(results.ctypes.data))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_verify_apply_constraints")
    return results


def prepare_verify_batch(cands):
    """Marshals a candidate list once; the result can be passed to verify_loop_candidates repeatedly."""
    n = len(cands)
    arr = (L.VerifyJob * n)()
    keep = []
    for i, c in enumerate(cands):
        pf, nf, kf = _cloud_ptr(c["from_peaks"])
        pt, nt, kt = _cloud_ptr(c["to_peaks"])
        keep += [kf, kt]
        j = arr[i]
        j.from_scan, j.to_scan = c["from_scan"]._h, c["to_scan"]._h
        j.from_peaks, j.to_peaks, j.n_from, j.n_to = pf, pt, nf, nt
        for k in range(3):
            j.from_pose[k] = float(c["from_pose"][k])
            j.t_be_guess[k] = float(c.get("t_be_guess", (0.0, 0.0, 0.0))[k])
        j.sc_sim, j.odom_bounds = float(c.get("sc_sim", 0.0)), float(c.get("odom_bounds", 0.0))
        j.group = int(c.get("group", 0))
    return (arr, n, keep + [cands])


def loop_verify_params(**kw):
    """cfear_loop_verify_params with the reference's defaults (loopclosure.h:122-127: verify_via_odometry, odom_sigma_error
    0.03, transl_guess, speedup off; odometry_coupled_closure as the detector's default).  Keywords name its own fields,
    verify = a verify_params() record, or fields of that record."""
    p = L.LoopVerifyParams()
    L.lib().cfear_loop_verify_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "verify":
            p.verify = v
        elif k in ("odom_sigma_error", "verify_via_odometry", "transl_guess", "speedup", "odometry_coupled_closure"):
            setattr(p, k, type(getattr(p, k))(v))
        elif k in ("align_coef", "loop_coef"):
            for i, x in enumerate(v):
                getattr(p.verify, k)[i] = float(x)
        else:
            if k == "pad" or not hasattr(p.verify, k):
                raise L.CfearError(L.ERR_INVALID_ARGUMENT, "unknown cfear_loop_verify_params field %r" % (k,))
            setattr(p.verify, k, type(getattr(p.verify, k))(v))
    return p


def loop_relative_motions(poses_xyt, node_off):
    """rel_xyt [n_nodes, 3] of cfear_loop_graphs from the nodes' poses: RelativeMotion(k, k + 1) = pose[k]^-1 * pose[k + 1]
    within every graph (the entry of a graph's last node is 0), for graphs whose odometry constraints are their poses'."""
    P = np.asarray(poses_xyt, np.float64).reshape(-1, 3)
    rel = np.zeros_like(P)
    for g in range(len(node_off) - 1):
        for k in range(int(node_off[g]), int(node_off[g + 1]) - 1):
            a, b = P[k], P[k + 1]
            c, s = np.cos(a[2]), np.sin(a[2])
            inv = np.array([-(c * a[0] + s * a[1]), s * a[0] - c * a[1], -a[2]])
            ci, si = np.cos(inv[2]), np.sin(inv[2])
            rel[k] = (ci * b[0] - si * b[1] + inv[0], si * b[0] + ci * b[1] + inv[1], inv[2] + b[2])
    return rel


def _loop_graphs(graphs):
    """cfear_loop_graphs of dict(node_off, table, xyzi, point_off, poses, rel): the flat arrays of sc_flatten_graphs plus a
    ScanTable over all nodes, the nodes' poses [n, 3] and their relative motions [n, 3] (or None) -> (record, keep-alive)."""
    node_off = np.ascontiguousarray(graphs["node_off"], np.int32)
    po = None if graphs.get("point_off") is None else np.ascontiguousarray(graphs["point_off"], np.int64)
    poses = None if graphs.get("poses") is None else np.ascontiguousarray(graphs["poses"], np.float64)
    rel = None if graphs.get("rel") is None else np.ascontiguousarray(graphs["rel"], np.float64)
    xyzi = graphs.get("xyzi")
    if xyzi is not None and not _is_torch(xyzi):
        xyzi = np.ascontiguousarray(xyzi, np.float32)
    g = L.LoopGraphs()
    g.n_graphs = node_off.shape[0] - 1
    g.node_off = node_off.ctypes.data
    table = graphs.get("table")
    g.table = table._h if table is not None else None
    g.peaks_xyzi = _ptr(xyzi)[0]
    g.peak_off = None if po is None else po.ctypes.data
    g.poses_xyt = None if poses is None else poses.ctypes.data
    g.rel_xyt = None if rel is None else rel.ctypes.data
    return g, [node_off, po, poses, rel, xyzi, table]


def _loop_verify_outputs(ctx, cap, device_out, want_loops):
    if device_out:
        import torch
        dev = "cuda:%d" % ctx.device
        res = torch.zeros(max(cap, 1) * L.VERIFY_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        lst = torch.zeros(max(cap, 1) * L.LOOP_VERIFY_CANDIDATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        loops = torch.zeros(max(cap, 1) * L.LOOP_CANDIDATE_DTYPE.itemsize, dtype=torch.uint8, device=dev) if want_loops else None
    else:
        res = np.zeros(max(cap, 1), L.VERIFY_RESULT_DTYPE)
        lst = np.zeros(max(cap, 1), L.LOOP_VERIFY_CANDIDATE_DTYPE)
        loops = np.zeros(max(cap, 1), L.LOOP_CANDIDATE_DTYPE) if want_loops else None
    return res, lst, loops


def _loop_verify_result(n, res, lst, loops):
    sizes = (L.VERIFY_RESULT_DTYPE.itemsize, L.LOOP_VERIFY_CANDIDATE_DTYPE.itemsize, L.LOOP_CANDIDATE_DTYPE.itemsize)
    cut = [None if x is None else (x[:n * sz] if _is_torch(x) else x[:n]) for x, sz in zip((res, lst, loops), sizes)]
    return dict(n=n, results=cut[0], list=cut[1], loops=cut[2])


def loop_verify_candidates(cands):
    """LOOP_VERIFY_CANDIDATE_DTYPE records from such an array or from dicts with graph, from, to and optionally guess_nr,
    query (default: 2^16 graph + from), skip, guess_xyt, sc_sim, odom_term."""
    if isinstance(cands, np.ndarray) and cands.dtype == L.LOOP_VERIFY_CANDIDATE_DTYPE:
        return np.ascontiguousarray(cands)
    out = np.zeros(len(cands), L.LOOP_VERIFY_CANDIDATE_DTYPE)
    for i, c in enumerate(cands):
        g, f = int(c.get("graph", 0)), int(c["from"])
        out[i] = (g, f, int(c["to"]), int(c.get("guess_nr", 0)), int(c.get("query", (g << 16) + f)), int(c.get("skip", 0)),
                  np.asarray(c.get("guess_xyt", (0.0, 0.0, 0.0)), np.float64).reshape(3), float(c.get("sc_sim", 0.0)),
                  float(c.get("odom_term", 0.0)))
    return out


def verify_graph_candidates(graphs, cands, par=None, ctx=None, device_out=False, want_loops=False):
    """cfear_verify_graph_candidates: a candidate list of a batch of graphs (MiniClosure / GTVicinity pairs, a caller's own)
    verified as verify_loop_candidates verifies it, with the scans, peaks, poses and quality["odom-bounds"] looked up and
    computed on the device.  graphs: dict(node_off, table = a ScanTable with one entry per node, xyzi + point_off = the
    nodes' peaks as sc_flatten_graphs lays them out (NumPy or torch CUDA), poses [n, 3], rel [n, 3] or None (see
    loop_relative_motions)).  cands: loop_verify_candidates() input, or a torch CUDA uint8 tensor of such records.
    -> dict(n, results = VERIFY_RESULT_DTYPE records, list = LOOP_VERIFY_CANDIDATE_DTYPE records, loops =
    LOOP_CANDIDATE_DTYPE records with guess_xyt = the registered t_be, if want_loops); with device_out all three as torch
    CUDA uint8 tensors of the records' bytes, accepted = rank = 0 (verify_apply_constraints is the caller's)."""
    ctx = ctx or default_context()
    par = par or loop_verify_params()
    g, keep = _loop_graphs(graphs)
    if _is_torch(cands):
        n = cands.numel() // L.LOOP_VERIFY_CANDIDATE_DTYPE.itemsize
    else:
        cands = loop_verify_candidates(cands)
        n = cands.shape[0]
    res, lst, loops = _loop_verify_outputs(ctx, n, device_out, want_loops)
    _torch_ready(ctx, res, lst, loops, cands, graphs.get("xyzi"))
    ctx.check(ctx._lib.cfear_verify_graph_candidates(ctx.h, C.byref(g), _ptr(cands)[0] if n else None, n, C.byref(par), _ptr(res)[0],
                                                     _ptr(lst)[0], _ptr(loops)[0]))
    del keep
    return _loop_verify_result(n, res, lst, loops)


def verify_sc_rows(graphs, rows, n_out, n_detect=None, par=None, ctx=None, device_out=False, want_loops=False):
    """cfear_verify_sc_rows: the body of ScanContextClosure::SearchAndAddConstraint (loopclosure.cpp:653-724) for the rows
    of sc_detect_batch(device_out=True) or (records=True), which never have to leave the device: row -> (from, to, guess_nr),
    the speedup rule, Tsrcguess under transl_guess, VerifyByOdometry, registration and verification, ApplyConstratins per
    query (host results).  graphs: as verify_graph_candidates; rows [D, n_candidates] SC_CANDIDATE_DTYPE (or the uint8
    [D, n_candidates, 64] tensor), n_out [D]; n_detect one count per graph (default: every node).  -> as
    verify_graph_candidates, n = the number of compacted candidates."""
    ctx = ctx or default_context()
    par = par or loop_verify_params()
    g, keep = _loop_graphs(graphs)
    nd = None if n_detect is None else np.ascontiguousarray(n_detect, np.int32)
    if _is_torch(rows):
        nc = int(rows.shape[1]) if rows.dim() >= 2 else 0
    else:
        rows = np.ascontiguousarray(rows, L.SC_CANDIDATE_DTYPE)
        nc = int(rows.shape[1]) if rows.ndim == 2 else 0
    if n_out is not None and not _is_torch(n_out):
        n_out = np.ascontiguousarray(n_out, np.int32)
    D = int(np.diff(np.asarray(graphs["node_off"])).clip(0).sum()) if nd is None else int(nd.clip(0).sum())
    res, lst, loops = _loop_verify_outputs(ctx, D * max(nc, 0), device_out, want_loops)
    n = C.c_int32(0)
    _torch_ready(ctx, res, lst, loops, rows, n_out, graphs.get("xyzi"))
    ctx.check(ctx._lib.cfear_verify_sc_rows(ctx.h, C.byref(g), _ptr(rows)[0], _ptr(n_out)[0], None if nd is None else nd.ctypes.data, nc,
                                            C.byref(par), _ptr(res)[0], _ptr(lst)[0], _ptr(loops)[0], C.byref(n)))
    del keep
    return _loop_verify_result(int(n.value), res, lst, loops)


def verify_sample_covariances(graphs, out, par=None, ctx=None):
    """cfear_verify_sample_covariances: sampled covariances (use_covariance_sampling_in_loop_closure) for the candidates
    verify_graph_candidates / verify_sc_rows verified, as a pass of its own.  out: the dict either returned, with host
    records or with device_out; its `results` are updated IN PLACE -- `cov` and `cov_sampled` of every candidate that was
    registered and whose fit is accepted, no other byte -- and `out` is returned.  par: loop_verify_params(); its
    verify.sampling is what is read (use_covariance_sampling is not)."""
    ctx = ctx or default_context()
    par = par or loop_verify_params()
    g, keep = _loop_graphs(graphs)
    n = int(out["n"])
    res, lst = out["results"], out["list"]
    if not _is_torch(res) and not (res.flags["C_CONTIGUOUS"] and res.flags["WRITEABLE"]):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "results must be a contiguous, writeable array: they are updated in place")
    _torch_ready(ctx, res, lst)
    ctx.check(ctx._lib.cfear_verify_sample_covariances(ctx.h, C.byref(g), _ptr(lst)[0] if n else None, n, C.byref(par),
                                                       _ptr(res)[0] if n else None))
    del keep
    return out


def cov_fit_records(regs, samples, sampling=None, ctx=None):
    """cfear_cov_fit_records: the covariance fit of cost sampling as a kernel.  regs [n] RESULT_DTYPE, samples [n, m]
    RESULT_DTYPE (m = samples_per_axis^3: the records the matcher's sampling mode leaves) -> (success [n] int32,
    cov [n, 6, 6]).  With torch CUDA uint8 tensors of the records' bytes for both, the outputs are torch CUDA tensors
    (int32 [n], float64 [n, 6, 6]) and the call is only enqueued."""
    ctx = ctx or default_context()
    sp = sampling or n_scan_normal_reg.sampling_params()
    if _is_torch(regs) != _is_torch(samples):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "regs and samples must be both NumPy arrays or both torch CUDA tensors")
    if _is_torch(regs):
        import torch
        n = regs.numel() // L.RESULT_DTYPE.itemsize
        cov = torch.zeros((n, 6, 6), dtype=torch.float64, device=regs.device)
        ok = torch.zeros(n, dtype=torch.int32, device=regs.device)
    else:
        regs = np.ascontiguousarray(regs, L.RESULT_DTYPE)
        samples = np.ascontiguousarray(samples, L.RESULT_DTYPE)
        n = regs.shape[0]
        cov, ok = np.zeros((n, 6, 6), np.float64), np.zeros(n, np.int32)
    _torch_ready(ctx, regs, samples, cov, ok)
    ctx.check(ctx._lib.cfear_cov_fit_records(ctx.h, _ptr(regs)[0], _ptr(samples)[0], n, C.byref(sp), _ptr(cov)[0], _ptr(ok)[0]))
    return ok, cov


def covariance_by_sampling_candidates(table, cands, regs, par=None, sampling=None, ctx=None):
    """cfear_covariance_by_sampling_candidates: covariance by cost sampling for candidate pairs of a ScanTable, the
    counterpart of n_scan_normal_reg.RegisterCandidates, with no host round trip between the samples and the covariance.
    cands: a CANDIDATE_DTYPE array or a torch CUDA uint8 tensor of such records; regs: the RESULT_DTYPE records of the
    candidates' registration (NumPy), or a torch CUDA uint8 tensor of them -- then the outputs are torch CUDA tensors.
    par: the RegParams (or n_scan_normal_reg) of that registration.  -> (success [n] int32, cov [n, 6, 6])."""
    ctx = ctx or default_context()
    reg = _tie_reg(par, ctx)
    sp = sampling or n_scan_normal_reg.sampling_params()
    if _is_torch(cands):
        n = cands.numel() // L.CANDIDATE_DTYPE.itemsize
    else:
        cands = np.ascontiguousarray(cands, dtype=L.CANDIDATE_DTYPE)
        n = cands.shape[0]
    if _is_torch(regs):
        import torch
        cov = torch.zeros((n, 6, 6), dtype=torch.float64, device=regs.device)
        ok = torch.zeros(n, dtype=torch.int32, device=regs.device)
    else:
        regs = np.ascontiguousarray(regs, L.RESULT_DTYPE)
        cov, ok = np.zeros((n, 6, 6), np.float64), np.zeros(n, np.int32)
    _torch_ready(ctx, cands, regs, cov, ok)
    ctx.check(ctx._lib.cfear_covariance_by_sampling_candidates(ctx.h, table._h, _ptr(cands)[0] if n else None, n, C.byref(reg.par),
                                                               _ptr(regs)[0], C.byref(sp), _ptr(cov)[0], _ptr(ok)[0]))
    return ok, cov


def logreg_params(ctx=None, **kw):
    """cfear_logreg_params with the reference's settings (C = 1, balanced class weights, intercept, 100 Newton steps)."""
    p = L.LogregParams()
    L.lib().cfear_logreg_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in ("C", "class_weight_balanced", "fit_intercept", "max_iterations"):
            raise KeyError(k)
        setattr(p, k, float(v) if k == "C" else int(v))
    return p


def logreg_fit_batch(jobs, ctx=None, **params):
    """cfear_logreg_fit_batch: every model of `jobs` fitted in one launch -> LOGREG_RESULT_DTYPE array (coef[n_features:] = 0).
    A job is a dict, or a tuple in this order, of
      X         float64 [n_rows, row_stride], NumPy (host) or torch CUDA tensor, rows contiguous
      y         float64 [n_rows], 0 or 1
      columns   optional: the indices into a row that are the model's features (default: all of them, at most 8)
      row_mask  optional: uint8 / bool [n_rows], 0 = the row is left out
    Jobs that pass the same array object share its upload.  params: C, class_weight_balanced, fit_intercept,
    max_iterations.  A job's own failure is its record's status; arguments the library refuses raise CfearError."""
    ctx = ctx or default_context()
    par = logreg_params(ctx, **params)
    n = len(jobs)
    arr = (L.LogregJob * max(n, 1))()
    seen, keep = {}, []

    def buf(x, dtype):
        if x is None:
            return None, None
        if id(x) not in seen:
            if _is_torch(x):
                import torch
                want = {np.float64: torch.float64, np.uint8: torch.uint8}[dtype]
                v = x.view(torch.uint8) if dtype is np.uint8 and x.dtype == torch.bool else x
                assert v.dtype == want and v.is_contiguous(), "torch buffers must be contiguous %s" % want
            else:
                v = np.ascontiguousarray(x, dtype=dtype)
            seen[id(x)] = v
            keep.append((x, v))
        v = seen[id(x)]
        return _ptr(v)[0], v

    for i, job in enumerate(jobs):
        if not isinstance(job, dict):
            job = dict(zip(("X", "y", "columns", "row_mask"), job))
        pX, X = buf(job["X"], np.float64)
        py, y = buf(job["y"], np.float64)
        pm, m = buf(job.get("row_mask"), np.uint8)
        assert X.ndim == 2 and y.ndim == 1 and y.shape[0] == X.shape[0] and (m is None or tuple(m.shape) == (X.shape[0],))
        cols = job.get("columns")
        j = arr[i]
        j.X, j.y, j.row_mask = pX, py, pm
        j.n_rows, j.row_stride = int(X.shape[0]), int(X.shape[1])
        if cols is None:
            j.columns, j.n_features = None, int(X.shape[1])
        else:
            c = (C.c_int32 * len(cols))(*[int(k) for k in cols])
            keep.append(c)
            j.columns, j.n_features = c, len(cols)
    out = np.zeros(n, L.LOGREG_RESULT_DTYPE)
    ctx.check(ctx._lib.cfear_logreg_fit_batch(ctx.h, arr, n, C.byref(par), out.ctypes.data))
    return out


class LogisticRegression:
    """PythonClassifierInterface + LogisticRegression (alignmentinterface.cpp:14-279): training rows, the two text
    formats, predict_linear.  fit() is sklearn's LogisticRegression(class_weight="balanced", max_iter=1000), the
    call the reference makes through pybind11 (:192-222); fit_device() minimises the same objective on the GPU
    (cfear_logreg_fit_batch) and needs no sklearn."""

    def __init__(self):
        self.X_ = np.zeros((0, 0))
        self.y_ = np.zeros((0,))
        self.coef_ = None
        self.intercept_ = 0.0
        self.is_fit_ = False

    def IsFit(self):
        return self.is_fit_

    def AddDataPoint(self, X_i, y_i):                                   # :51-67
        X_i = np.atleast_2d(np.asarray(X_i, np.float64))
        y_i = np.atleast_1d(np.asarray(y_i, np.float64))
        self.X_ = X_i if self.X_.shape[0] == 0 else np.vstack([self.X_, X_i])
        self.y_ = y_i if self.y_.shape[0] == 0 else np.concatenate([self.y_, y_i])

    def DataValid(self):                                                # :175-187
        return (self.X_.shape[0] == self.y_.shape[0] and self.y_.shape[0] >= 1 and np.isfinite(self.X_).all()
                and np.isfinite(self.y_).all())

    def fit(self):
        if not self.DataValid():
            raise ValueError("training data invalid")                   # the reference calls exit(0) (:194-196)
        from sklearn.linear_model import LogisticRegression as SkLR
        clf = SkLR(class_weight="balanced", max_iter=1000).fit(self.X_, self.y_)
        self.coef_ = np.asarray(clf.coef_[0], np.float64).copy()
        self.intercept_ = float(clf.intercept_[0])
        self.is_fit_ = True

    def _take_record(self, r):
        """Adopts one cfear_logreg_result; what the reference exits on raises ValueError, as fit() does."""
        self.fit_record_ = r
        if r["status"] == L.ERR_INVALID_ARGUMENT:
            raise ValueError("training data invalid")
        if r["status"] != L.OK:
            raise L.CfearError(int(r["status"]), "logistic regression did not converge in %d Newton steps" % r["iterations"])
        self.coef_ = np.array(r["coef"][:self.X_.shape[1]], np.float64)
        self.intercept_ = float(r["intercept"])
        self.is_fit_ = True

    def fit_device(self, ctx=None, **params):
        """fit() on the GPU: the minimiser of sklearn's objective by Newton's method in fp64 -> the cfear_logreg_result
        record (objective, grad_inf, iterations, confusion, balanced_accuracy: what the reference prints, :211)."""
        if not self.DataValid():
            raise ValueError("training data invalid")
        self._take_record(logreg_fit_batch([(self.X_, self.y_)], ctx, **params)[0])
        return self.fit_record_

    def LoadData(self, path):                                           # :103-134: "y,x0,x1,..." per line
        rows = [ln.strip().split(",") for ln in open(path) if ln.strip()]
        if rows:
            a = np.array(rows, dtype=np.float64)
            self.y_, self.X_ = a[:, 0].copy(), a[:, 1:].copy()

    def SaveData(self, path):                                           # :152-173, default ostream precision (%g)
        with open(path, "w") as f:
            for y, x in zip(self.y_, self.X_):
                f.write(",".join(["%g" % y] + ["%g" % v for v in x]) + "\n")

    def LoadCoefficients(self, path):                                   # :224-253: "intercept,c0,c1,..."
        for ln in open(path):
            v = [float(t) for t in ln.strip().split(",") if t]
            if v:
                self.intercept_, self.coef_ = v[0], np.array(v[1:], np.float64)
        self.is_fit_ = True

    def SaveCoefficients(self, path):                                   # :255-269
        with open(path, "w") as f:
            f.write(",".join(["%g" % self.intercept_] + ["%g" % c for c in self.coef_]) + "\n")

    def predict_linear(self, X):                                        # :271-279
        return np.atleast_2d(np.asarray(X, np.float64)) @ self.coef_ + self.intercept_

    def predict_proba(self, X):                                         # :21-33: P(y = 1); zeros when not fitted
        if not self.is_fit_:
            return np.zeros(np.atleast_2d(X).shape[0])
        return 1.0 / (1.0 + np.exp(-self.predict_linear(X)))


class ScanLearningInterface:
    """ScanLearningInterface (alignment_checker/alignmentinterface.h:96-213, alignmentinterface.cpp:288-510).
    A scan is a dict {"T": (x, y, theta), "cldPeaks": float32 [n, 4], "CFEAR": MapPointNormal} (s_scan, :103-109).
    Every CorAl / CFEAR quality evaluation of one call -- the 13 perturbations of AddTrainingData -- is one launch."""

    range_error_, min_dist_btw_scans_ = 0.5, 0.5                         # alignmentinterface.h:196-197
    small_th_err, medium_th_err, large_th_err = 0.5 * np.pi / 180.0, 2 * np.pi / 180.0, 15 * np.pi / 180.0

    def __init__(self, combined=True, ctx=None):
        self.ctx = ctx or default_context()
        self.combined_ = combined
        self.cfear_class, self.coral_class, self.combined_class = LogisticRegression(), LogisticRegression(), LogisticRegression()
        self.frame_ = 0
        self.prev_ = None
        e = self.range_error_                                            # CreatePerturbations (:479-495)
        self.vek_perturbation_ = [(0.0, 0.0, 0.0)]
        for m, th in ((1, self.small_th_err), (2, self.medium_th_err), (4, self.large_th_err)):
            self.vek_perturbation_ += [(m * e, 0.0, th), (0.0, m * e, th), (-m * e, 0.0, th), (0.0, -m * e, th)]

    def _quality(self, current, prev, offsets):
        """X_CorAl, X_CFEAR [len(offsets), 3] for ref = current, src = prev * Toffset (getCorAlQualityMeasure :437-456,
        getCFEARQualityMeasure :459-478)."""
        cj = [(current["cldPeaks"], current["T"], prev["cldPeaks"], prev["T"], o) for o in offsets]
        qj = [(current["CFEAR"], current["T"], prev["CFEAR"], prev["T"], o) for o in offsets]
        co, _ = coral_quality_batch(cj, 1.0, False, False, self.ctx)
        X_coral = np.stack([co["joint"], co["sep"], co["overlap"]], 1).astype(np.float64)
        X_cfear = cfear_quality_batch(qj, "P2L", self.ctx)
        return X_coral, X_cfear

    def AddTrainingData(self, current):                                  # :296-347
        first = self.frame_ == 0
        self.frame_ += 1
        if first:
            self.prev_ = current
            return
        d = np.hypot(current["T"][0] - self.prev_["T"][0], current["T"][1] - self.prev_["T"][1])
        if d < self.min_dist_btw_scans_:
            return
        Xc, Xf = self._quality(current, self.prev_, self.vek_perturbation_)
        for verr, xc, xf in zip(self.vek_perturbation_, Xc, Xf):
            y = float(sum(abs(v) for v in verr) < 0.0001)
            if self.combined_:
                self.combined_class.AddDataPoint(np.concatenate([xc, xf]), y)
            else:
                self.coral_class.AddDataPoint(xc, y)
                self.cfear_class.AddDataPoint(xf, y)
        self.prev_ = current

    def AddTrainingDataBatch(self, scans):
        """AddTrainingData for a whole sequence: the same first-frame, min_dist_btw_scans_ and prev_ bookkeeping as calling
        it scan by scan, but every kept pair x the 13 perturbations goes through ONE coral_quality_batch launch and ONE
        cfear_quality_batch launch instead of one of each per pair."""
        pairs = []
        for current in scans:
            first = self.frame_ == 0
            self.frame_ += 1
            if first:
                self.prev_ = current
                continue
            d = np.hypot(current["T"][0] - self.prev_["T"][0], current["T"][1] - self.prev_["T"][1])
            if d < self.min_dist_btw_scans_:
                continue
            pairs.append((current, self.prev_))
            self.prev_ = current
        if not pairs:
            return
        cj = [(c["cldPeaks"], c["T"], p["cldPeaks"], p["T"], o) for c, p in pairs for o in self.vek_perturbation_]
        qj = [(c["CFEAR"], c["T"], p["CFEAR"], p["T"], o) for c, p in pairs for o in self.vek_perturbation_]
        co, _ = coral_quality_batch(cj, 1.0, False, False, self.ctx)
        Xc = np.stack([co["joint"], co["sep"], co["overlap"]], 1).astype(np.float64)
        Xf = cfear_quality_batch(qj, "P2L", self.ctx)
        y = np.array([float(sum(abs(v) for v in verr) < 0.0001) for verr in self.vek_perturbation_] * len(pairs), np.float64)
        if self.combined_:
            self.combined_class.AddDataPoint(np.concatenate([Xc, Xf], 1), y)
        else:
            self.coral_class.AddDataPoint(Xc, y)
            self.cfear_class.AddDataPoint(Xf, y)

    def PredAlignment(self, current, prev, quality=None):                # :349-367
        """-> (quality dict, X_CorAl, X_CFEAR); `valid` of the reference is valid1 && valid2 of two locals that
        are never written, i.e. always false, and unused by its callers."""
        quality = {} if quality is None else quality
        Xc, Xf = self._quality(current, prev, [(0.0, 0.0, 0.0)])
        if self.combined_:
            quality[COMBINED_COST] = float(self.combined_class.predict_linear(np.concatenate([Xc[0], Xf[0]]))[0])
        else:
            quality[CORAL_COST] = float(self.coral_class.predict_proba(Xc)[0])
            quality[CFEAR_COST] = float(self.cfear_class.predict_proba(Xf)[0])
        return quality, Xc, Xf

    def _files(self, d, combined_name, coral_name, cfear_name):
        d = str(d)
        if self.combined_:
            return [(self.combined_class, d + combined_name)]
        return [(self.coral_class, d + coral_name), (self.cfear_class, d + cfear_name)]

    def LoadData(self, d):                                               # :376-383
        for clf, f in self._files(d, "/combined.txt", "/CorAl.txt", "/CFEAR.txt"):
            clf.LoadData(f)

    def SaveData(self, d):                                               # :386-393
        for clf, f in self._files(d, "/combined.txt", "/CorAl.txt", "/CFEAR.txt"):
            clf.SaveData(f)

    def LoadCoefficients(self, d):                                       # :396-403 (dir is concatenated without "/")
        for clf, f in self._files(d, "trained_alignment_classifier.txt", "trained_alignment_classifier_CorAl.txt",
                                  "trained_alignment_classifier_CFEAR.txt"):
            clf.LoadCoefficients(f)

    def SaveCoefficients(self, d):                                       # :405-412
        for clf, f in self._files(d, "/trained_alignment_classifier.txt", "/trained_alignment_classifier_CorAl.txt",
                                  "/trained_alignment_classifier_CFEAR.txt"):
            clf.SaveCoefficients(f)

    def FitModels(self, model="LogisticRegression"):                     # :423-434
        for clf, _ in self._files("", "", "", ""):
            clf.fit()

    def FitModelsDevice(self, **params):
        """FitModels on the GPU: the models this interface owns (combined, or CorAl and CFEAR) in one
        cfear_logreg_fit_batch call -> their records."""
        models = [clf for clf, _ in self._files("", "", "", "")]
        for clf in models:
            if not clf.DataValid():
                raise ValueError("training data invalid")
        out = logreg_fit_batch([(clf.X_, clf.y_) for clf in models], self.ctx, **params)
        for clf, r in zip(models, out):
            clf._take_record(r)
        return out

    def verify_params(self, **kw):
        """cfear_verify_params carrying this interface's combined classifier."""
        assert self.combined_ and self.combined_class.IsFit()
        return verify_params(self.ctx, align_intercept=self.combined_class.intercept_,
                             align_coef=list(self.combined_class.coef_), **kw)


def _cloud_ptr(cloud):
    """float32 [n, 4] NumPy array or torch CUDA tensor -> (pointer, n, keep-alive)."""
    if isinstance(cloud, np.ndarray):
        c = np.ascontiguousarray(cloud, dtype=np.float32)
        assert c.ndim == 2 and c.shape[1] == 4
        return c.ctypes.data, c.shape[0], c
    assert cloud.dim() == 2 and cloud.shape[1] == 4 and cloud.is_contiguous()
    return cloud.data_ptr(), int(cloud.shape[0]), cloud


# ------------------------------------------------------------------------------------------------
# replay of a recorded trajectory
# ------------------------------------------------------------------------------------------------
def odometry_replay(clouds, trace, par=None, seq_offsets=None, audit=False, ctx=None):
    """cfear_odometry_replay / cfear_odometry_replay_clouds: every frame registered from the RECORDED pose of the frame before
    it and the recorded keyframe set, as a few batched launches -- no frame's input depends on another frame's result.
    clouds: one float32 [n, 4] array (NumPy or torch CUDA) per frame, the filtered clouds BEFORE compensation, all sequences
    one behind the other -- or ONE uint8 array [frames, rows, cols] of raw sweeps (NumPy or torch CUDA, laid out as
    OdometryKeyframeFuser.process takes them), which go through the filter par selects first; trace: [frames, 3] (x, y,
    theta), another build's, ground truth or OdometryKeyframeFuser's own; seq_offsets: [n_seq + 1] frame offsets of the
    sequences (default: one sequence); audit: fold the tie and voxel-order audits into the records (CFEAR_REPLAY_AUDIT; the
    caveats of include/cfear_hip.h apply), else those fields are -1.  -> a REPLAY_FRAME_DTYPE array [frames].  A frame whose
    cloud is empty carries the status in reg_status, as do the frames whose window holds it; nothing is raised."""
    ctx = ctx or default_context()
    par = par or odometry_params()
    trace = np.ascontiguousarray(trace, dtype=np.float64).reshape(-1, 3)
    n = trace.shape[0]
    flags = L.REPLAY_AUDIT if audit else 0
    if (isinstance(clouds, np.ndarray) or _is_torch(clouds)) and clouds.ndim == 3:      # raw sweeps
        img = clouds if _is_torch(clouds) else np.ascontiguousarray(clouds, dtype=np.uint8)
        d, batch, rows, cols = _desc(img)
        if _is_torch(img):
            import torch
            assert img.dtype == torch.uint8 and img.stride(-1) == 1
            d.stride, d.batch_stride = img.stride(-2), img.stride(0)
        seq = np.ascontiguousarray([0, n] if seq_offsets is None else seq_offsets, dtype=np.int32)
        if seq.ndim != 1 or seq.shape[0] < 2:
            raise ValueError("odometry_replay: seq_offsets holds the sequences' first frames and the number of frames")
        _torch_ready(ctx, img)
        out = np.zeros(n, L.REPLAY_FRAME_DTYPE)
        rc = ctx._lib.cfear_odometry_replay(ctx.h, C.byref(d), _ptr(img)[0], C.byref(par), trace.ctypes.data, seq.ctypes.data,
                                            seq.shape[0] - 1, flags, out.ctypes.data)
        ctx.check(rc, allowed=(L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY))
        return out
    clouds = list(clouds)
    if len(clouds) != n:
        raise ValueError("odometry_replay: %d clouds for %d trace poses" % (len(clouds), n))
    seq = np.ascontiguousarray([0, n] if seq_offsets is None else seq_offsets, dtype=np.int32)
    if seq.ndim != 1 or seq.shape[0] < 2 or seq[-1] != n:
        raise ValueError("odometry_replay: seq_offsets must end at the number of frames")
    arr = (L.ScCloud * max(n, 1))()
    keep = []
    for i, c in enumerate(clouds):
        ptr, m, k = _cloud_ptr(c)
        arr[i].xyzi, arr[i].n = (ptr if m else None), m
        keep.append(k)
    _torch_ready(ctx, *keep)
    out = np.zeros(n, L.REPLAY_FRAME_DTYPE)
    rc = ctx._lib.cfear_odometry_replay_clouds(ctx.h, arr, C.byref(par), trace.ctypes.data, seq.ctypes.data, seq.shape[0] - 1, flags,
                                               out.ctypes.data)
    ctx.check(rc, allowed=(L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY))
    return out


def replay_summary(records, tol_xy, tol_theta, seq_offsets=None):
    """What a replay says about two builds: a frame is EQUAL when |dev| <= (tol_xy, tol_xy, tol_theta), else it DIFFERS; a
    differing frame is `exposed` when the audit flagged it (records["exposed"] > 0: a tie or a voxel order may legally
    decide it) -- without the audit (exposed = -1) every differing frame counts as not exposed.  Frames without a job (the
    first of a sequence, failed scans) are counted apart.  -> dict(n_frames, n_no_job, n_equal, n_differ_exposed,
    n_differ_not_exposed, worst_dev_equal / _differ_exposed / _differ_not_exposed ([3] maxima of |dev|), first_not_exposed:
    per sequence the first frame (index into records) that differs and is not exposed, -1 where none)."""
    r = np.asarray(records)
    n = r.shape[0]
    seq = np.asarray([0, n] if seq_offsets is None else seq_offsets, dtype=np.int64)
    d = np.abs(r["dev"])
    job = r["n_targets"] > 0
    equal = job & (d[:, 0] <= tol_xy) & (d[:, 1] <= tol_xy) & (d[:, 2] <= tol_theta)
    differ = job & ~equal
    exposed = differ & (r["exposed"] > 0)
    hidden = differ & ~exposed

    def worst(mask):
        return d[mask].max(axis=0) if mask.any() else np.zeros(3)
    first = []
    for a, b in zip(seq[:-1], seq[1:]):
        idx = np.flatnonzero(hidden[a:b])
        first.append(int(a + idx[0]) if idx.size else -1)
    return dict(n_frames=int(n), n_no_job=int((~job).sum()), n_equal=int(equal.sum()), n_differ_exposed=int(exposed.sum()),
                n_differ_not_exposed=int(hidden.sum()), worst_dev_equal=worst(equal), worst_dev_differ_exposed=worst(exposed),
                worst_dev_differ_not_exposed=worst(hidden), first_not_exposed=first)


# ------------------------------------------------------------------------------------------------
# radar Scan Context (loop-candidate generation; place_recognition_radar)
# ------------------------------------------------------------------------------------------------
def sc_params(**kw):
    """cfear_sc_params with TBV's defaults (40 x 120, 80 m, search ratio 0.1, sum / 1000)."""
    p = L.ScParams()
    L.lib().cfear_sc_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "desc_function" and isinstance(v, str):
            v = {"sum": 0, "max": 1}[v]
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def sc_descriptors(clouds, par=None, shifts_y=(0.0,), ctx=None, device_out=False):
    """MakeRadarCloudContext (RadarScancontext.cpp:59-131) for a list of clouds and lateral shifts.
    -> (desc [n, A, R, S], ringkey [n, A, R], sectorkey [n, A, S]); with device_out the descriptors stay in HBM
    (torch CUDA float64 tensor, accepted by sc_distance_batch) and only the keys come back to the host."""
    ctx = ctx or default_context()
    par = par or sc_params()
    n, A = len(clouds), len(shifts_y)
    arr = (L.ScCloud * max(n, 1))()
    keep = []
    for i, c in enumerate(clouds):
        ptr, m, k = _cloud_ptr(c)
        keep.append(k)
        arr[i].xyzi, arr[i].n = ptr, m
    R, S = par.num_ring, par.num_sector
    if device_out:
        import torch
        desc = torch.zeros((n, A, R, S), dtype=torch.float64, device="cuda:%d" % ctx.device)
    else:
        desc = np.zeros((n, A, R, S), np.float64)
    rk = np.zeros((n, A, R), np.float64)
    sk = np.zeros((n, A, S), np.float64)
    sh = (C.c_double * A)(*[float(v) for v in shifts_y])
    _torch_ready(ctx, desc, *clouds)
    ctx.check(ctx._lib.cfear_sc_descriptors(ctx.h, arr, n, C.byref(par), sh, A, _ptr(desc)[0], rk.ctypes.data,
                                            sk.ctypes.data))
    return desc, rk, sk


def sc_distance_batch(desc_q, desc_c, pairs, par=None, ctx=None):
    """distanceBtnScanContext (Scancontext.cpp:157-189) for pairs (query index, candidate index).
    desc_q [nq, R, S], desc_c [nc, R, S] float64 -> (dist [n_pairs], argmin_shift [n_pairs])."""
    ctx = ctx or default_context()
    par = par or sc_params()
    q = desc_q.contiguous() if _is_torch(desc_q) else np.ascontiguousarray(desc_q, dtype=np.float64)
    c = desc_c.contiguous() if _is_torch(desc_c) else np.ascontiguousarray(desc_c, dtype=np.float64)
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    dist = np.zeros(pr.shape[0], np.float64)
    shift = np.zeros(pr.shape[0], np.int32)
    if pr.shape[0]:
        _torch_ready(ctx, q, c)
        ctx.check(ctx._lib.cfear_sc_distance_batch(ctx.h, _ptr(q)[0], q.shape[0], _ptr(c)[0], c.shape[0],
                                                   pr.ctypes.data, pr.shape[0], C.byref(par), dist.ctypes.data,
                                                   shift.ctypes.data))
    return dist, shift


def sc_raw_params(**kw):
    """cfear_sc_raw_params with TBV's values (radar_threshold 0, no normalisation, INTER_AREA, an azimuth-major
    sweep read transposed); keyword overrides use the C field names (interpolation also takes "area")."""
    p = L.ScRawParams()
    L.lib().cfear_sc_raw_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "interpolation" and isinstance(v, str):
            v = {"nearest_neighbor": 0, "bilinear": 1, "bicubic": 2, "area": L.SC_INTER_AREA}[v]
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _image_desc(img):
    """PolarDesc of a uint8 [B, H, W] / [H, W] NumPy array or torch tensor whose rows are contiguous (any row and
    batch stride) -> (desc, pointer, keep-alive)."""
    if _is_torch(img):
        assert img.dtype.is_floating_point is False and img.element_size() == 1, "uint8 images"
        st = list(img.stride())
        if st[-1] != 1:
            img = img.contiguous()
            st = list(img.stride())
        ptr = img.data_ptr()
    else:
        if img.dtype != np.uint8:
            raise TypeError("uint8 images")
        if img.strides[-1] != 1:
            img = np.ascontiguousarray(img)
        st = list(img.strides)
        ptr = img.ctypes.data
    shape = tuple(img.shape)
    d = L.PolarDesc()
    d.rows, d.cols = shape[-2], shape[-1]
    d.stride = st[-2]
    d.batch = shape[0] if len(shape) == 3 else 1
    d.batch_stride = st[0] if len(shape) == 3 else d.rows * d.stride
    return d, ptr, img


def sc_raw_descriptors(imgs, par=None, raw=None, ctx=None, device_out=False):
    """MakeRadarContext (RadarScancontext.cpp:41-57) of raw polar sweeps: uint8 [B, H, W] or [H, W], NumPy (host) or torch
    CUDA (device), rows contiguous.  -> (desc [B, R, S] float64, ringkey [B, R], sectorkey [B, S]; [R, S], [R], [S] for
    one 2-D sweep).  raw defaults to TBV's settings with transpose = (H < W), the reader's rule (PNGReaderInterface::Get).
    With device_out the descriptors stay in HBM (torch CUDA tensor); the keys always come back to the host."""
    ctx = ctx or default_context()
    par = par or sc_params()
    if raw is None:
        raw = sc_raw_params(transpose=int(imgs.shape[-2] < imgs.shape[-1]))
    d, ptr, keep = _image_desc(imgs)
    B, R, S = d.batch, par.num_ring, par.num_sector
    if device_out:
        import torch
        desc = torch.zeros((B, R, S), dtype=torch.float64, device="cuda:%d" % ctx.device)
    else:
        desc = np.zeros((B, R, S), np.float64)
    rk = np.zeros((B, R), np.float64)
    sk = np.zeros((B, S), np.float64)
    _torch_ready(ctx, desc, imgs)
    ctx.check(ctx._lib.cfear_sc_raw_descriptors(ctx.h, ptr, C.byref(d), C.byref(par), C.byref(raw), _ptr(desc)[0],
                                                rk.ctypes.data, sk.ctypes.data))
    del keep
    if len(imgs.shape) == 2:
        return desc[0], rk[0], sk[0]
    return desc, rk, sk


class RSCManager:
    """RSCManager (place_recognition_radar RadarScancontext.{h,cpp}) for cloud descriptors: the descriptor
    database, the recent-node exclusion, the odometry similarity and the candidate ranking are host policy
    restated here; descriptors and scan-context distances run on the GPU."""

    DISTANCE_EXCLUDE_RECENT = 10.0                    # Scancontext.h:108
    AUGMENTS_Y = (-2.0, 2.0, -4.0, 4.0)               # RadarScancontext.cpp:164

    def __init__(self, par=None, num_candidates_from_tree=10, n_candidates=3, odom_sigma_error=0.05,
                 odometry_coupled_closure=True, augment_sc=True, ctx=None, raw_par=None):
        self.ctx = ctx
        self.par = par or sc_params()
        self.raw_par = raw_par                        # cfear_sc_raw_params of the raw path; None: the reader's rule per image
        self.NUM_CANDIDATES_FROM_TREE = int(num_candidates_from_tree)
        self.N_candidates = int(n_candidates)
        self.odom_sigma_error = float(odom_sigma_error)
        self.odometry_coupled_closure = bool(odometry_coupled_closure)
        self.augment_sc = bool(augment_sc)
        self.polarcontexts_ = []                      # [R, S] float64 per node (device tensors with the GPU hooks)
        self.polarcontext_invkeys_mat_ = []           # float32 ring keys (eig2stdvec), [R] per node
        self.odom_poses_ = []                         # (x, y, theta)
        self.odom_similarity = np.zeros(0)
        self.NUM_EXCLUDE_RECENT = 0
        self.current_and_augments_ = []               # (desc, ring key float32, (tx, ty, theta) of the augmentation)

    # the two device operations (tests substitute the CPU oracle here to check the host policy around them)
    def _descriptors(self, clouds, shifts):
        return sc_descriptors(clouds, self.par, shifts, self.ctx, device_out=True)   # the database lives in HBM

    def _distances(self, desc_q, desc_c, pairs):
        return sc_distance_batch(desc_q, desc_c, pairs, self.par, self.ctx)

    def _raw_descriptor(self, img):
        return sc_raw_descriptors(img, self.par, self.raw_par, self.ctx, device_out=True)

    def makeAndSaveScancontextAndKeysRadarRaw(self, img, Todom):
        """RadarScancontext.cpp:148-154 (+ :133-146, :181-222): the descriptor of the node's raw sweep [H, W]; the node
        has no lateral augmentations, whatever augment_sc says."""
        desc, rk, _ = self._raw_descriptor(img)
        self.polarcontexts_.append(desc)
        self.polarcontext_invkeys_mat_.append(rk.astype(np.float32))
        self.current_and_augments_ = [(desc, rk.astype(np.float32), (0.0, 0.0, 0.0))]
        self._exclude_and_update_likelihood(np.asarray(Todom, np.float64))

    def makeAndSaveScancontextAndKeysRadarCloud(self, cloud, Todom):
        """RadarScancontext.cpp:156-180 (+ :133-146, :181-225)."""
        shifts = (0.0,) + (self.AUGMENTS_Y if self.augment_sc else ())
        desc, rk, _ = self._descriptors([cloud], shifts)
        self.polarcontexts_.append(desc[0, 0])
        self.polarcontext_invkeys_mat_.append(rk[0, 0].astype(np.float32))
        self.current_and_augments_ = [(desc[0, k], rk[0, k].astype(np.float32), (0.0, float(shifts[k]), 0.0))
                                      for k in range(len(shifts))]
        self._exclude_and_update_likelihood(np.asarray(Todom, np.float64))

    def _exclude_and_update_likelihood(self, Todom):                       # RadarScancontext.cpp:181-222
        self.odom_poses_.append(Todom)
        P = np.asarray(self.odom_poses_)
        if len(P) <= 2:
            self.NUM_EXCLUDE_RECENT = 2
        else:
            distance, n_ex, prev = 0.0, 0, P[-1]
            i = len(P) - 1
            while i >= 0 and distance < self.DISTANCE_EXCLUDE_RECENT:
                distance = distance + float(np.hypot(*(P[i][:2] - prev[:2])))   # |(Tprev^-1 T_i).translation()|
                prev = P[i]
                n_ex += 1
                i -= 1
            self.NUM_EXCLUDE_RECENT = n_ex
        idx_current = len(P) - 1
        self.odom_similarity = np.zeros(idx_current)
        tprev = Todom[:2].copy()
        trav = 0.0
        for i in range(idx_current - 1, -1, -1):
            t_i = P[i][:2]
            trav += float(np.hypot(*(tprev - t_i)))
            tprev = t_i
            est = float(np.hypot(*(Todom[:2] - t_i)))
            error = max(est - 5.0, 0.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.float64(error) / np.float64(trav)
            prob = np.exp(-rel * rel / (2 * self.odom_sigma_error * self.odom_sigma_error))
            self.odom_similarity[i] = 1.0 - prob

    def _odometry_nn_search(self, curr_key):                                # RadarScancontext.cpp:259-284
        key = np.append(curr_key.astype(np.float32), np.float32(0.0))
        idx_current = len(self.polarcontext_invkeys_mat_) - 1
        cands = []
        for idx in range(0, max(idx_current - 1 - self.NUM_EXCLUDE_RECENT, 0)):
            other = np.append(self.polarcontext_invkeys_mat_[idx], np.float32(10 * self.odom_similarity[idx]))
            l2 = np.float32(0.0)                      # `float l2`, err in double (L2norm, :250-257)
            for a_, b_ in zip(key, other):
                err = np.float64(a_ - b_)             # float subtraction promoted to double
                l2 = np.float32(np.float64(l2) + err * err)
            cands.append((float(l2), idx))
        cands.sort()                                  # lower_bound insertion == sort by (distance, index)
        return [i for _, i in cands[:self.NUM_CANDIDATES_FROM_TREE]]

    TREE_MAKING_PERIOD_ = 50                          # Scancontext.h:116

    @staticmethod
    def _l2_adaptor(K, q):
        """nanoflann::L2_Adaptor::evalMetric (the reference's vendored nanoflann.hpp:383-408) in float: groups of four
        squared differences are added among themselves first, then to the running sum; the tail one by one."""
        K = np.asarray(K, np.float32)
        e = K - np.asarray(q, np.float32)[None]
        e2 = e * e
        d = np.zeros(K.shape[0], np.float32)
        g4 = (K.shape[1] // 4) * 4
        for c in range(0, g4, 4):
            d = d + (((e2[:, c] + e2[:, c + 1]) + e2[:, c + 2]) + e2[:, c + 3])
        for c in range(g4, K.shape[1]):
            d = d + e2[:, c]
        return d

    def _vanilla_nn_search(self, curr_key):                                 # RadarScancontext.cpp:225-248
        """The ring-key kd-tree retrieval with the reference's bookkeeping: the tree is rebuilt only on every
        TREE_MAKING_PERIOD_-th CALL (one call per augmentation of every node) from the keys older than the recent-node
        exclusion AT THAT MOMENT, and a tree with fewer points than NUM_CANDIDATES_FROM_TREE leaves the rest of the
        zero-initialised index vector in place (node 0 is then proposed again).  The search itself is exact (nanoflann,
        eps = 0), so a linear scan with the tree's own metric arithmetic returns the same neighbours; equal distances
        come back in index order here, in tree-visiting order there (tests/test_ref_nanoflann.py)."""
        if getattr(self, "_tree_counter", None) is None:
            self._tree_counter, self._tree_keys = 0, np.zeros((0, 0), np.float32)
        if self._tree_counter % self.TREE_MAKING_PERIOD_ == 0:
            n = len(self.polarcontext_invkeys_mat_) - self.NUM_EXCLUDE_RECENT
            self._tree_keys = np.asarray(self.polarcontext_invkeys_mat_[:max(n, 0)], np.float32).copy()
        self._tree_counter += 1
        K = self._tree_keys
        out = [0] * self.NUM_CANDIDATES_FROM_TREE
        if K.shape[0] > 0:
            d = self._l2_adaptor(K, curr_key)
            order = np.argsort(d, kind="stable")[:self.NUM_CANDIDATES_FROM_TREE]
            for j, i in enumerate(order):
                out[j] = int(i)
        return out

    def detectLoopClosureID(self):
        """RadarScancontext.cpp:286-345 -> list of candidates dict(min_dist, min_dist_sc, min_dist_odom,
        yaw_diff_rad, nn_idx, argmin_shift, Taug), closest first."""
        if len(self.polarcontext_invkeys_mat_) < self.NUM_EXCLUDE_RECENT + 1:
            return []
        jobs = []                                     # (query k, candidate idx) in the reference's visiting order
        for k, (_d, rk, _T) in enumerate(self.current_and_augments_):
            idxs = self._odometry_nn_search(rk) if self.odometry_coupled_closure else self._vanilla_nn_search(rk)
            jobs += [(k, i) for i in idxs]
        if not jobs:
            return []
        def stack(xs):
            if _is_torch(xs[0]):
                import torch
                return torch.stack(xs)
            return np.stack(xs)
        qd = stack([d for d, _, _ in self.current_and_augments_])
        uniq = sorted({i for _, i in jobs})
        pos = {i: p for p, i in enumerate(uniq)}
        cd = stack([self.polarcontexts_[i] for i in uniq])
        dist, shift = self._distances(qd, cd, [(k, pos[i]) for k, i in jobs])
        unit = 360.0 / float(self.par.num_sector)
        similar = []
        for (k, i), d_sc, sh in zip(jobs, dist, shift):
            d_odom = float(self.odom_similarity[i]) if self.odometry_coupled_closure else 0.0
            d_tot = float(d_sc) + d_odom if self.odometry_coupled_closure else float(d_sc)
            similar.append(dict(min_dist=d_tot, min_dist_sc=float(d_sc), min_dist_odom=d_odom,
                                # deg2rad(float) (RadarScancontext.cpp:6-9): float degrees, double product, float result
                                yaw_diff_rad=float(np.float32(float(np.float32(sh * unit)) * np.pi / 180.0)), nn_idx=int(i),
                                argmin_shift=int(sh), Taug=self.current_and_augments_[k][2]))
            similar.sort(key=lambda c: c["min_dist"])     # std::sort + erase of the worst (:317-320)
            if len(similar) > self.N_candidates:
                similar.pop()
        return similar


def sc_manager_params(par=None, num_candidates_from_tree=10, n_candidates=3, odom_sigma_error=0.05,
                      odometry_coupled_closure=True, augment_sc=True):
    """cfear_sc_manager_params: TBV's defaults with RSCManager's keyword overrides (par: cfear_sc_params)."""
    p = L.ScManagerParams()
    L.lib().cfear_sc_manager_params_default(C.byref(p))
    if par is not None:
        p.sc = par
    p.num_candidates_from_tree, p.n_candidates = int(num_candidates_from_tree), int(n_candidates)
    p.odom_sigma_error = float(odom_sigma_error)
    p.odometry_coupled_closure, p.augment_sc = int(odometry_coupled_closure), int(augment_sc)
    return p


def _sc_candidates(rows):
    """cfear_sc_candidate records -> RSCManager's candidate dicts, closest first."""
    return [dict(min_dist=float(c["min_dist"]), min_dist_sc=float(c["min_dist_sc"]), min_dist_odom=float(c["min_dist_odom"]),
                 yaw_diff_rad=float(c["yaw_diff_rad"]), nn_idx=int(c["nn_idx"]), argmin_shift=int(c["argmin_shift"]),
                 Taug=tuple(float(v) for v in c["Taug"])) for c in rows]


def sc_node_affines(poses_xyt):
    """Rows 0 and 1 of every node's node -> world matrix and of its inverse, built from (x, y, theta) the way
    examples/loop_closure_demo.py does (transform_cloud of the pose, and of xyt_inverse of the pose): scalar cos / sin
    calls, the inverse's angle negated.  -> (T [n, 8], Tinv [n, 8]) float64, the rows of cfear_sc_node."""
    P = np.asarray(poses_xyt, np.float64).reshape(-1, 3)
    T = np.zeros((P.shape[0], 8))
    Ti = np.zeros((P.shape[0], 8))
    for i, a in enumerate(P):
        c, s = np.cos(a[2]), np.sin(a[2])
        T[i] = (c, -s, 0.0, a[0], s, c, 0.0, a[1])
        inv = np.array([-(c * a[0] + s * a[1]), s * a[0] - c * a[1], -a[2]])       # xyt_inverse
        ci, si = np.cos(inv[2]), np.sin(inv[2])
        Ti[i] = (ci, -si, 0.0, inv[0], si, ci, 0.0, inv[1])
    return T, Ti


def _sc_nodes(clouds, poses_xyt, affines, ids):
    """cfear_sc_node array of clouds (float32 [n, 4] NumPy or torch CUDA) with their matrices -> (array, keep-alive)."""
    T, Ti = affines if affines is not None else sc_node_affines(poses_xyt)
    n = len(clouds)
    if len(T) != n or len(Ti) != n or (ids is not None and len(ids) != n):
        raise ValueError("one pose (or matrix pair) and one id per cloud")
    arr = (L.ScNode * max(n, 1))()
    keep = []
    for i, c in enumerate(clouds):
        ptr, m, k = _cloud_ptr(c)
        keep.append(k)
        arr[i].cloud.xyzi, arr[i].cloud.n = ptr, m
        arr[i].T[:] = [float(v) for v in T[i]]
        arr[i].Tinv[:] = [float(v) for v in Ti[i]]
        arr[i].id = int(ids[i]) if ids is not None else i
    return arr, keep


def sc_local_map_descriptors(clouds, poses_xyt=None, n_aggregate=1, centers=None, par=None, shifts_y=(0.0,), ids=None,
                             affines=None, ctx=None, device_out=False):
    """ScansToLocalMap + MakeRadarCloudContext (loopclosure.cpp:553-591) of the local maps of `centers` (node indices;
    default every node): each node's cloud is in its own frame, merged with the nodes whose id lies within n_aggregate of
    the centre's, on the GPU.  Poses (x, y, theta) or affines = (T, Tinv) [n, 8]; ids default to 0 .. n - 1.
    -> (desc [nc, A, R, S], ringkey [nc, A, R], sectorkey [nc, A, S]), as sc_descriptors of the merged clouds."""
    ctx = ctx or default_context()
    par = par or sc_params()
    arr, keep = _sc_nodes(clouds, poses_xyt, affines, ids)
    ctr = np.ascontiguousarray(np.arange(len(clouds)) if centers is None else centers, dtype=np.int32)
    nc, A, R, S = ctr.shape[0], len(shifts_y), par.num_ring, par.num_sector
    if device_out:
        import torch
        desc = torch.zeros((nc, A, R, S), dtype=torch.float64, device="cuda:%d" % ctx.device)
    else:
        desc = np.zeros((nc, A, R, S), np.float64)
    rk = np.zeros((nc, A, R), np.float64)
    sk = np.zeros((nc, A, S), np.float64)
    sh = (C.c_double * A)(*[float(v) for v in shifts_y])
    _torch_ready(ctx, desc, *clouds)
    ctx.check(ctx._lib.cfear_sc_local_map_descriptors(ctx.h, arr, len(clouds), ctr.ctypes.data, nc, int(n_aggregate), C.byref(par),
                                                      sh, A, _ptr(desc)[0], rk.ctypes.data, sk.ctypes.data))
    del keep
    return desc, rk, sk


def _sc_upload_clouds(clouds, ctx):
    """Host clouds of a whole graph in one host-to-device copy (one torch CUDA tensor, viewed per node): the C-ABI would
    stage every host cloud with a copy of its own.  -> (clouds, keep-alive)."""
    if not clouds or not all(isinstance(c, np.ndarray) for c in clouds):
        return clouds, None
    import torch
    flat = np.concatenate([np.ascontiguousarray(c, np.float32).reshape(-1, 4) for c in clouds])
    dev = torch.from_numpy(flat).to("cuda:%d" % ctx.device)
    torch.cuda.current_stream(dev.device).synchronize()             # the library enqueues on its own stream
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])])
    return [dev[off[i]:off[i + 1]] for i in range(len(clouds))], dev


def sc_detect_sequence(clouds, poses_xyt=None, n_aggregate=1, n_detect=None, ids=None, affines=None, par=None, ctx=None,
                       upload_clouds=True, **manager_kw):
    """Scan Context candidate proposal for a whole graph in one call (cfear_sc_detect_sequence): what RSCManagerNative
    returns when nodes 0 .. n_detect - 1 (default: every node) are added in order with their local maps (n_aggregate) and
    poses, each detected right after it is added.  Clouds: float32 [n, 4] NumPy (uploaded together unless upload_clouds is
    False) or torch CUDA.  manager_kw: RSCManagerNative's keywords (num_candidates_from_tree, n_candidates,
    odom_sigma_error, odometry_coupled_closure, augment_sc).  -> one list of candidate dicts per node."""
    ctx = ctx or default_context()
    p = sc_manager_params(par, **manager_kw)
    if upload_clouds:
        clouds, _dev = _sc_upload_clouds(clouds, ctx)
    arr, keep = _sc_nodes(clouds, poses_xyt, affines, ids)
    n = len(clouds)
    nd = n if n_detect is None else int(n_detect)
    out = np.zeros((max(nd, 1), max(int(p.n_candidates), 1)), L.SC_CANDIDATE_DTYPE)
    n_out = np.zeros(max(nd, 1), np.int32)
    ctx.check(ctx._lib.cfear_sc_detect_sequence(ctx.h, C.byref(p), arr, n, int(n_aggregate), nd, out.ctypes.data,
                                                n_out.ctypes.data))
    del keep
    return [_sc_candidates(out[i, :n_out[i]]) for i in range(nd)]


def _is_u8(x):
    return str(getattr(x, "dtype", "")).endswith("uint8")


def sc_flatten_graphs(graphs, ids=None):
    """The flat tables of cfear_sc_batch from one (clouds, poses) or (sweeps, poses) pair per graph, built with NumPy: clouds
    are float32 [m, 4] arrays (NumPy or torch CUDA, one per node), sweeps one uint8 [n, H, W] array or a list of [H, W]
    ones; poses [n, 3] (x, y, theta).  ids: one array per graph (default 0, 1, ... in each).
    -> dict(node_off, T, Tinv, ids, and xyzi + point_off or imgs), what sc_detect_batch takes as flat=."""
    sizes = [len(g[1]) for g in graphs]
    flat = dict(node_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    poses = np.concatenate([np.zeros((0, 3))] + [np.asarray(g[1], np.float64).reshape(-1, 3) for g in graphs])
    flat["T"], flat["Tinv"] = sc_node_affines(poses)
    flat["ids"] = None if ids is None else np.concatenate([np.zeros(0, np.int32)] + [np.asarray(i, np.int32) for i in ids])
    data = [g[0] for g, n in zip(graphs, sizes) if n > 0]
    for d, n in zip(data, [n for n in sizes if n > 0]):
        if len(d) != n:
            raise ValueError("one pose per cloud or sweep")
    if data and (_is_u8(data[0]) or _is_u8(data[0][0])):
        host = isinstance(data[0] if _is_u8(data[0]) else data[0][0], np.ndarray)
        if not host:
            import torch
        data = [d if _is_u8(d) else (np.stack(d) if host else torch.stack(list(d))) for d in data]
        flat["imgs"] = data[0] if len(data) == 1 else (np.concatenate(data) if host else torch.cat(data))
        return flat
    clouds = [c for d in data for c in d]
    flat["point_off"] = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    if all(isinstance(c, np.ndarray) for c in clouds):
        flat["xyzi"] = np.concatenate([np.zeros((0, 4), np.float32)] + [np.asarray(c, np.float32).reshape(-1, 4) for c in clouds])
    else:
        import torch
        flat["xyzi"] = torch.cat([c.reshape(-1, 4) for c in clouds])
    return flat


def sc_detect_batch(graphs=None, n_aggregate=1, n_detect=None, ids=None, par=None, raw_par=None, ctx=None, device_out=False,
                    flat=None, records=False, **manager_kw):
    """Scan Context candidate proposal for a batch of graphs in one call (cfear_sc_detect_batch): for every graph what a fresh
    RSCManagerNative returns when the graph's nodes 0 .. n_detect[g] - 1 (default: all) are added in order -- with their
    local maps (n_aggregate) in cloud mode, with their raw sweeps in raw mode -- each detected right after it is added.
    graphs: see sc_flatten_graphs; or flat = its result (pre-flattened arrays; host clouds cross in ONE copy).  raw_par:
    cfear_sc_raw_params of raw mode (default: an azimuth-major sweep, transpose = 1).  manager_kw: as sc_detect_sequence.
    -> one list per graph of per-node candidate lists (nn_idx counts within the graph); with device_out the record tensor
    (torch CUDA uint8 [nodes, n_candidates, 64], viewable as _lib.SC_CANDIDATE_DTYPE on the host), the counts (torch CUDA
    int32 [nodes]) and the first row of every graph (NumPy [graphs + 1]); with records the same three on the host (the
    records as a _lib.SC_CANDIDATE_DTYPE array [nodes, n_candidates])."""
    ctx = ctx or default_context()
    p = sc_manager_params(par, **manager_kw)
    if flat is None:
        flat = sc_flatten_graphs(graphs, ids)
    node_off = np.ascontiguousarray(flat["node_off"], np.int32)
    G, N = node_off.shape[0] - 1, int(node_off[-1])
    nd = np.diff(node_off).astype(np.int32) if n_detect is None else np.ascontiguousarray(n_detect, np.int32)
    T = np.ascontiguousarray(flat["T"], np.float64)
    b = L.ScBatch()
    b.n_graphs, b.node_off, b.n_detect, b.T = G, node_off.ctypes.data, nd.ctypes.data, T.ctypes.data
    keep = [T]
    if flat.get("ids") is not None:
        keep.append(np.ascontiguousarray(flat["ids"], np.int32))
        b.ids = keep[-1].ctypes.data
    if "imgs" in flat:
        b.mode = L.SC_NODES_RAW
        raw = raw_par if raw_par is not None else sc_raw_params(transpose=1)
        d, ptr, k = _image_desc(flat["imgs"])
        if len(flat["imgs"].shape) == 2:
            d.batch = 1
        keep += [raw, d, k]
        b.imgs, b.desc, b.raw = ptr, C.pointer(d), C.pointer(raw)
        dev_in = [flat["imgs"]]
    else:
        b.mode, b.n_aggregate = L.SC_NODES_CLOUD, int(n_aggregate)
        Ti = np.ascontiguousarray(flat["Tinv"], np.float64)
        po = np.ascontiguousarray(flat["point_off"], np.int64)
        xyzi = flat["xyzi"] if _is_torch(flat["xyzi"]) else np.ascontiguousarray(flat["xyzi"], np.float32)
        keep += [Ti, po, xyzi]
        b.Tinv, b.point_off, b.xyzi = Ti.ctypes.data, po.ctypes.data, _ptr(xyzi)[0]
        dev_in = [xyzi]
    if nd.shape[0] != G:
        raise ValueError("one n_detect per graph")
    D, nc = int(nd.sum()), max(int(p.n_candidates), 1)
    if device_out:
        import torch
        out = torch.zeros((max(D, 1), nc, 64), dtype=torch.uint8, device="cuda:%d" % ctx.device)
        n_out = torch.zeros(max(D, 1), dtype=torch.int32, device=out.device)
    else:
        out = np.zeros((max(D, 1), nc), L.SC_CANDIDATE_DTYPE)
        n_out = np.zeros(max(D, 1), np.int32)
    _torch_ready(ctx, out, n_out, *dev_in)
    ctx.check(ctx._lib.cfear_sc_detect_batch(ctx.h, C.byref(p), C.byref(b), _ptr(out)[0], _ptr(n_out)[0]))
    del keep
    row_off = np.concatenate([[0], np.cumsum(nd)])
    if device_out or records:
        return out[:D], n_out[:D], row_off
    return [[_sc_candidates(out[i, :n_out[i]]) for i in range(row_off[g], row_off[g + 1])] for g in range(G)]


class RSCManagerNative:
    """The same manager as a library object (cfear_sc_manager_*): database in HBM, policy in the library's C++.
    Same two calls as RSCManager; what a C++ host uses (include/cfear_hip.hpp)."""

    def __init__(self, par=None, num_candidates_from_tree=10, n_candidates=3, odom_sigma_error=0.05,
                 odometry_coupled_closure=True, augment_sc=True, ctx=None, raw_par=None):
        self.ctx = ctx or default_context()
        self.raw_par = raw_par
        p = sc_manager_params(par, num_candidates_from_tree, n_candidates, odom_sigma_error, odometry_coupled_closure, augment_sc)
        self.par = p
        self._h = C.c_void_p()
        self.ctx.check(self.ctx._lib.cfear_sc_manager_create(self.ctx.h, C.byref(p), C.byref(self._h)))

    def makeAndSaveScancontextAndKeysRadarCloud(self, cloud, Todom):
        ptr, n, _keep = _cloud_ptr(cloud)
        T = (C.c_double * 3)(*[float(v) for v in Todom])
        self.ctx.check(self.ctx._lib.cfear_sc_manager_add(self._h, ptr, n, T))

    def makeAndSaveScancontextAndKeysRadarRaw(self, img, Todom):
        if len(img.shape) != 2:
            raise ValueError("one sweep [H, W]")
        raw = self.raw_par if self.raw_par is not None else sc_raw_params(transpose=int(img.shape[0] < img.shape[1]))
        d, ptr, _keep = _image_desc(img)
        T = (C.c_double * 3)(*[float(v) for v in Todom])
        self.ctx.check(self.ctx._lib.cfear_sc_manager_add_raw(self._h, ptr, C.byref(d), C.byref(raw), T))

    def detectLoopClosureID(self):
        out = np.zeros(max(int(self.par.n_candidates), 1), L.SC_CANDIDATE_DTYPE)
        n = C.c_int32()
        self.ctx.check(self.ctx._lib.cfear_sc_manager_detect(self._h, out.ctypes.data, out.shape[0], C.byref(n)))
        return _sc_candidates(out[:n.value])

    def size(self):
        return self.ctx._lib.cfear_sc_manager_size(self._h)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "h", None):              # the context may already be gone at interpreter exit: its
                self.ctx._lib.cfear_sc_manager_destroy(self._h)   # objects died with it, destroying them again would be a use after free
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def odometry_params(**kw):
    """cfear_odometry_params with the CFEAR-3 / Oxford preset; keyword overrides use the C field names
    (nested: kstrong_k_strongest, cacfar_window_size, reg_cost, cov_sampling_xy_range, ...)."""
    p = L.OdometryParams()
    L.lib().cfear_odometry_params_default(C.byref(p))
    return _override_odometry_params(p, kw)


def _override_odometry_params(p, kw):
    for k, v in kw.items():
        for prefix, sub in (("kstrong_", p.kstrong), ("cacfar_", p.cacfar), ("reg_", p.reg),
                            ("cov_sampling_", p.cov_sampling)):
            if k.startswith(prefix) and hasattr(sub, k[len(prefix):]):
                setattr(sub, k[len(prefix):], v)
                break
        else:
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
    return p


class EvalTrajectory:
    """The KITTI-style trajectory text of the reference's evaluation (EvalTrajectory::Write, eval_trajectory.cpp:169-183;
    MatToString, types.cpp:64-73): one pose per line, the top three rows of the 4 x 4 matrix, std::fixed (6 decimals).

    An instance is the reference's collector (eval_trajectory.h:70-184): the Callback*Eigen methods append stamped poses,
    Save() synchronises the two vectors by time (One2OneCorrespondance through sync_trajectories) and writes the five files
    of EvalTrajectory::Save (:265-315).  A stamped pose is (pose, cov, t): a KITTI row [12] (or a 3 x 4 / 4 x 4 matrix),
    a 6 x 6 covariance or None (zeros), and the stamp in nanoseconds (ros::Time::toNSec())."""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self.est_vek, self.gt_vek = [], []

    @staticmethod
    def _stamped(p):
        pose, cov, t = p
        pose = np.asarray(pose, np.float64)
        pose = pose.reshape(-1)[:12].copy() if pose.size in (12, 16) else None
        if pose is None:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "a pose is a KITTI row [12], or a 3 x 4 or 4 x 4 matrix")
        cov = np.zeros(36) if cov is None else np.asarray(cov, np.float64).reshape(36).copy()
        return pose, cov, int(t)

    def CallbackEigen(self, Test, Tgt):
        self.CallbackESTEigen(Test)
        self.CallbackGTEigen(Tgt)

    def CallbackGTEigen(self, Tgt):
        self.gt_vek.append(self._stamped(Tgt))

    def CallbackESTEigen(self, Test):
        self.est_vek.append(self._stamped(Test))

    def GetSize(self):
        return min(len(self.gt_vek), len(self.est_vek))

    def GetGtVek(self):
        """-> [(stamp ns, (x, y, theta))]: the pairs AddGroundTruth of the C++ mirror takes; the poses are loop_stats' gt_xyt.
        After Save() the vector is the interpolated one, so its stamps are the estimate's (offline_odometry.cpp:134-137)."""
        return [(t, (p[3], p[7], math.atan2(p[4], p[0]))) for p, _, t in self.gt_vek]

    @staticmethod
    def _arrays(vek):
        n = len(vek)
        return (np.array([p for p, _, _ in vek], np.float64).reshape(n, 12), np.array([c for _, c, _ in vek], np.float64).reshape(n, 36),
                np.array([t for _, _, t in vek], np.int64))

    def Interpolate(self, t):
        """Interpolate(t, Tinterpolated) (eval_trajectory.h:141-144): -> (found, (pose, cov, t)); the search starts from the
        first ground-truth pose, and the covariance is that of the pose before t (:455)."""
        gt, cov, gs = self._arrays(self.gt_vek)
        r = sync_trajectories(None, [np.array([t], np.int64)], [gt], [gs], mode="independent", ctx=self.ctx)
        if r.counts[0] == 0:
            return False, None
        return True, (r.gt[0].copy(), cov[r.rows["gt_index"][0]].copy(), int(t))

    def Save(self, est_dir, gt_dir, name):
        """EvalTrajectory::Save (:265-315): est_dir/name, est_dir/tum_name, est_dir/cov_name and, with a ground truth,
        gt_dir/name and gt_dir/tum_name, after One2OneCorrespondance -- which also replaces the two vectors by the
        synchronised ones.  -> the paths written."""
        if not self.est_vek and not self.gt_vek:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "Nothing to evaluate")
        est, cov, es = self._arrays(self.est_vek)
        gt, gcov, gs = self._arrays(self.gt_vek)
        if len(self.gt_vek):
            r = sync_trajectories([est], [es], [gt], [gs], mode="chained", ctx=self.ctx)
            n = int(r.counts[0])
            rows = r.rows[:n]
            est, cov, es = r.est[:n], cov[rows["est_index"]], r.stamps[:n]
            gt, gcov = r.gt[:n], gcov[rows["gt_index"]]
            self.est_vek = [(est[i].copy(), cov[i].copy(), int(es[i])) for i in range(n)]
            self.gt_vek = [(gt[i].copy(), gcov[i].copy(), int(es[i])) for i in range(n)]
        written = []
        os.makedirs(est_dir, exist_ok=True)
        if len(gs):
            os.makedirs(gt_dir, exist_ok=True)
            written += [os.path.join(gt_dir, name), os.path.join(gt_dir, "tum_" + name)]
            kitti_write(written[0], gt)
            tum_write(written[1], gt, es)
        paths = [os.path.join(est_dir, name), os.path.join(est_dir, "tum_" + name), os.path.join(est_dir, "cov_" + name)]
        kitti_write(paths[0], est)
        tum_write(paths[1], est, es)
        cov_write(paths[2], cov, es)
        return written + paths

    @staticmethod
    def MatToString(pose):
        x, y, th = (float(v) for v in pose)
        c, s = np.cos(th), np.sin(th)
        m = (c, -s, 0.0, x, s, c, 0.0, y, 0.0, 0.0, 1.0, 0.0)
        return " ".join("%f" % v for v in m)

    @staticmethod
    def Write(path, poses):
        with open(path, "w") as f:
            for p in np.asarray(poses, np.float64).reshape(-1, 3):
                f.write(EvalTrajectory.MatToString(p) + "\n")

    @staticmethod
    def Read(path):
        """-> poses [n, 3] (x, y, theta) of a planar trajectory file."""
        a = np.loadtxt(path, dtype=np.float64, ndmin=2)
        assert a.shape[1] == 12
        return np.stack([a[:, 3], a[:, 7], np.arctan2(a[:, 4], a[:, 0])], 1)


PRESETS = {"CFEAR-1": 1, "CFEAR-2": 2, "CFEAR-3": 3, "CFEAR-3-s10": 4}
DATASETS = {"oxford": 0, "mulran": 1, "kvarntorp": 2, "volvo": 3}


def odometry_preset(preset="CFEAR-3", dataset="oxford", **kw):
    """cfear_odometry_params of one of the reference's shipped configurations (launch/oxford/eval/params/baseline/
    oxford_cfear-{1,2,3,3-s10}) on one of its sensor setups (tbv_slam/script/*/run_tbv_simple.sh); keyword overrides
    as in odometry_params.  Non-Oxford datasets expect [range bins][azimuths] images (rotate_ccw)."""
    p = L.OdometryParams()
    rc = L.lib().cfear_odometry_params_preset(C.byref(p), PRESETS[preset], DATASETS[dataset.lower()])
    if rc != L.OK:
        raise L.CfearError(rc, "unknown preset / dataset")
    return _override_odometry_params(p, kw)


class OdometryKeyframeFuser:
    """n_streams independent radarDriver + OdometryKeyframeFuser pairs advanced one frame per call
    (radar_driver.cpp:163-176 + odometrykeyframefuser.cpp:143-259), everything on the GPU."""

    def __init__(self, n_streams, rows, cols, par=None, ctx=None):
        """rows x cols: the layout of the images passed to process() -- azimuths x range bins, or range bins x
        azimuths when par.rotate_ccw is set (non-Oxford drivers, radar_driver.cpp:74-90)."""
        self.ctx = ctx or default_context()
        self.par = par or odometry_params()
        d = L.PolarDesc()
        d.rows, d.cols, d.stride, d.batch = rows, cols, cols, n_streams
        d.batch_stride = rows * cols
        self.n_streams = n_streams
        self._h = C.c_void_p()
        self.ctx.check(self.ctx._lib.cfear_odometry_create(self.ctx.h, n_streams, C.byref(d), C.byref(self.par),
                                                           C.byref(self._h)))
        self._info = np.zeros(n_streams, L.FRAMEINFO_DTYPE)

    def process(self, polar, polar_next=None):
        """polar: uint8 [n_streams, rows, cols] (NumPy or torch CUDA).  Returns a FRAMEINFO_DTYPE array.
        polar_next (optional): the NEXT frame's images; their filter is enqueued behind this frame's
        kernels so the GPU works while the host applies this frame's keyframe policy.  The next call
        must pass that same buffer as `polar`."""
        self._keep = (polar, polar_next)
        # per-stream failures (an empty sweep, a capacity overflow) are results, not exceptions: the other streams
        # have advanced and their info is filled in -- inspect info["reg_status"]
        self._info[:] = 0
        return self._done(self.ctx._lib.cfear_odometry_process_prefetch(self._h, _ptr(polar)[0], _ptr(polar_next)[0],
                                                                        self._info.ctypes.data))

    _PER_STREAM = (L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY)

    def _done(self, rc):
        """A status that some stream reports as its own (info.reg_status) is that stream's result; anything else is a
        failed call."""
        if rc in self._PER_STREAM and (self._info["reg_status"] == rc).any():
            return self._info.copy()
        self.ctx.check(rc)
        return self._info.copy()

    def process_offsets(self, base, offsets, offsets_next=None):
        """The same step for sweeps that do not sit at a constant stride: stream b's image starts `offsets[b]` bytes
        into the device buffer `base` (a ring of frames, one buffer per sequence).  offsets / offsets_next: int64
        [n_streams].  offsets_next prefetches the next frame's filter; pass the same values as `offsets` next time."""
        self._keep = (base,)
        o = np.ascontiguousarray(offsets, np.int64)
        on = None if offsets_next is None else np.ascontiguousarray(offsets_next, np.int64)
        assert o.shape == (self.n_streams,) and (on is None or on.shape == o.shape)
        self._info[:] = 0
        return self._done(self.ctx._lib.cfear_odometry_process_offsets(self._h, _ptr(base)[0], o.ctypes.data,
                                                                       None if on is None else on.ctypes.data,
                                                                       self._info.ctypes.data))

    def discard_prefetch(self):
        """Forget a prefetched filter output (call before REUSING an image buffer for different content)."""
        self.ctx.check(self.ctx._lib.cfear_odometry_discard_prefetch(self._h))

    def process_clouds(self, clouds, peaks=None):
        """pointcloudCallback(cloud, cloud_peaks, ...) (odometrykeyframefuser.cpp:413-426) for every stream: the caller's
        driver has filtered the sweeps already.  clouds / peaks: one float32 [n, 4] array (NumPy or torch CUDA) per
        stream; peaks are kept only with par.keep_nodes.  Returns a FRAMEINFO_DTYPE array."""
        def pack(lst):
            arr = (L.ScCloud * self.n_streams)()
            keep = []
            for i, c in enumerate(lst):
                ptr, n, k = _cloud_ptr(c)
                arr[i].xyzi, arr[i].n = ptr, n
                keep.append(k)
            return arr, keep
        assert len(clouds) == self.n_streams and (peaks is None or len(peaks) == self.n_streams)
        ca, k1 = pack(clouds)
        pa, k2 = pack(peaks) if peaks is not None else (None, None)
        self._info[:] = 0
        return self._done(self.ctx._lib.cfear_odometry_process_clouds(self._h, ca, pa, self._info.ctypes.data))

    def node(self, stream, device=False):
        """The RadarScan of `stream`'s last processed frame (scan_, odometrykeyframefuser.cpp:172, 244; types.h:119-122)
        -> dict(scan=MapPointNormal copy of cloud_normal_, cloud=cloud_nopeaks_, peaks=cloud_peaks_ (par.keep_nodes)).
        Clouds are NumPy arrays, or torch CUDA tensors with device=True.  Valid until the next process()."""
        lib = self.ctx._lib
        h = C.c_void_p()
        self.ctx.check(lib.cfear_odometry_get_scan(self._h, int(stream), C.byref(h)))
        out = {"scan": MapPointNormal._from_handle(h, self.ctx)}
        for name, fn in (("cloud", lib.cfear_odometry_get_cloud), ("peaks", lib.cfear_odometry_get_peaks)):
            if name == "peaks" and not self.par.keep_nodes:
                continue
            n = C.c_int32()
            self.ctx.check(fn(self._h, int(stream), None, 0, C.byref(n)))
            if device:
                import torch
                buf = torch.empty((n.value, 4), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
            else:
                buf = np.empty((n.value, 4), np.float32)
            if n.value:
                self.ctx.check(fn(self._h, int(stream), _ptr(buf)[0], n.value, C.byref(n)))
            out[name] = buf
        return out

    def constraint(self, stream):
        """OdometryKeyframeFuser::AddToGraph (odometrykeyframefuser.cpp:428-445): the odometry Constraint3d from the keyframe
        the last frame added to the keyframe before it -> dict (SaveSimpleGraph layout), or None if the last frame added
        no keyframe (or the first one)."""
        c = L.GraphConstraint()
        rc = self.ctx._lib.cfear_odometry_get_constraint(self._h, int(stream), C.byref(c))
        if rc == L.ERR_INVALID_ARGUMENT:
            return None
        self.ctx.check(rc)
        return dict(id_begin=int(c.id_begin), id_end=int(c.id_end), t_be=np.array(list(c.t_be.p) + list(c.t_be.q)),
                    information=np.array(c.information).reshape(6, 6), type=int(c.type), quality={}, info="")

    def covariance(self):
        """cov_current of every stream after the last frame -> (cov [n_streams,6,6], sampled [n_streams] bool):
        Register's constant diagonal, Identity after a failed registration, or the sampled covariance when
        par.estimate_cov_by_sampling is set (odometrykeyframefuser.cpp:196, 203-208)."""
        cov = np.zeros((self.n_streams, 6, 6), np.float64)
        flag = np.zeros(self.n_streams, np.int32)
        self.ctx.check(self.ctx._lib.cfear_odometry_get_covariance(self._h, cov.ctypes.data, flag.ctypes.data))
        return cov, flag.astype(bool)

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "h", None):              # the context may already be gone at interpreter exit: its
                self.ctx._lib.cfear_odometry_destroy(self._h)   # objects died with it, destroying them again would be a use after free
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- a parameter grid of odometry streams as one batch ---------------------------------------------------------
def kstrong_rowkeys_derive(sel_range, sel_intensity, sel_count, classes, z_min_sup, ctx=None):
    """cfear_kstrong_rowkeys_derive: the row keys of several k-strongest parameter sets from the sel_* lists of ONE sweep
    (filter_kstrongest on torch CUDA images at (k_sup, z_min_sup), k_sup <= 64).  sel_range int32 / sel_intensity uint8
    [n_images, rows, k_sup], sel_count int32 [n_images, rows]; classes: (image, k, z_min, range_res, min_distance) each.
    Returns (row_keys uint32-as-int32 [n_classes, rows, 64], row_counts int32 [n_classes, rows, 2]) as CUDA tensors: what
    filter_kstrongest_rowkeys gives image `image` with the class's own parameters, at a row stride of 64."""
    import torch
    ctx = ctx or default_context()
    n_images, rows, k_sup = sel_range.shape
    arr = (L.RowkeysClass * max(len(classes), 1))()
    for i, (image, k, z_min, range_res, min_distance) in enumerate(classes):
        arr[i] = L.RowkeysClass(int(image), int(k), float(z_min), float(range_res), float(min_distance))
    keys = torch.zeros((len(classes), rows, 64), dtype=torch.int32, device=sel_range.device)
    cnt = torch.zeros((len(classes), rows, 2), dtype=torch.int32, device=sel_range.device)
    ctx.check(ctx._lib.cfear_kstrong_rowkeys_derive(ctx.h, _ptr(sel_range)[0], _ptr(sel_intensity)[0], _ptr(sel_count)[0], n_images, rows,
                                                    k_sup, float(z_min_sup), arr, len(classes), _ptr(keys)[0], _ptr(cnt)[0]))
    return keys, cnt


def odometry_grid_configs(preset="CFEAR-3", dataset="oxford", **lists):
    """The configurations of a parameter grid: the product of the keyword lists (names as in odometry_params) over
    odometry_preset(preset, dataset), last keyword fastest -- the order of the reference's grid_search loops when the
    keywords are given in its order.  A scalar is a list of one."""
    import itertools
    names = list(lists)
    values = [list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] for v in lists.values()]
    return [odometry_preset(preset, dataset, **dict(zip(names, combo))) for combo in itertools.product(*values)]


def _grid_args(rows, cols, configs, n_sequences, stream_sequence, stream_config):
    d = L.PolarDesc()
    d.rows, d.cols, d.stride, d.batch = int(rows), int(cols), int(cols), int(n_sequences)
    d.batch_stride = int(rows) * int(cols)
    arr = (L.OdometryParams * max(len(configs), 1))()
    for i, p in enumerate(configs):
        C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(L.OdometryParams))
    sq = None if stream_sequence is None else np.ascontiguousarray(stream_sequence, np.int32)
    sc = None if stream_config is None else np.ascontiguousarray(stream_config, np.int32)
    assert sq is None or sc is None or sq.shape == sc.shape
    n = len(configs) * int(n_sequences) if sq is None and sc is None else len(sq if sq is not None else sc)
    return d, arr, sq, sc, n


def odometry_grid_plan(rows, cols, configs, n_sequences, stream_sequence=None, stream_config=None, n_streams=None):
    """cfear_odometry_grid_plan: how OdometryGrid groups its streams, as dict(streams=GRID_STREAM_DTYPE array, totals=dict).
    Host code only: needs no GPU and no context.  Raises CfearError with the refusal's reason."""
    d, arr, sq, sc, n = _grid_args(rows, cols, configs, n_sequences, stream_sequence, stream_config)
    n = n if n_streams is None else int(n_streams)
    streams = np.zeros(max(n, 1), L.GRID_STREAM_DTYPE)
    totals = L.GridTotals()
    why = C.create_string_buffer(256)
    rc = L.lib().cfear_odometry_grid_plan(C.byref(d), arr, len(configs), None if sq is None else sq.ctypes.data,
                                          None if sc is None else sc.ctypes.data, n, streams.ctypes.data, C.byref(totals), why, 256)
    if rc != L.OK:
        raise L.CfearError(rc, why.value.decode())
    return dict(streams=streams[:n], totals={name: int(getattr(totals, name)) for name, _ in L.GridTotals._fields_})


class OdometryGrid:
    """A parameter grid of odometry streams advanced one frame per call (the reference's grid_search / loss_function
    evaluations: one job per (sequence, configuration)).  Stream s runs configs[stream_config[s]] on the images of sequence
    stream_sequence[s]; with both None the streams are the full product, sequence-major and configuration fastest.  Per
    stream the results are those of an OdometryKeyframeFuser with that configuration; the polar sweep runs once per sequence
    image, the surface and matcher stages once per group of equal parameters (odometry_grid_plan)."""

    def __init__(self, rows, cols, configs, n_sequences, stream_sequence=None, stream_config=None, ctx=None):
        self.ctx = ctx or default_context()
        d, arr, sq, sc, n = _grid_args(rows, cols, configs, n_sequences, stream_sequence, stream_config)
        self.configs = list(configs)
        self.n_streams, self.n_sequences = n, int(n_sequences)
        self._h = C.c_void_p()
        self.ctx.check(self.ctx._lib.cfear_odometry_grid_create(self.ctx.h, C.byref(d), arr, len(configs),
                                                                None if sq is None else sq.ctypes.data,
                                                                None if sc is None else sc.ctypes.data, n, C.byref(self._h)))
        self.stream_sequence = np.repeat(np.arange(n_sequences), len(configs)) if sq is None else sq
        self.stream_config = np.tile(np.arange(len(configs)), n_sequences) if sc is None else sc
        self._info = np.zeros(n, L.FRAMEINFO_DTYPE)

    _PER_STREAM = (L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY)

    def process(self, polar):
        """polar: uint8 [n_sequences, rows, cols] (NumPy or torch CUDA).  Returns a FRAMEINFO_DTYPE array [n_streams]; a
        stream's own failure (an empty sweep, a capacity overflow) is its info["reg_status"], not an exception."""
        self._keep = polar
        self._info[:] = 0
        rc = self.ctx._lib.cfear_odometry_grid_process(self._h, _ptr(polar)[0], self._info.ctypes.data)
        if not (rc in self._PER_STREAM and (self._info["reg_status"] == rc).any()):
            self.ctx.check(rc)
        return self._info.copy()

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "h", None):
                self.ctx._lib.cfear_odometry_grid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- simple_graph.sgh (types.cpp:103-130): host-only, no GPU ---------------------------------------------------
def pose3d_from_xyt(xyt):
    """PoseEigToCeres of a planar pose -> (p [3], q [4] = x, y, z, w)."""
    p = L.Pose3d()
    L.lib().cfear_pose3d_from_xyt((C.c_double * 3)(*[float(v) for v in xyt]), C.byref(p))
    return np.array(p.p), np.array(p.q)


def _pose3d(v):
    p = L.Pose3d()
    if v is None:
        p.q[3] = 1.0
    elif len(v) == 3:
        L.lib().cfear_pose3d_from_xyt((C.c_double * 3)(*[float(x) for x in v]), C.byref(p))
    else:
        for i in range(3):
            p.p[i] = float(v[i])
        for i in range(4):
            p.q[i] = float(v[3 + i])
    return p


def _graph_cloud(c, keep):
    g = L.GraphCloud()
    if c is None:
        g.n = -1
        return g
    xyzi = c if not isinstance(c, dict) else c["xyzi"]
    a = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    keep.append(a)
    g.xyzi, g.n = a.ctypes.data, a.shape[0]
    if isinstance(c, dict):
        g.seq, g.stamp = int(c.get("seq", 0)), int(c.get("stamp", 0))
        fid = c.get("frame_id", "").encode()
        keep.append(fid)
        g.frame_id = fid
    return g


def SaveSimpleGraph(path, nodes):
    """SaveSimpleGraph (types.cpp:103-113).  nodes: list of dicts with keys T, Tgt (xyt or p+q 7-vectors), has_Tgt, idx,
    stamp, motion (4x4), cloud_peaks, cloud_nopeaks (float [n, 4] or dict(xyzi, stamp, seq, frame_id) or None), cells
    (CELL_DTYPE array or None), radius, weight_intensity, input_is_nopeaks (default True), normal_input, constraints
    (list of dicts: id_begin, id_end, t_be, information [6, 6], type, quality {str: float}, info)."""
    keep = []
    arr = (L.GraphNode * len(nodes))()
    for i, nd in enumerate(nodes):
        g = arr[i]
        g.T, g.Tgt = _pose3d(nd.get("T")), _pose3d(nd.get("Tgt"))
        g.has_Tgt, g.idx, g.stamp = int(nd.get("has_Tgt", 0)), int(nd.get("idx", i)), int(nd.get("stamp", 0))
        m = np.asarray(nd.get("motion", np.eye(4)), np.float64).reshape(4, 4)
        for k, v in enumerate(m.T.reshape(-1)):                       # Affine3d::data() is column-major
            g.motion[k] = float(v)
        g.cloud_peaks = _graph_cloud(nd.get("cloud_peaks"), keep)
        g.cloud_nopeaks = _graph_cloud(nd.get("cloud_nopeaks"), keep)
        g.normal_input = _graph_cloud(nd.get("normal_input"), keep)
        cells = nd.get("cells")
        g.has_normal = int(cells is not None)
        g.input_is_nopeaks = int(nd.get("input_is_nopeaks", True))
        if cells is not None:
            ca = np.ascontiguousarray(cells, L.CELL_DTYPE)
            keep.append(ca)
            g.cells, g.n_cells = ca.ctypes.data, ca.shape[0]
        g.radius, g.weight_intensity = float(nd.get("radius", 0.0)), int(nd.get("weight_intensity", 0))
        cons = nd.get("constraints", [])
        carr = (L.GraphConstraint * max(len(cons), 1))()
        keep.append(carr)
        for j, c in enumerate(cons):
            carr[j].id_begin, carr[j].id_end = int(c["id_begin"]), int(c["id_end"])
            carr[j].t_be = _pose3d(c.get("t_be"))
            info = np.asarray(c.get("information", np.eye(6)), np.float64).reshape(-1)
            for k in range(36):
                carr[j].information[k] = float(info[k])
            carr[j].type = int(c.get("type", 0))
            q = c.get("quality", {})
            keys = sorted(q)                                          # std::map order
            ka = (C.c_char_p * max(len(keys), 1))(*[k.encode() for k in keys])
            va = (C.c_double * max(len(keys), 1))(*[float(q[k]) for k in keys])
            keep += [ka, va]
            carr[j].n_quality, carr[j].quality_keys, carr[j].quality_values = len(keys), ka, va
            ib = c.get("info", "").encode()
            keep.append(ib)
            carr[j].info = ib
        g.constraints, g.n_constraints = carr, len(cons)
    rc = L.lib().cfear_graph_save(os.fsencode(path), arr, len(nodes))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_graph_save(%s)" % path)


def LoadSimpleGraph(path):
    """LoadSimpleGraph (types.cpp:115-130) -> list of node dicts (the SaveSimpleGraph layout; poses as p+q 7-vectors and
    'T_xyt' as (x, y, theta); 'scan' is NOT built here -- feed node['cells'] to MapPointNormal(cells=...) on a GPU box)."""
    lib = L.lib()
    h = C.c_void_p()
    rc = lib.cfear_graph_load(os.fsencode(path), C.byref(h))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_graph_load(%s)" % path)
    try:
        out = []
        for i in range(lib.cfear_graph_size(h)):
            g = L.GraphNode()
            assert lib.cfear_graph_node_at(h, i, C.byref(g)) == L.OK

            def pose(p):
                return np.array(list(p.p) + list(p.q))

            def cloud(c):
                if c.n < 0:
                    return None
                a = np.ctypeslib.as_array(C.cast(c.xyzi, C.POINTER(C.c_float)), (c.n, 4)).copy() if c.n else np.zeros((0, 4), np.float32)
                return dict(xyzi=a, stamp=int(c.stamp), seq=int(c.seq), frame_id=(c.frame_id or b"").decode())
            xyt = (C.c_double * 3)()
            lib.cfear_pose3d_to_xyt(C.byref(g.T), xyt)
            nd = dict(T=pose(g.T), T_xyt=np.array(xyt), Tgt=pose(g.Tgt), has_Tgt=bool(g.has_Tgt), idx=int(g.idx), stamp=int(g.stamp),
                      motion=np.array(g.motion).reshape(4, 4).T.copy(), cloud_peaks=cloud(g.cloud_peaks),
                      cloud_nopeaks=cloud(g.cloud_nopeaks), normal_input=cloud(g.normal_input), input_is_nopeaks=bool(g.input_is_nopeaks),
                      cells=None, radius=float(g.radius), weight_intensity=bool(g.weight_intensity), constraints=[])
            if g.has_normal:
                nd["cells"] = (np.frombuffer(C.string_at(g.cells, g.n_cells * L.CELL_DTYPE.itemsize), L.CELL_DTYPE).copy()
                               if g.n_cells else np.zeros(0, L.CELL_DTYPE))
            for j in range(g.n_constraints):
                c = g.constraints[j]
                nd["constraints"].append(dict(
                    id_begin=int(c.id_begin), id_end=int(c.id_end), t_be=pose(c.t_be), information=np.array(c.information).reshape(6, 6),
                    type=int(c.type), quality={c.quality_keys[k].decode(): float(c.quality_values[k]) for k in range(c.n_quality)},
                    info=(c.info or b"").decode()))
            out.append(nd)
        return out
    finally:
        lib.cfear_graph_destroy(h)


def pose_graph_optimize(poses, ids, constraints, **par):
    """CeresLeastSquares::Solve (tbv_slam/src/tbv_slam/ceresoptimizer.cpp:13-62) over the nodes `poses` ([n, 7] = p, q(x, y, z, w),
    or [n, 3] planar (x, y, theta)) with node ids `ids` (ascending) and `constraints` (SaveSimpleGraph's constraint dicts:
    id_begin, id_end, t_be, information, type).  Keyword overrides: the cfear_pgo_params fields.  Host code, no GPU
    (pose_graph_optimize_batch solves many graphs in one device call).
    Returns (poses [n, 7], summary dict)."""
    lib = L.lib()
    poses = np.asarray(poses, np.float64)
    n = poses.shape[0]
    arr = (L.Pose3d * n)()
    for i in range(n):
        arr[i] = _pose3d(poses[i])
    ida = np.ascontiguousarray(ids, np.uint64)
    carr = (L.GraphConstraint * max(len(constraints), 1))()
    for j, c in enumerate(constraints):
        carr[j].id_begin, carr[j].id_end = int(c["id_begin"]), int(c["id_end"])
        carr[j].t_be = _pose3d(c.get("t_be"))
        info = np.asarray(c.get("information", np.eye(6)), np.float64).reshape(-1)
        for k in range(36):
            carr[j].information[k] = float(info[k])
        carr[j].type = int(c.get("type", 0))
    p = L.PgoParams()
    lib.cfear_pgo_params_default(C.byref(p))
    for k, v in par.items():
        setattr(p, k, type(getattr(p, k))(v))
    s = L.PgoSummary()
    rc = lib.cfear_pgo_solve(arr, ida.ctypes.data, n, carr, len(constraints), C.byref(p), C.byref(s))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_pgo_solve")
    out = np.array([list(a.p) + list(a.q) for a in arr])
    return out, dict(initial_cost=s.initial_cost, final_cost=s.final_cost, iterations=s.iterations, usable=bool(s.usable),
                     num_residual_blocks=s.num_residual_blocks, linear_iterations=s.linear_iterations)


def _pgo_graph_arrays(poses, ids, constraints, where):
    """One graph as the arrays cfear_pgo_solve_batch reads: poses [n, 7], ids [n] uint64, constraints [m] records."""
    poses = np.asarray(poses, np.float64)
    if poses.ndim != 2 or poses.shape[1] not in (3, 7):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: poses must be [n, 7] (p, q) or [n, 3] (x, y, theta), got %s" % (where, poses.shape))
    if poses.shape[1] == 3:
        poses = np.array([np.concatenate(pose3d_from_xyt(p)) for p in poses]).reshape(-1, 7)
    ids = np.asarray(ids)
    if ids.ndim != 1 or ids.shape[0] != poses.shape[0]:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: %d ids for %d poses" % (where, ids.size, poses.shape[0]))
    if ids.size and ids.min() < 0:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: negative node id" % where)
    rec = np.zeros(len(constraints), L.GRAPH_CONSTRAINT_DTYPE)
    for j, c in enumerate(constraints):
        try:
            rec[j]["id_begin"], rec[j]["id_end"] = int(c["id_begin"]), int(c["id_end"])
            t = c.get("t_be")
            t = np.array([0, 0, 0, 0, 0, 0, 1.0]) if t is None else np.asarray(t, np.float64).reshape(-1)
            rec[j]["t_be"] = np.concatenate(pose3d_from_xyt(t)) if t.size == 3 else t
            rec[j]["information"] = np.asarray(c.get("information", np.eye(6)), np.float64).reshape(36)
            rec[j]["type"] = int(c.get("type", 0))
        except (KeyError, ValueError, TypeError, OverflowError) as e:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: constraint %d: %s" % (where, j, e))
    return np.ascontiguousarray(poses), ids.astype(np.uint64), rec


def pose_graph_optimize_batch(graphs, ctx=None, **par):
    """cfear_pgo_solve_batch: every graph of `graphs` -- (poses, ids, constraints) triples as pose_graph_optimize takes them,
    the planar [n, 3] shorthand included -- solved in ONE device call, one wavefront per graph.  Keyword overrides: the
    cfear_pgo_params fields, one set for the batch.  Returns a list of (poses [n, 7], summary dict), in the order given.
    A graph that pose_graph_optimize would refuse fails the whole call: CfearError with .graph = its index; nothing is solved."""
    lib = L.lib()
    p = L.PgoParams()
    lib.cfear_pgo_params_default(C.byref(p))
    for k, v in par.items():
        if not hasattr(p, k):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "unknown cfear_pgo_params field %r" % k)
        setattr(p, k, type(getattr(p, k))(v))
    arrs = []
    for g, tri in enumerate(graphs):
        if len(tri) != 3:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "graph %d: a (poses, ids, constraints) triple is needed" % g)
        arrs.append(_pgo_graph_arrays(tri[0], tri[1], tri[2], "graph %d" % g))
    if not arrs:
        return []
    node_off = np.concatenate([[0], np.cumsum([a[0].shape[0] for a in arrs])]).astype(np.int64)
    con_off = np.concatenate([[0], np.cumsum([a[2].shape[0] for a in arrs])]).astype(np.int64)
    poses = np.ascontiguousarray(np.concatenate([a[0] for a in arrs], 0))
    ids = np.ascontiguousarray(np.concatenate([a[1] for a in arrs]))
    cons = np.ascontiguousarray(np.concatenate([a[2] for a in arrs]))
    summ = np.zeros(len(arrs), L.PGO_SUMMARY_DTYPE)
    ctx = ctx or default_context()
    bad = C.c_int32(-1)
    rc = ctx._lib.cfear_pgo_solve_batch(ctx.h, poses.ctypes.data, ids.ctypes.data, node_off.ctypes.data, int(node_off[-1]),
                                        cons.ctypes.data, con_off.ctypes.data, int(con_off[-1]), len(arrs), C.byref(p),
                                        summ.ctypes.data, C.byref(bad))
    if rc != L.OK:
        err = L.CfearError(rc, ctx._lib.cfear_last_error(ctx.h).decode())
        err.graph = int(bad.value)
        raise err
    return [(poses[node_off[g]:node_off[g + 1]].copy(),
             dict(initial_cost=float(s["initial_cost"]), final_cost=float(s["final_cost"]), iterations=int(s["iterations"]),
                  usable=bool(s["usable"]), num_residual_blocks=int(s["num_residual_blocks"]),
                  linear_iterations=int(s["linear_iterations"])))
            for g, s in enumerate(summ)]


def pose_graph_prefixes(poses, ids, constraints):
    """The graphs the reference's optimisation thread solves while ONE sequence is mapped: one per accepted loop
    (type 1 constraint, in the order given), holding the nodes up to the loop's later node and every constraint, of any
    type, between them.  Returns a list of (poses, ids, constraints) triples for pose_graph_optimize_batch; ids must ascend."""
    poses, ids = np.asarray(poses, np.float64), np.asarray(ids)
    if ids.ndim != 1 or ids.shape[0] != poses.shape[0] or np.any(ids[1:] <= ids[:-1]):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "ids must ascend and number the poses")
    known = set(int(i) for i in ids)
    out = []
    for c in constraints:
        if int(c.get("type", 0)) != 1:
            continue
        last = max(int(c["id_begin"]), int(c["id_end"]))
        if int(c["id_begin"]) not in known or int(c["id_end"]) not in known:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "loop %d -> %d joins an unknown node" % (c["id_begin"], c["id_end"]))
        n = int(np.searchsorted(ids, last, side="right"))
        out.append((poses[:n].copy(), ids[:n].copy(),
                    [k for k in constraints if max(int(k["id_begin"]), int(k["id_end"])) <= last]))
    return out


# ------------------------------------------------------------------------------------------------
# loop candidates without descriptors: GTVicinityClosure / MiniClosure (tbv_slam/src/tbv_slam/loopclosure.cpp:394-552)
# ------------------------------------------------------------------------------------------------
def closure_params(mode="gtvicinity", **kw):
    """cfear_closure_params with the reference's defaults for `mode` ("gtvicinity": loopclosure.h:84-86, "mini": :95-97);
    keyword overrides: min_d_travel, max_d_travel, max_d_close, verify_via_odometry, odom_sigma_error."""
    if mode not in L.CLOSURE_MODE:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "mode must be one of %s, got %r" % (sorted(L.CLOSURE_MODE), mode))
    p = L.ClosureParams()
    L.lib().cfear_closure_params_default(C.byref(p), L.CLOSURE_MODE[mode])
    for k, v in kw.items():
        if k == "mode" or not hasattr(p, k):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "unknown cfear_closure_params field %r" % k)
        setattr(p, k, type(getattr(p, k))(v))
    return p


def _closure_graph_arrays(graph, where):
    """One graph as the arrays cfear_closure_candidates_batch reads -> positions [n, 3], steps [n], rel_xyt [n, 3] or None."""
    if len(graph) not in (2, 3):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: (poses, constraints) or (positions, steps[, rel_xyt]) is needed" % where)
    second = graph[1]
    from_constraints = len(graph) == 2 and not isinstance(second, np.ndarray) and (len(second) == 0 or isinstance(second[0], dict))
    pos = np.asarray(graph[0], np.float64)
    if pos.ndim != 2 or pos.shape[1] not in ((3, 7) if from_constraints else (3,)):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: %s, got %s" % (
            where, "poses must be [n, 7] (p, q) or [n, 3] (x, y, theta)" if from_constraints else "positions must be [n, 3]", pos.shape))
    n = pos.shape[0]
    if not from_constraints:
        steps = np.asarray(second, np.float64).reshape(-1)
        rel = None if len(graph) == 2 or graph[2] is None else np.asarray(graph[2], np.float64).reshape(-1, 3)
        for name, arr in (("steps", steps), ("rel_xyt", rel)):
            if arr is not None and arr.shape[0] not in (n, max(n - 1, 0)):
                raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: %d %s for %d nodes (one per node, or one per step)" % (where, arr.shape[0], name, n))
        pad = lambda a: a if a.shape[0] == n else np.concatenate([a, np.zeros((1,) + a.shape[1:])])
        return np.ascontiguousarray(pos), pad(steps), None if rel is None else pad(rel)
    # node k is pose k; the odometry constraint between k and k + 1 (either direction: ConstraintsHandler's key is the
    # unordered pair) gives RelativeMotion(k, k + 1) = its t_be as it stands, and the step its translation's norm
    positions = np.zeros((n, 3))
    positions[:, :(2 if pos.shape[1] == 3 else 3)] = pos[:, :(2 if pos.shape[1] == 3 else 3)]
    steps, rel, seen = np.zeros(n), np.zeros((n, 3)), np.zeros(n, bool)
    for j, c in enumerate(second):
        try:
            if int(c.get("type", 0)) != 0:
                continue
            a, b = int(c["id_begin"]), int(c["id_end"])
            t = np.asarray(c["t_be"], np.float64).reshape(-1)
            if t.size not in (3, 7):
                raise ValueError("t_be must hold 3 or 7 values")
        except (KeyError, ValueError, TypeError, OverflowError) as e:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: constraint %d: %s" % (where, j, e))
        k = min(a, b)
        if abs(a - b) != 1 or k < 0 or k + 1 >= n:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: odometry constraint %d joins nodes %d and %d (node ids are 0 .. n - 1, consecutive)" % (where, j, a, b))
        x, y, z = (float(t[0]), float(t[1]), 0.0 if t.size == 3 else float(t[2]))
        steps[k] = np.sqrt((x * x + y * y) + z * z)
        if t.size == 3:
            rel[k] = t
        else:
            pz, out = _pose3d(t), (C.c_double * 3)()
            L.lib().cfear_pose3d_to_xyt(C.byref(pz), out)
            rel[k] = list(out)
        seen[k] = True
    if n > 1 and not seen[:n - 1].all():
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: no odometry constraint between nodes %d and %d" % (
            where, int(np.argmin(seen[:n - 1])), int(np.argmin(seen[:n - 1])) + 1))
    return positions, steps, rel


def closure_candidates(graphs, mode="gtvicinity", ctx=None, **params):
    """cfear_closure_candidates_batch: the loop candidates GTVicinityClosure (mode="gtvicinity", the pairs the reference trains
    and evaluates its loop classifiers on) or MiniClosure (mode="mini", --miniloop-enabled) proposes for every graph of
    `graphs` in ONE device call -- the reference's first SearchAndAddConstraint() from fresh state on a complete graph.
    A graph is (poses, constraints): poses [n, 7] (p, q) or [n, 3] (x, y, theta), node ids 0 .. n - 1, and the odometry
    constraints as OdometryKeyframeFuser.constraint() returns them (other types are skipped); or (positions [n, 3], steps
    [n or n - 1][, rel_xyt [n or n - 1, 3]]) with steps[k] / rel_xyt[k] the odometry from node k to k + 1.  Without rel_xyt
    (then for every graph) odom_bounds stays 0.  Keyword overrides: closure_params().  Returns one CLOSURE_CANDIDATE_DTYPE
    array per graph, a record per origin node: to (-1: none), exhausted, eucl, trav, rel, odom_bounds.  A graph the call
    refuses raises CfearError with .graph = its index."""
    p = closure_params(mode, **params)
    arrs = [_closure_graph_arrays(g, "graph %d" % k) for k, g in enumerate(graphs)]
    if not arrs:
        return []
    with_rel = [a[2] is not None for a in arrs]
    if any(with_rel) and not all(with_rel):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "rel_xyt for every graph or for none")
    off = np.concatenate([[0], np.cumsum([a[0].shape[0] for a in arrs])]).astype(np.int64)
    pos = np.ascontiguousarray(np.concatenate([a[0] for a in arrs], 0))
    steps = np.ascontiguousarray(np.concatenate([a[1] for a in arrs]))
    rel = np.ascontiguousarray(np.concatenate([a[2] for a in arrs], 0)) if all(with_rel) else None
    out = np.zeros(int(off[-1]), L.CLOSURE_CANDIDATE_DTYPE)
    ctx = ctx or default_context()
    bad = C.c_int32(-1)
    rc = ctx._lib.cfear_closure_candidates_batch(ctx.h, pos.ctypes.data, steps.ctypes.data, None if rel is None else rel.ctypes.data,
                                                 off.ctypes.data, int(off[-1]), len(arrs), C.byref(p), out.ctypes.data, C.byref(bad))
    if rc != L.OK:
        err = L.CfearError(rc, ctx._lib.cfear_last_error(ctx.h).decode())
        err.graph = int(bad.value)
        raise err
    return [out[off[g]:off[g + 1]].copy() for g in range(len(arrs))]


def closure_verify_jobs(cands, nodes, poses_xyt, group_base=0):
    """One graph's closure_candidates records as verify_loop_candidates / prepare_verify_batch input: a dict per origin that
    got a candidate, in origin order.  nodes: a dict(scan=MapPointNormal, peaks=float32 [n, 4]) per graph node;
    poses_xyt [n, 3].  As the reference hands its pairs on (loopclosure.cpp:451-452, 538-539): from = max(origin, to),
    to = min(origin, to); sc_sim = 0 as CreateMiniloopConstraint sets it; odom_bounds from the record; group = group_base +
    origin.  t_be_guess is the identity: the reference passes a default-constructed Pose3d there, which types.h:48 leaves
    uninitialised, so the identity is this project's choice, not a restatement."""
    poses_xyt = np.asarray(poses_xyt, np.float64).reshape(-1, 3)
    jobs = []
    for i, c in enumerate(cands):
        if c["to"] < 0:
            continue
        fr, to = max(i, int(c["to"])), min(i, int(c["to"]))
        jobs.append({"from": fr, "to": to, "from_scan": nodes[fr]["scan"], "to_scan": nodes[to]["scan"], "from_peaks": nodes[fr]["peaks"],
                     "to_peaks": nodes[to]["peaks"], "from_pose": poses_xyt[fr], "t_be_guess": (0.0, 0.0, 0.0), "sc_sim": 0.0,
                     "odom_bounds": float(c["odom_bounds"]), "group": int(group_base) + i})
    return jobs


# ------------------------------------------------------------------------------------------------
# trajectory evaluation: the KITTI odometry metric (radar_kitti_benchmark/python/kitti_odometry.py)
# ------------------------------------------------------------------------------------------------
def eval_params(step_size=10, alignment="6dof", lengths=None):
    """cfear_eval_params: eval_odom.py's defaults.  alignment: None / "none" or "6dof"; the devkit's "scale", "7dof" and
    "scale_7dof" are passed on and refused by the library."""
    p = L.EvalParams()
    L.lib().cfear_eval_params_default(C.byref(p))
    if alignment not in L.EVAL_ALIGN:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "unknown alignment %r" % (alignment,))
    p.step_size, p.alignment = int(step_size), L.EVAL_ALIGN[alignment]
    if lengths is not None:
        if len(lengths) != L.EVAL_NUM_LENGTHS:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%d lengths are evaluated" % L.EVAL_NUM_LENGTHS)
        for k, v in enumerate(lengths):
            p.lengths[k] = float(v)
    return p


def kitti_read(path):
    """load_poses_from_txt (kitti_odometry.py:93-121) -> float64 [n, 12]; lines of 12 numbers, or of 13 with the index first."""
    lib = L.lib()
    n = C.c_int64()
    rc = lib.cfear_kitti_read(os.fsencode(path), None, 0, C.byref(n))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_kitti_read(%s)" % path)
    out = np.zeros((n.value, 12), np.float64)
    rc = lib.cfear_kitti_read(os.fsencode(path), out.ctypes.data, n.value, C.byref(n))
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_kitti_read(%s)" % path)
    return out


def kitti_write(path, poses):
    """EvalTrajectory::Write (eval_trajectory.cpp:169-183): one pose per line, 12 numbers with 6 decimals."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    rc = L.lib().cfear_kitti_write(os.fsencode(path), poses.ctypes.data, poses.shape[0])
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_kitti_write(%s)" % path)


def kitti_from_xyt(xyt):
    """Planar poses [..., 3] (x, y, theta), e.g. OdometryKeyframeFuser's info["pose"] of one stream over time -> [..., 12]."""
    xyt = np.ascontiguousarray(xyt, np.float64)
    assert xyt.shape[-1] == 3
    out = np.zeros(xyt.shape[:-1] + (12,), np.float64)
    rc = L.lib().cfear_kitti_from_xyt(xyt.ctypes.data, xyt.size // 3, 3, out.ctypes.data)
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_kitti_from_xyt")
    return out


def _stamped_file(fn, path, values, width, stamps):
    values = np.ascontiguousarray(values, np.float64).reshape(-1, width)
    stamps = np.ascontiguousarray(stamps, np.int64).reshape(-1)
    if stamps.shape[0] != values.shape[0]:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s(%s): %d stamps for %d records" % (fn, path, stamps.shape[0], values.shape[0]))
    rc = getattr(L.lib(), fn)(os.fsencode(path), values.ctypes.data, stamps.ctypes.data, values.shape[0])
    if rc != L.OK:
        raise L.CfearError(rc, "%s(%s)" % (fn, path))


def tum_write(path, poses, stamps):
    """EvalTrajectory::WriteTUM (eval_trajectory.cpp:185-211): `sec.nsec x y z qx qy qz qw` per pose; stamps in nanoseconds."""
    _stamped_file("cfear_tum_write", path, poses, 12, stamps)


def cov_write(path, cov, stamps):
    """EvalTrajectory::WriteCov (eval_trajectory.cpp:214-232): the stamp and the 36 entries of the 6 x 6 covariance per line."""
    _stamped_file("cfear_cov_write", path, cov, 36, stamps)


class SyncResult:
    """What sync_trajectories returns: est, gt [N, 12], stamps [N] and rows [N] (L.SYNC_ROW_DTYPE; on the device a uint8
    [N, 16] tensor, rows_host() reads it back) hold pair t's counts[t] kept rows from offsets[t] on; offsets and counts are
    host arrays.  eval_trajectories(r.est, r.gt, lengths=r.counts, offsets=r.offsets) scores it as it is."""

    def __init__(self, est, gt, stamps, rows, counts, offsets):
        self.est, self.gt, self.stamps, self.rows, self.counts, self.offsets = est, gt, stamps, rows, counts, offsets

    def rows_host(self):
        return self.rows.cpu().numpy().view(L.SYNC_ROW_DTYPE).reshape(-1) if _is_torch(self.rows) else self.rows

    def pair(self, t):
        """Pair t's kept rows as host arrays: dict(est, gt, stamps, rows)."""
        sl = slice(int(self.offsets[t]), int(self.offsets[t]) + int(self.counts[t]))
        host = lambda x: None if x is None else (x[sl].cpu().numpy() if _is_torch(x) else x[sl])
        return dict(est=host(self.est), gt=host(self.gt), stamps=host(self.stamps), rows=self.rows_host()[sl])


def sync_trajectories(est, est_stamps, gt, gt_stamps, mode="chained", ctx=None):
    """EvalTrajectory's timestamp synchronisation for a batch of (estimate, ground truth) pairs in one device call
    (cfear_sync_trajectories): every estimate keeps the ground truth interpolated at its stamp, estimates that no two
    ground-truth poses bracket are dropped.  mode "chained": One2OneCorrespondance (eval_trajectory.cpp:400-423);
    "independent": Interpolate(t, out) per stamp (eval_trajectory.h:141-144).

    est, gt: lists (one entry per pair) of [n, 12] KITTI rows, est_stamps, gt_stamps: lists of [n] int64 nanoseconds; all
    NumPy arrays, or all torch CUDA tensors (float64 / int64).  est may be None (labelling stamps).  -> SyncResult, on the
    side the inputs are on."""
    if mode not in L.SYNC_MODE:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "unknown mode %r" % (mode,))
    n_traj = len(est_stamps)
    if len(gt) != n_traj or len(gt_stamps) != n_traj or (est is not None and len(est) != n_traj):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "est, est_stamps, gt and gt_stamps must hold one entry per pair")
    everything = list(est_stamps) + list(gt) + list(gt_stamps) + (list(est) if est is not None else [])
    device = any(_is_torch(x) for x in everything)
    if device and not all(_is_torch(x) for x in everything):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "poses and stamps must all be torch CUDA tensors or all be host arrays")
    if device:
        import torch
        dev = everything[0].device
        for x in everything:
            if not x.is_cuda or x.dtype not in (torch.float64, torch.int64):
                raise L.CfearError(L.ERR_INVALID_ARGUMENT, "float64 poses and int64 stamps on the device are needed, got %s on %s" % (x.dtype, x.device))
        cat = lambda xs, w, dt: (torch.cat([x.reshape(-1, w) if w else x.reshape(-1) for x in xs]).contiguous() if xs
                                 else torch.zeros((0, w) if w else (0,), dtype=dt, device=dev))
        zeros = lambda shape, dt: torch.zeros(shape, dtype={np.float64: torch.float64, np.int64: torch.int64, np.uint8: torch.uint8}[dt], device=dev)
        f64, i64 = torch.float64, torch.int64
    else:
        cat = lambda xs, w, dt: (np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape((-1, w) if w else (-1,)) for x in xs]))
                                 if xs else np.zeros((0, w) if w else (0,), dt))
        zeros = lambda shape, dt: np.zeros(shape, dt)
        f64, i64 = np.float64, np.int64
    es, gs = cat(list(est_stamps), 0, i64), cat(list(gt_stamps), 0, i64)
    e = None if est is None else cat(list(est), 12, f64)
    g = cat(list(gt), 12, f64)
    le = np.array([int(x.shape[0]) for x in est_stamps], np.int32)
    lg = np.array([int(x.shape[0]) for x in gt_stamps], np.int32)
    if g.shape[0] != int(lg.sum()) or (e is not None and e.shape[0] != int(le.sum())):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "a pair's poses and stamps differ in length")
    n = int(le.sum())
    offsets = np.zeros(n_traj, np.int64)
    offsets[1:] = np.cumsum(le[:-1])
    e_out = None if e is None else zeros((n, 12), np.float64)
    g_out, s_out = zeros((n, 12), np.float64), zeros((n,), np.int64)
    rows = zeros((n, 16), np.uint8) if device else np.zeros(n, L.SYNC_ROW_DTYPE)
    counts = np.zeros(n_traj, np.int32)
    ctx = ctx or default_context()
    if device:
        _torch_ready(ctx, es, gs, g, g_out, s_out, rows)
    ctx.check(ctx._lib.cfear_sync_trajectories(ctx.h, L.SYNC_MODE[mode], _ptr(e)[0], _ptr(es)[0], None, le.ctypes.data, _ptr(g)[0], _ptr(gs)[0],
                                               None, lg.ctypes.data, n_traj, _ptr(e_out)[0], _ptr(g_out)[0], _ptr(s_out)[0], _ptr(rows)[0],
                                               counts.ctypes.data))
    return SyncResult(e_out, g_out, s_out, rows, counts, offsets)


def eval_trajectories(est, gt, lengths=None, step_size=10, alignment="6dof", want_rows=True, par=None, ctx=None, offsets=None):
    """The KITTI odometry metric of a batch of (estimate, ground truth) pairs in one call (cfear_eval_trajectories).

    est, gt: lists of [n_i, 12] arrays (one per pair), or one [N, 12] array / torch CUDA tensor each holding the pairs one
    after the other with `lengths` [n_traj] (a single pair when lengths is None), or pair t at offsets[t] when `offsets`
    [n_traj] is given (sync_trajectories' layout).  Returns (summaries, rows): structured
    arrays of L.EVAL_SUMMARY_DTYPE [n_traj] and L.EVAL_ROW_DTYPE [n_rows] (None unless want_rows); figures in radians and
    fractions (write_result's conversions: include/cfear_hip.h).  A pair whose two trajectories differ in length, one with
    fewer than 2 poses, step_size < 1 and the scale / 7dof alignments raise CfearError(ERR_INVALID_ARGUMENT)."""
    p = par if par is not None else eval_params(step_size, alignment)
    lib = L.lib()
    if isinstance(est, (list, tuple)):
        if not isinstance(gt, (list, tuple)) or len(gt) != len(est):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "est and gt must hold the same number of trajectories")
        if offsets is not None:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "offsets address one flat array: lists of trajectories follow each other")
        est = [np.asarray(e, np.float64).reshape(-1, 12) for e in est]
        gt = [np.asarray(g, np.float64).reshape(-1, 12) for g in gt]
        le = np.array([e.shape[0] for e in est], np.int32)
        lg = np.array([g.shape[0] for g in gt], np.int32)
        rc = lib.cfear_eval_check(C.byref(p), le.ctypes.data, lg.ctypes.data, len(est))
        if rc != L.OK:
            raise L.CfearError(rc, "evaluation refused: step_size >= 1, alignment none / 6dof, every pair of one length >= 2")
        est = np.ascontiguousarray(np.concatenate(est, 0)) if est else np.zeros((0, 12))
        gt = np.ascontiguousarray(np.concatenate(gt, 0)) if gt else np.zeros((0, 12))
        lengths = le
    else:
        if _is_torch(est) != _is_torch(gt):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "est and gt must both be torch CUDA tensors or both be host arrays")
        if _is_torch(est):
            import torch
            for name, x in (("est", est), ("gt", gt)):
                # the kernels read 96 bytes per pose: anything but contiguous float64 [N, 12] on the device would be read past its end
                if x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != 12 or not x.is_cuda or not x.is_contiguous():
                    raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: a contiguous float64 [N, 12] CUDA tensor is needed, got %s %s on %s"
                                       % (name, x.dtype, tuple(x.shape), x.device))
        else:
            est, gt = (np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 12)) for a in (est, gt))
        n_e, n_g = est.shape[0], gt.shape[0]
        lengths = np.array([n_e], np.int32) if lengths is None else np.ascontiguousarray(lengths, np.int32)
        lg = lengths if n_g == n_e else np.array([n_g], np.int32)
        rc = lib.cfear_eval_check(C.byref(p), lengths.ctypes.data, lg.ctypes.data, len(lengths))
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.int64)
            inside = len(offsets) == len(lengths) and (offsets >= 0).all() and (offsets + lengths <= n_e).all()
        else:
            inside = int(lengths.sum()) == n_e
        if rc != L.OK or n_e != n_g or not inside or len(lg) != len(lengths):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "evaluation refused: step_size >= 1, alignment none / 6dof, est and gt "
                               "of one shape, lengths >= 2 that add up to it (or lie inside it from `offsets` on)")
    ctx = ctx or default_context()
    n_traj = len(lengths)
    summaries = np.zeros(n_traj, L.EVAL_SUMMARY_DTYPE)
    rows, cap = None, 0
    if want_rows:
        # every start frame has at most one row per length
        cap = int(sum((int(n) + p.step_size - 1) // p.step_size for n in lengths)) * L.EVAL_NUM_LENGTHS
        rows = np.zeros(max(cap, 1), L.EVAL_ROW_DTYPE)
    n_rows = C.c_int64()
    ctx.check(ctx._lib.cfear_eval_trajectories(ctx.h, _ptr(est)[0], _ptr(gt)[0], None if offsets is None else offsets.ctypes.data,
                                               lengths.ctypes.data, n_traj, C.byref(p),
                                               summaries.ctypes.data, rows.ctypes.data if want_rows else None, cap,
                                               C.byref(n_rows)))
    return summaries, (rows[:n_rows.value] if want_rows else None)


def eval_result_lines(seq, s):
    """write_result (kitti_odometry.py:608-630): the 12 lines of result.txt for one summary record."""
    return ["Sequence-nr, {} \n".format(seq),
            "Trans.err.(%), {:.5f} \n".format(s["ave_t_err"] * 100),
            "Rot.err.(deg/100m), {:.5f} \n".format(s["ave_r_err"] / np.pi * 180 * 100),
            "ATE(m), {:.5f} \n".format(s["ate"]),
            "RPE(m), {:.5f} \n".format(s["rpe_trans"]),
            "RPE-dev(m), {:.5f} \n".format(s["rpe_trans_dev"]),
            "RPE(deg), {:.5f} \n".format(s["rpe_rot"] * 180 / np.pi),
            "RPE-dev(deg), {:.5f} \n".format(s["rpe_rot_dev"] * 180 / np.pi),
            "bias-x(m), {:.6f} \n".format(s["bias_x"]),
            "bias-y(m), {:.6f} \n".format(s["bias_y"]),
            "bias-theta(deg), {:.6f} \n".format(s["bias_theta"] * 180 / np.pi),
            "RMSE (m), {:.5f} \n".format(s["rmse_trans"])]


class KittiEvalOdom:
    """KittiEvalOdom of radar_kitti_benchmark/python/kitti_odometry.py (:82-91, :636-784) without the plots: eval() scores
    every NN.txt of result_dir (NN = 00 .. 34, as the devkit's seq_list) against gt_dir/NN.txt in ONE evaluator call and
    writes result_dir/result.txt and result_dir/errors/NN.txt in the devkit's format, so the directory can be diffed
    against one the devkit wrote."""

    def __init__(self, step_size=10, ctx=None):
        self.step_size = step_size
        self.lengths = [100, 200, 300, 400, 500, 600, 700, 800]
        self.ctx = ctx

    def eval(self, gt_dir, result_dir, alignment=None, seqs=None):
        if seqs is None:
            seqs = [i for i in range(35) if os.path.exists(os.path.join(result_dir, "%02d.txt" % i))]
        self.eval_seqs = list(seqs)
        est = [kitti_read(os.path.join(result_dir, "%02d.txt" % i)) for i in self.eval_seqs]
        gt = [kitti_read(os.path.join(gt_dir, "%02d.txt" % i)) for i in self.eval_seqs]
        summaries, rows = eval_trajectories(est, gt, par=eval_params(self.step_size, alignment, self.lengths), ctx=self.ctx)
        os.makedirs(os.path.join(result_dir, "errors"), exist_ok=True)
        with open(os.path.join(result_dir, "result.txt"), "w") as f:
            for k, i in enumerate(self.eval_seqs):
                r = rows[rows["trajectory"] == k]
                with open(os.path.join(result_dir, "errors", "%02d.txt" % i), "w") as fe:       # save_sequence_errors, :251-262
                    fe.writelines("%d %r %r %d %r\n" % (a, float(b), float(c), int(d), float(e)) for a, b, c, d, e in
                                  zip(r["first_frame"], r["r_err"], r["t_err"], r["length"], r["speed"]))
                f.writelines(eval_result_lines(i, summaries[k]))
        return summaries, rows


# ------------------------------------------------------------------------------------------------
# scoring the loop detector: loop rows (PoseGraph::UpdateStatistics), loop.csv (EvaluationManager), ROC / PR curves
# (place_recognition_radar/python/LoopClosureEval.py, evaluation/3_loop_closure/3_loop_closure.py)
# ------------------------------------------------------------------------------------------------
def _struct_params(cls, default, kw, what):
    p = cls()
    default(C.byref(p))
    for k, v in kw.items():
        if k == "pad" or not hasattr(p, k):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "unknown %s field %r" % (what, k))
        setattr(p, k, type(getattr(p, k))(v))
    return p


def loop_stats_params(**kw):
    """cfear_loop_stats_params with the reference's constants: max_distance 6, max_registration_translation 4,
    max_registration_rotation_deg 2.5 (EvaluationManager.cpp:14-16), no_loop_distance 100000, min_index_gap 10
    (posegraph.cpp:334,358)."""
    return _struct_params(L.LoopStatsParams, L.lib().cfear_loop_stats_params_default, kw, "cfear_loop_stats_params")


def loop_curves_params(**kw):
    """cfear_loop_curves_params: p_threshold 0.9, drop_intermediate 1, reference_endpoints 1."""
    return _struct_params(L.LoopCurvesParams, L.lib().cfear_loop_curves_params_default, kw, "cfear_loop_curves_params")


def _device_bytes(n, like):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device=like.device)


def loop_stats_flat(node_offsets, gt_xyt, has_gt, candidates, ctx=None, **params):
    """cfear_loop_stats_batch on the flat arrays: node_offsets int64 [n_graphs + 1] (host), gt_xyt float64 [n_nodes, 3],
    has_gt uint8 [n_nodes] and candidates (LOOP_CANDIDATE_DTYPE records) all NumPy, or all torch CUDA tensors (the candidates
    then as their bytes, uint8 [n_cand * 40]).  Returns LOOP_ROW_DTYPE records: a NumPy array, or for device buffers a uint8
    tensor of their bytes.  A refusal raises CfearError with .candidate = the candidate it names (-1: none)."""
    par = loop_stats_params(**params)
    off = np.ascontiguousarray(node_offsets, np.int64)
    device = _is_torch(gt_xyt) or _is_torch(candidates)
    ctx = ctx or default_context()
    if device:
        n_cand = candidates.numel() // L.LOOP_CANDIDATE_DTYPE.itemsize
        rows = _device_bytes(n_cand * L.LOOP_ROW_DTYPE.itemsize, candidates)
        _torch_ready(ctx, gt_xyt, has_gt, candidates, rows)
    else:
        gt_xyt = np.ascontiguousarray(gt_xyt, np.float64).reshape(-1, 3)
        has_gt = np.ascontiguousarray(has_gt, np.uint8)
        candidates = np.ascontiguousarray(candidates, L.LOOP_CANDIDATE_DTYPE)
        n_cand = candidates.shape[0]
        rows = np.zeros(n_cand, L.LOOP_ROW_DTYPE)
    n_nodes = int(has_gt.shape[0])
    bad = C.c_int64(-1)
    rc = ctx._lib.cfear_loop_stats_batch(ctx.h, off.ctypes.data, _ptr(gt_xyt)[0], _ptr(has_gt)[0], n_nodes, len(off) - 1,
                                         _ptr(candidates)[0], n_cand, C.byref(par), _ptr(rows)[0], C.byref(bad))
    if rc != L.OK:
        err = L.CfearError(rc, ctx._lib.cfear_last_error(ctx.h).decode())
        err.candidate = int(bad.value)
        raise err
    return rows


def loop_candidates(cands):
    """LOOP_CANDIDATE_DTYPE records from such an array, or from dicts / tuples of (graph, from, to, guess_nr, guess_xyt)."""
    if isinstance(cands, np.ndarray) and cands.dtype == L.LOOP_CANDIDATE_DTYPE:
        return np.ascontiguousarray(cands)
    out = np.zeros(len(cands), L.LOOP_CANDIDATE_DTYPE)
    for i, c in enumerate(cands):
        if not isinstance(c, dict):
            c = dict(zip(("graph", "from", "to", "guess_nr", "guess_xyt"), c))
        out[i] = (int(c.get("graph", 0)), int(c["from"]), int(c["to"]), int(c.get("guess_nr", 0)),
                  np.asarray(c.get("guess_xyt", (0.0, 0.0, 0.0)), np.float64).reshape(3))
    return out


def loop_stats(graphs, candidates, ctx=None, **params):
    """cfear_loop_stats_batch: PoseGraph::UpdateStatistics (posegraph.cpp:332-371) and EvaluationManager::
    getCandidateLoopStatus for every candidate of a batch of graphs in one device call.  graphs: a list of gt_xyt [n, 3]
    planar ground-truth poses, or of (gt_xyt, has_gt [n]); candidates: loop_candidates() input, `graph` indexing `graphs`.
    Keyword overrides: loop_stats_params().  Returns LOOP_ROW_DTYPE records in candidate order: diff (loop.csv's diff.x,
    diff.y, diff.z), closest_loop_distance, candidate_loop_distance, transl_error, rot_error, close_xy, id_close, is_loop,
    candidate_close, prediction_pos_ok."""
    gts, has = [], []
    for k, g in enumerate(graphs):
        gt, h = g if isinstance(g, tuple) else (g, None)
        gt = np.asarray(gt, np.float64).reshape(-1, 3)
        h = np.ones(gt.shape[0], np.uint8) if h is None else np.asarray(h).astype(np.uint8).reshape(-1)
        if h.shape[0] != gt.shape[0]:
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "graph %d: %d has_gt flags for %d poses" % (k, h.shape[0], gt.shape[0]))
        gts.append(gt)
        has.append(h)
    off = np.concatenate([[0], np.cumsum([g.shape[0] for g in gts])]).astype(np.int64)
    gt = np.concatenate(gts, 0) if gts else np.zeros((0, 3))
    h = np.concatenate(has) if has else np.zeros(0, np.uint8)
    return loop_stats_flat(off, gt, h, loop_candidates(candidates), ctx, **params)


LOOP_CURVE_ARRAYS = ("roc_fpr", "roc_tpr", "roc_thr", "pr_precision", "pr_recall", "pr_thr")


def loop_curves_flat(row_offsets, y, score, pos_ok=None, ctx=None, **params):
    """cfear_loop_curves_batch on the flat arrays: row_offsets int64 [n_exp + 1] (host); y uint8, score float64 and the
    optional pos_ok uint8, [n_rows] each, all NumPy or all torch CUDA tensors.  Returns (arrays, records): the six curve
    arrays of n_rows + n_exp entries (NaN where the call wrote nothing) keyed by LOOP_CURVE_ARRAYS, of the inputs' kind, and
    the LOOP_CURVES_RESULT_DTYPE records (NumPy).  A refusal raises CfearError with .experiment."""
    par = loop_curves_params(**params)
    off = np.ascontiguousarray(row_offsets, np.int64)
    n_exp = len(off) - 1
    ctx = ctx or default_context()
    if _is_torch(score):
        import torch
        n_rows = int(score.shape[0])
        arrays = {k: torch.full((n_rows + n_exp,), float("nan"), dtype=torch.float64, device=score.device) for k in LOOP_CURVE_ARRAYS}
        _torch_ready(ctx, y, score, pos_ok, *arrays.values())
    else:
        y = np.ascontiguousarray(y, np.uint8)
        score = np.ascontiguousarray(score, np.float64)
        pos_ok = None if pos_ok is None else np.ascontiguousarray(pos_ok, np.uint8)
        n_rows = int(score.shape[0])
        arrays = {k: np.full(n_rows + n_exp, np.nan) for k in LOOP_CURVE_ARRAYS}
    if int(y.shape[0]) != n_rows or (pos_ok is not None and int(pos_ok.shape[0]) != n_rows):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "y, score and pos_ok must hold one entry per row")
    rec = np.zeros(max(n_exp, 0), L.LOOP_CURVES_RESULT_DTYPE)
    bad = C.c_int32(-1)
    rc = ctx._lib.cfear_loop_curves_batch(ctx.h, off.ctypes.data, _ptr(y)[0], _ptr(score)[0], _ptr(pos_ok)[0], n_rows, n_exp,
                                          C.byref(par), *[_ptr(arrays[k])[0] for k in LOOP_CURVE_ARRAYS], rec.ctypes.data, C.byref(bad))
    if rc != L.OK:
        err = L.CfearError(rc, ctx._lib.cfear_last_error(ctx.h).decode())
        err.experiment = int(bad.value)
        raise err
    return arrays, rec


def loop_curve_slices(arrays, rec, row_offsets):
    """One dict per experiment of a loop_curves_flat() answer: the six arrays cut to their lengths, and `record`."""
    out = []
    for e, r in enumerate(rec):
        o = int(row_offsets[e]) + e
        lens = dict(roc_fpr=r["n_roc"], roc_tpr=r["n_roc"], roc_thr=r["n_roc"], pr_precision=r["n_pr"], pr_recall=r["n_pr"],
                    pr_thr=max(int(r["n_pr"]) - 1, 0))
        d = {k: arrays[k][o:o + int(lens[k])] for k in LOOP_CURVE_ARRAYS}
        d["record"] = r
        out.append(d)
    return out


def loop_curves(experiments, ctx=None, curves=None, **params):
    """cfear_loop_curves_batch: sklearn's roc_curve, auc and precision_recall_curve, and the confusion matrix, accuracy,
    precision and recall at p_threshold, for every experiment in one device call and without sklearn.  experiments: a list
    of (y, score) or (y, score, pos_ok) -- pos_ok for all or for none.  Keyword overrides: loop_curves_params().  Returns a
    dict per experiment: roc_fpr, roc_tpr, roc_thr, pr_precision, pr_recall, pr_thr and `record` (auc, accuracy,
    precision, recall, n_pos, n_neg, confusion = tn, fp, fn, tp, n_thresholds, n_roc, n_pr, status).  An experiment with no
    rows, one class only, a label other than 0 or 1 or a NaN score has status ERR_INVALID_ARGUMENT and empty arrays.
    curves: a stand-in for loop_curves_flat with its signature (the tests' NumPy model)."""
    if not experiments:
        return []
    with_ok = [len(e) > 2 and e[2] is not None for e in experiments]
    if any(with_ok) and not all(with_ok):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "pos_ok for every experiment or for none")
    off = np.concatenate([[0], np.cumsum([len(e[1]) for e in experiments])]).astype(np.int64)
    y = np.concatenate([np.asarray(e[0]).astype(np.uint8).reshape(-1) for e in experiments])
    score = np.concatenate([np.asarray(e[1], np.float64).reshape(-1) for e in experiments])
    ok = np.concatenate([np.asarray(e[2]).astype(np.uint8).reshape(-1) for e in experiments]) if all(with_ok) else None
    if curves is None:
        arrays, rec = loop_curves_flat(off, y, score, ok, ctx, **params)
    else:
        arrays, rec = curves(off, y, score, ok, **params)
    return loop_curve_slices(arrays, rec, off)


LOOP_CSV_HEADER = ("from.x,from.y,from.z,to.x,to.y,to.z,close.x,close.y,close.z,diff.x,diff.y,diff.z,closest_loop_distance,"
                   "candidate_loop_distance,id_from,id_to,id_close,guess_nr").split(",")   # LoopCandidates::namesToString


def loop_table(graphs, candidates, rows, quality, **columns):
    """The columns of loop.csv for loop_stats() rows, as a dict of NumPy arrays in file order: the 18 of LOOP_CSV_HEADER,
    then `quality` (name -> [n_cand] values) in the order of the reference's std::map (sorted by name), then `columns`
    (the pars_str / vals_str pair of EvaluationManager::writeResultsToCSV: a scalar or an [n_cand] array each)."""
    cands = loop_candidates(candidates)
    gts = [np.asarray(g[0] if isinstance(g, tuple) else g, np.float64).reshape(-1, 3) for g in graphs]
    n = len(cands)
    pf = np.array([gts[c["graph"]][c["from"]] for c in cands]).reshape(n, 3)
    pt = np.array([gts[c["graph"]][c["to"]] for c in cands]).reshape(n, 3)
    zero = np.zeros(n)
    t = {"from.x": pf[:, 0], "from.y": pf[:, 1], "from.z": zero, "to.x": pt[:, 0], "to.y": pt[:, 1], "to.z": zero,
         "close.x": rows["close_xy"][:, 0], "close.y": rows["close_xy"][:, 1], "close.z": zero,
         "diff.x": rows["diff"][:, 0], "diff.y": rows["diff"][:, 1], "diff.z": rows["diff"][:, 2],
         "closest_loop_distance": rows["closest_loop_distance"], "candidate_loop_distance": rows["candidate_loop_distance"],
         "id_from": cands["from"].astype(np.int64), "id_to": cands["to"].astype(np.int64),
         "id_close": rows["id_close"].astype(np.int64), "guess_nr": cands["guess_nr"].astype(np.int64)}
    for k in sorted(quality):
        t[k] = np.asarray(quality[k], np.float64).reshape(n)
    for k, v in columns.items():
        t[k] = np.broadcast_to(np.asarray(v), (n,)).copy()
    return t


def write_loop_csv(path, table, quality_names=()):
    """EvaluationManager::writeResultsToCSV (EvaluationManager.cpp:29-57): the header of LoopCandidates::namesToString and
    one line per row of `table` (loop_table()).  The row's own floating-point values are written as "%.6g", which is what
    the reference's setprecision(6) stream writes; the columns named in quality_names as "%.6f" (Join, cfear_radarodometry/
    utils.h:64-83, is std::fixed); integers and strings as they are.  The reference's scripts therefore see ROUNDED rows:
    labels computed from a file can differ from the flags of loop_stats() where an error lies within the rounding of a
    limit."""
    names = list(table)
    with open(path, "w") as f:
        f.write(",".join(names) + "\n")
        cols = [np.asarray(table[k]) for k in names]
        for i in range(len(cols[0]) if cols else 0):
            vals = []
            for k, c in zip(names, cols):
                v = c[i]
                if c.dtype.kind == "f":
                    vals.append(("%.6f" if k in quality_names else "%.6g") % v)
                else:
                    vals.append(str(v))
            f.write(",".join(vals) + "\n")


def read_loop_csv(path):
    """loop.csv -> a dict of NumPy arrays in file order (what pandas.read_csv(skipinitialspace=True) gives the reference's
    scripts): int64 where every value of a column is an integer literal, float64 where every value is a number, else str."""
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    names = [s.strip() for s in lines[0].split(",")]
    cells = [[s.strip() for s in ln.split(",")] for ln in lines[1:]]
    table = {}
    for j, k in enumerate(names):
        col = [r[j] for r in cells]
        for kind in (np.int64, np.float64):
            try:
                table[k] = np.array([kind(v) for v in col], kind)
                break
            except ValueError:
                continue
        else:
            table[k] = np.array(col)
    return table


def write_loop_result(path, train, test, coef, intercept, p_threshold, nr_correct_candidates, nr_loops):
    """WriteFile of place_recognition_radar/python/LoopClosureEval.py:26-52 (its lines :31-46).  train, test: records or
    dicts with accuracy, precision and recall."""
    ratio = nr_correct_candidates / nr_loops if nr_loops else float("nan")
    lines = ["Training accuracy[%], {:.3f}\n".format(train["accuracy"] * 100),
             "Training precision [%], {:.3f}\n".format(train["precision"] * 100),
             "Training recall [%], {:.3f}\n".format(train["recall"] * 100),
             "Testing accurac [%], {:.3f}\n".format(test["accuracy"] * 100),
             "Testing precision [%], {:.3f}\n".format(test["precision"] * 100),
             "Testing recall [%], {:.3f}\n".format(test["recall"] * 100),
             "nr correct candidates, {}\n".format(nr_correct_candidates),
             "nr loops, {}\n".format(nr_loops),
             "correct_loop_ratio [%], {:.3f}\n".format(ratio * 100),
             "Coef, {}\n".format(np.asarray(coef, np.float64).reshape(1, -1)),
             "Intercept {}\n".format(np.asarray(intercept, np.float64).reshape(-1)),
             "Threshold, {}\n".format(p_threshold)]
    with open(path, "w") as f:
        f.writelines(lines)
    return lines


class LoopClosureEval:
    """evaluation/3_loop_closure/3_loop_closure.py's loop over the settings 1) - 8) of the paper's ablation, without pandas,
    sklearn or matplotlib: labels, training rows, classifiers (logreg_fit_batch, all models of all settings in one call),
    probabilities, best-guess selection and the curves of all settings in one loop_curves() call.
    table: loop.csv's columns as a dict of arrays (loop_table() / read_loop_csv()); it needs diff.x, diff.y, diff.z,
    closest_loop_distance, id_from, id_to, guess_nr, odom-bounds, sc-sim, alignment_quality.  The three columns that tell
    the settings apart ("SC - odometry_coupled_closure", "Scan Context - raw_scan_context", "SC - augment_sc") default to
    1, 0, 1 where the table lacks them.  The script's TrainClassifier leaves class weights alone, so class_weight_balanced
    is 0 here.  The threshold statistics in a setting's record are those of its masked score y_prob at p_threshold, with
    `candidate close` as pos_ok."""

    NAMES = ("1) Radar Scan Context", "2) Aggregated point cloud map", "3) Origin augmentation", "4) Alignment loop verification",
             "5) Odometry decoupled", "6) Odometry coupled", "7) Cascaded classifier", "8) Multiple candidate selection")
    FEATURE_COLS_ALL = (["sc-sim"], ["odom-bounds", "sc-sim"], ["sc-sim", "alignment_quality"],
                        ["odom-bounds", "sc-sim", "alignment_quality"])
    COUPLED, RAW, AUGMENT = "SC - odometry_coupled_closure", "Scan Context - raw_scan_context", "SC - augment_sc"

    def __init__(self, table, p_threshold=0.9, max_distance=6.0, max_registration_distance=4.0, max_registration_rotation=2.5,
                 ctx=None):
        n = len(table["guess_nr"])
        t = {k: np.asarray(v) for k, v in table.items()}
        for k, v in ((self.COUPLED, 1), (self.RAW, 0), (self.AUGMENT, 1)):
            t.setdefault(k, np.full(n, v, np.int64))
        dx, dy, dz = (np.asarray(t[k], np.float64) for k in ("diff.x", "diff.y", "diff.z"))
        transl = np.sqrt(dx * dx + dy * dy)                                                     # 3_loop_closure.py:87-92
        t["is loop"] = (np.asarray(t["closest_loop_distance"], np.float64) < max_distance).astype(np.int64)
        t["candidate close"] = (transl < max_registration_distance) & (np.fabs(dz) < max_registration_rotation * math.pi / 180.0)
        t["candidate transl_error"] = transl
        t["candidate rot_error"] = 180.0 / math.pi * np.fabs(dz)
        t["prediction pos ok"] = ((t["is loop"] == 0) | t["candidate close"]).astype(np.int64)
        keep = np.asarray(t["guess_nr"]) >= 0                                                   # :93
        self.table = {k: v[keep] for k, v in t.items()}
        self.p_threshold = float(p_threshold)
        self.ctx = ctx

    @classmethod
    def settings_name(cls, feature_cols=None, guess0=True, radar_raw=1, augment=0, odometry_coupled=1, cascaded=False):
        """GetNameFromSettings (3_loop_closure.py:26-52): the setting's name, '' for a combination that is not one of the
        eight; without arguments, the eight names."""
        if feature_cols is None:
            return list(cls.NAMES)
        sc, al, full = ["sc-sim"], ["sc-sim", "alignment_quality"], ["odom-bounds", "sc-sim", "alignment_quality"]
        known = {(tuple(sc), True, 0, 1, 0, False): 0, (tuple(sc), True, 0, 0, 0, False): 1, (tuple(sc), True, 0, 0, 1, False): 2,
                 (tuple(al), True, 0, 0, 1, False): 3, (tuple(full), True, 0, 0, 1, False): 4, (tuple(full), True, 1, 0, 1, False): 5,
                 (tuple(full), True, 1, 0, 1, True): 6, (tuple(full), False, 1, 0, 1, False): 7}
        k = known.get((tuple(feature_cols), bool(guess0), int(odometry_coupled), int(radar_raw), int(augment), bool(cascaded)))
        return "" if k is None else cls.NAMES[k]

    def settings(self):
        """The named combinations present in the table, in the script's product order (:96-111), each a dict with its name,
        its settings, `rows` (the table rows of the combination) and `train` (those of guess 0 with `prediction pos ok` and
        id_from != id_to, :115-118)."""
        t = self.table
        uniq = lambda k: list(dict.fromkeys(np.asarray(t[k]).tolist()))
        out = []
        for guess0 in (True, False):
            for raw in uniq(self.RAW):
                for coupled in uniq(self.COUPLED):
                    for augment in uniq(self.AUGMENT):
                        for cols in self.FEATURE_COLS_ALL:
                            for cascaded in (True, False):
                                name = self.settings_name(cols, guess0, raw, augment, coupled, cascaded)
                                if not name:
                                    continue
                                rows = np.flatnonzero((t[self.COUPLED] == coupled) & (t[self.RAW] == raw) & (t[self.AUGMENT] == augment))
                                g0 = rows[t["guess_nr"][rows] == 0]
                                train = g0[(t["prediction pos ok"][g0] == 1) & (t["id_from"][g0] != t["id_to"][g0])]
                                out.append(dict(name=name, feature_cols=list(cols), guess0=guess0, cascaded=cascaded, rows=rows,
                                                guess0_rows=g0, train=train))
        return out

    def _features(self, cols):
        """The columns `cols` as one [rows, len(cols)] array; the same object for the same columns, so that the models
        that read it share one upload."""
        cache = self.__dict__.setdefault("_feature_cache", {})
        if tuple(cols) not in cache:
            cache[tuple(cols)] = np.ascontiguousarray(np.stack([np.asarray(self.table[c], np.float64) for c in cols], 1))
        return cache[tuple(cols)]

    def model_jobs(self, settings):
        """The logreg_fit_batch jobs of `settings` -> (jobs, where): where[i] = (setting index, "single" | "sc" | "align")."""
        y = np.asarray(self.table["is loop"], np.float64)
        jobs, where = [], []
        n = len(y)
        for s, st in enumerate(settings):
            mask = np.zeros(n, np.uint8)
            mask[st["train"]] = 1
            models = [("sc", ["odom-bounds", "sc-sim"]), ("align", ["alignment_quality"])] if st["cascaded"] else [("single", st["feature_cols"])]
            for kind, cols in models:
                jobs.append(dict(X=self._features(cols), y=y, row_mask=mask))
                where.append((s, kind))
        return jobs, where

    @staticmethod
    def _linear(X, m):
        return X @ np.asarray(m["coef"][:X.shape[1]], np.float64) + float(m["intercept"])

    def scores(self, settings, models, where):
        """(y, y_prob, pos_ok, rows) per setting from the fitted records: probabilities 1 / (1 + exp(-z)); for setting 8 the
        row of the highest probability among the nr_guess rows of every query, the first maximum winning (:133-141); for
        setting 7 the first classifier's predict() (z > 0) times the second's probability (:151-154); y_prob = probability x
        `prediction pos ok`."""
        t = self.table
        by = {w: m for w, m in zip(where, models)}
        out = []
        for s, st in enumerate(settings):
            sel = st["guess0_rows"]
            if not st["guess0"]:
                m = by[(s, "single")]
                rows = st["rows"]
                nr_guess = int(np.asarray(t["guess_nr"])[rows].max()) + 1
                p_all = 1.0 / (1.0 + np.exp(-self._linear(self._features(st["feature_cols"])[rows], m)))
                M = p_all.reshape(-1, nr_guess)
                sel = rows[np.arange(0, rows.shape[0], nr_guess) + np.argmax(M, axis=1)]
            if st["cascaded"]:
                z_sc = self._linear(self._features(["odom-bounds", "sc-sim"])[sel], by[(s, "sc")])
                z_al = self._linear(self._features(["alignment_quality"])[sel], by[(s, "align")])
                proba = (z_sc > 0.0).astype(np.float64) * (1.0 / (1.0 + np.exp(-z_al)))
            else:
                proba = 1.0 / (1.0 + np.exp(-self._linear(self._features(st["feature_cols"])[sel], by[(s, "single")])))
            y_prob = proba * t["prediction pos ok"][sel]
            out.append((t["is loop"][sel].astype(np.uint8), y_prob, np.asarray(t["candidate close"][sel]).astype(np.uint8), sel))
        return out

    def evaluate(self, models=None, curves=None, **curve_params):
        """All settings: one logreg_fit_batch call (unless `models`, the records of an earlier call, are given), then one
        loop_curves call.  Returns a list of dicts: name, models (the setting's fitted records), rows, y, y_prob, and the
        loop_curves() entries.  A setting whose training rows hold one class only raises ValueError, as sklearn does in the
        script."""
        settings = self.settings()
        jobs, where = self.model_jobs(settings)
        if models is None:
            models = logreg_fit_batch(jobs, self.ctx, class_weight_balanced=0) if jobs else np.zeros(0, L.LOGREG_RESULT_DTYPE)
        for (s, kind), m in zip(where, models):
            if m["status"] != L.OK:
                raise ValueError("%s: the %s classifier could not be fitted (status %d)" % (settings[s]["name"], kind, m["status"]))
        sc = self.scores(settings, models, where)
        curve_params.setdefault("p_threshold", self.p_threshold)
        cv = loop_curves([(y, p, ok) for y, p, ok, _ in sc], self.ctx, curves, **curve_params)
        out = []
        for s, st in enumerate(settings):
            d = dict(cv[s], name=st["name"], rows=sc[s][3], y=sc[s][0], y_prob=sc[s][1],
                     models=[m for (k, _), m in zip(where, models) if k == s])
            out.append(d)
        self.models_ = models
        return out


# ------------------------------------------------------------------------------------------------
# finishing a batch of pose graphs: PoseGraph::Align, SaveGraphString, OutputGraph and the maps of
# PoseGraphVis::ProcessFrame (tbv_slam/src/tbv_slam/posegraph.cpp:177-263, 539-584)
# ------------------------------------------------------------------------------------------------
def _finish_graph_arrays(graph, where):
    """One graph -> (poses [n, 7], gt [n, 7], has_gt [n] uint8).  A graph is a PoseGraph, a list of LoadSimpleGraph node dicts,
    or a (poses, gt, has_gt) tuple: poses [n, 7] (p, q) or [n, 3] (x, y, theta), gt likewise or None, has_gt [n] or None (all
    nodes have ground truth when gt is given)."""
    if isinstance(graph, PoseGraph):
        return graph.poses, graph.gt, graph.has_gt
    if isinstance(graph, (list, tuple)) and len(graph) and isinstance(graph[0], dict):
        ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
        poses = [nd["T"] for nd in graph]
        gt = [ident if nd.get("Tgt") is None else nd["Tgt"] for nd in graph]
        has = [bool(nd.get("has_Tgt", False)) for nd in graph]
    else:
        if len(graph) not in (1, 2, 3):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: node dicts, a PoseGraph or a (poses, gt, has_gt) tuple is needed" % where)
        poses, gt, has = graph[0], (graph[1] if len(graph) > 1 else None), (graph[2] if len(graph) > 2 else None)

    def seven(a, name):
        a = np.asarray(a, np.float64)
        if a.ndim != 2 or a.shape[1] not in (3, 7):
            raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: %s must be [n, 7] (p, q) or [n, 3] (x, y, theta), got %s" % (where, name, a.shape))
        if a.shape[1] == 3:
            a = np.array([np.concatenate(pose3d_from_xyt(p)) for p in a]).reshape(-1, 7)
        return np.ascontiguousarray(a)
    poses = seven(np.zeros((0, 7)) if len(poses) == 0 else poses, "poses")
    n = poses.shape[0]
    if gt is None:
        gt = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (n, 1))
        has = np.zeros(n, np.uint8) if has is None else has
    else:
        gt = seven(np.zeros((0, 7)) if len(gt) == 0 else gt, "gt")
    has = np.ones(n, np.uint8) if has is None else (np.asarray(has).reshape(-1) != 0).astype(np.uint8)
    if gt.shape[0] != n or has.shape[0] != n:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "%s: %d poses, %d ground-truth poses, %d flags" % (where, n, gt.shape[0], has.shape[0]))
    return poses, np.ascontiguousarray(gt), np.ascontiguousarray(has)


def _finish_batch(graphs):
    arrs = [_finish_graph_arrays(g, "graph %d" % k) for k, g in enumerate(graphs)]
    off = np.concatenate([[0], np.cumsum([a[0].shape[0] for a in arrs])]).astype(np.int64)
    cat = lambda k, shape, dt: (np.ascontiguousarray(np.concatenate([a[k] for a in arrs], 0)) if arrs else np.zeros(shape, dt))
    return cat(0, (0, 7), np.float64), cat(1, (0, 7), np.float64), cat(2, (0,), np.uint8), off


def graph_align_batch(graphs, ctx=None):
    """cfear_graph_align_batch: PoseGraph::Align (posegraph.cpp:235-263) for every graph of `graphs` (PoseGraph objects,
    LoadSimpleGraph node lists or (poses, gt, has_gt) tuples, see PoseGraph) in ONE device call.  Returns a list of
    (poses [n, 7], summary) in the order given; summary: dict(align [3, 4] = the transform every pose was left-multiplied by,
    ate = the mean distance to the ground truth afterwards, n_gt, status).  A graph whose ground-truth positions lie on one
    line keeps its poses and reports status L.ERR_SOLVER; the others are not affected.  PoseGraph objects are NOT updated
    (PoseGraph.Align does that)."""
    poses, gt, has, off = _finish_batch(graphs)
    summ = np.zeros(len(off) - 1, L.GRAPH_ALIGN_SUMMARY_DTYPE)
    ctx = ctx or default_context()
    ctx.check(ctx._lib.cfear_graph_align_batch(ctx.h, poses.ctypes.data, gt.ctypes.data, has.ctypes.data, off.ctypes.data, int(off[-1]),
                                               len(off) - 1, summ.ctypes.data))
    return [(poses[off[g]:off[g + 1]].copy(),
             dict(align=s["align"].reshape(3, 4).copy(), ate=float(s["ate"]), n_gt=int(s["n_gt"]), status=int(s["status"])))
            for g, s in enumerate(summ)]


def graph_map_batch(graphs, clouds=None, skip_frames=1, want_gt_map=True, ctx=None, device_out=False):
    """cfear_graph_map_batch: the maps PoseGraphVis::ProcessFrame builds (posegraph.cpp:539-584) for every graph of `graphs` in
    ONE device call: the cloud_peaks_ of every skip_frames-th node carried into the world by the node's pose, and, with
    want_gt_map, the same points of the nodes with ground truth carried by Tgt.  clouds: per graph a list of float32 [k, 4]
    arrays, one per node (None: the graphs' own clouds -- PoseGraph.clouds or the node dicts' cloud_peaks); when every cloud
    is a torch CUDA tensor the node arrays are uploaded too and the call reads device memory.  device_out: the maps are torch
    CUDA tensors.  Returns (map [N, 4], map_gt [M, 4] or None, summaries): graph g's points are
    map[summaries[g]["map_offset"]:][:summaries[g]["map_points"]], likewise map_gt_offset / map_gt_points."""
    poses, gt, has, off = _finish_batch(graphs)
    if clouds is None:
        clouds = []
        for g in graphs:
            if isinstance(g, PoseGraph):
                clouds.append(g.clouds)
            elif isinstance(g, (list, tuple)) and len(g) and isinstance(g[0], dict):
                clouds.append([np.zeros((0, 4), np.float32) if nd.get("cloud_peaks") is None else
                               (nd["cloud_peaks"]["xyzi"] if isinstance(nd["cloud_peaks"], dict) else nd["cloud_peaks"]) for nd in g])
            else:
                clouds.append(None)
    if len(clouds) != len(off) - 1 or any(c is None or len(c) != off[g + 1] - off[g] for g, c in enumerate(clouds)):
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "clouds must hold one [k, 4] array per node of every graph")
    flat = [c for per_graph in clouds for c in per_graph]
    device_in = bool(flat) and all(_is_torch(c) for c in flat)
    if any(_is_torch(c) for c in flat) and not device_in:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "the clouds must all be torch CUDA tensors or all be host arrays")
    coff = np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in flat])]).astype(np.int64)
    ctx = ctx or default_context()
    if device_in or device_out:
        import torch
    if device_in:
        for c in flat:
            if c.dtype != torch.float32 or not c.is_cuda or c.dim() != 2 or c.shape[1] != 4:
                raise L.CfearError(L.ERR_INVALID_ARGUMENT, "float32 [k, 4] CUDA tensors are needed, got %s %s on %s" % (c.dtype, tuple(c.shape), c.device))
        xyzi = torch.cat(flat).contiguous()
        d_poses, d_gt, d_has = (torch.from_numpy(a).to(xyzi.device) for a in (poses, gt, has))
        node_ptrs = (d_poses.data_ptr(), d_gt.data_ptr(), d_has.data_ptr())
        _torch_ready(ctx, xyzi, d_poses, d_gt, d_has)
    else:
        xyzi = (np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 4) for c in flat], 0)) if flat
                else np.zeros((0, 4), np.float32))
        node_ptrs = (poses.ctypes.data, gt.ctypes.data, has.ctypes.data)
    par = L.GraphMapParams(int(skip_frames), int(bool(want_gt_map)))
    summ = np.zeros(len(off) - 1, L.GRAPH_MAP_SUMMARY_DTYPE)

    def call(m, mg):
        return ctx._lib.cfear_graph_map_batch(ctx.h, node_ptrs[0], node_ptrs[1], node_ptrs[2], off.ctypes.data, int(off[-1]), len(off) - 1,
                                              _ptr(xyzi)[0], coff.ctypes.data, int(coff[-1]), C.byref(par), _ptr(m)[0],
                                              0 if m is None else int(m.shape[0]), _ptr(mg)[0], 0 if mg is None else int(mg.shape[0]),
                                              summ.ctypes.data)
    ctx.check(call(None, None), allowed=(L.ERR_CAPACITY,))            # the sizes
    n_map, n_gt = int(summ["map_points"].sum()), int(summ["map_gt_points"].sum())
    if device_out:
        dev = xyzi.device if device_in else torch.device("cuda", ctx.device)
        m = torch.zeros((n_map, 4), dtype=torch.float32, device=dev)
        mg = torch.zeros((n_gt, 4), dtype=torch.float32, device=dev) if want_gt_map else None
        _torch_ready(ctx, m, mg)
    else:
        m = np.zeros((n_map, 4), np.float32)
        mg = np.zeros((n_gt, 4), np.float32) if want_gt_map else None
    ctx.check(call(m, mg))
    return m, mg, summ


def SaveGraphString(path, poses, stamps):
    """PoseGraph::SaveGraphString (posegraph.cpp:177-187): per node the 12 numbers of its pose matrix with 6 decimals, a space,
    the stamp, and an empty line after every node line.  poses [n, 7] (p, q) or [n, 3]; stamps [n] unsigned integers."""
    poses = _finish_graph_arrays((poses,), "SaveGraphString")[0]
    stamps = np.ascontiguousarray(stamps, np.uint64).reshape(-1)
    if stamps.shape[0] != poses.shape[0]:
        raise L.CfearError(L.ERR_INVALID_ARGUMENT, "SaveGraphString(%s): %d stamps for %d poses" % (path, stamps.shape[0], poses.shape[0]))
    rc = L.lib().cfear_graph_string_write(os.fsencode(path), poses.ctypes.data, stamps.ctypes.data, poses.shape[0])
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_graph_string_write(%s)" % path)


def OutputGraph(est_path, gt_path, poses, gt=None, has_gt=None):
    """PoseGraph::OutputGraph (posegraph.cpp:201-234): the poses of the nodes with ground truth to est_path and their Tgt to
    gt_path, one KITTI line each; when no node has ground truth, every pose to est_path and an empty gt_path."""
    poses, gt, has = _finish_graph_arrays((poses, gt, has_gt), "OutputGraph")
    rc = L.lib().cfear_graph_output_write(os.fsencode(est_path), os.fsencode(gt_path), poses.ctypes.data, gt.ctypes.data, has.ctypes.data,
                                          poses.shape[0])
    if rc != L.OK:
        raise L.CfearError(rc, "cfear_graph_output_write(%s, %s)" % (est_path, gt_path))


class PoseGraph:
    """The end of tbv_slam's PoseGraph (posegraph.h) over the calls above: Align(), SaveGraphString(path), OutputGraph() and
    Map().  Fed by LoadSimpleGraph's node dicts (nodes=...), or by arrays: poses [n, 7] as pose_graph_optimize_batch returns
    them (or [n, 3] planar), gt likewise, has_gt [n], stamps [n], clouds = one float32 [k, 4] peak cloud per node.
    est_output_dir / gt_output_dir are PoseGraph::Parameters'; OutputGraph writes <dir>/00.txt into each."""

    def __init__(self, nodes=None, poses=None, gt=None, has_gt=None, stamps=None, clouds=None, est_output_dir=".", gt_output_dir=".",
                 ctx=None):
        if nodes is not None:
            self.poses, self.gt, self.has_gt = _finish_graph_arrays(list(nodes), "PoseGraph")
            stamps = [int(nd.get("stamp", 0)) for nd in nodes] if stamps is None else stamps
            if clouds is None:
                clouds = [np.zeros((0, 4), np.float32) if nd.get("cloud_peaks") is None else
                          (nd["cloud_peaks"]["xyzi"] if isinstance(nd["cloud_peaks"], dict) else nd["cloud_peaks"]) for nd in nodes]
        else:
            self.poses, self.gt, self.has_gt = _finish_graph_arrays((poses, gt, has_gt), "PoseGraph")
        n = self.poses.shape[0]
        self.stamps = np.zeros(n, np.uint64) if stamps is None else np.ascontiguousarray(stamps, np.uint64).reshape(-1)
        self.clouds = [np.zeros((0, 4), np.float32)] * n if clouds is None else list(clouds)
        self.est_output_dir, self.gt_output_dir, self.ctx = est_output_dir, gt_output_dir, ctx
        self.Tgtalign, self.ate = None, None

    def size(self):
        return self.poses.shape[0]

    def Align(self):
        """PoseGraph::Align: the poses are replaced; returns the summary (graph_align_batch), kept as Tgtalign / ate too."""
        (poses, s), = graph_align_batch([self], self.ctx)
        self.poses, self.Tgtalign, self.ate = poses, s["align"], s["ate"]
        return s

    def SaveGraphString(self, path):
        SaveGraphString(path, self.poses, self.stamps)

    def OutputGraph(self):
        for d in (self.est_output_dir, self.gt_output_dir):
            os.makedirs(d, exist_ok=True)
        OutputGraph(os.path.join(self.est_output_dir, "00.txt"), os.path.join(self.gt_output_dir, "00.txt"), self.poses, self.gt, self.has_gt)

    def Map(self, skip_frames=1, want_gt_map=True, device_out=False):
        """The maps of PoseGraphVis::ProcessFrame -> (map [N, 4], map_gt [M, 4] or None)."""
        m, mg, _ = graph_map_batch([self], None, skip_frames, want_gt_map, self.ctx, device_out)
        return m, mg
