"""Timing probe of cfear_filter_cen2018 on device-resident sweeps: ms per batch and sweeps/s (device events around
back-to-back calls), the library's own per-kernel event times, and the two bounds a batch has on the MI355X -- fp32 VALU
issue for the tap sums and HBM for reading the sweeps once.

  python tools/cen2018_probe.py --batch 4096 --cols 3360 --reps 5

Run it under `rocprofv3 --kernel-trace --stats -- python tools/cen2018_probe.py ... --reps 2 --no-profile` for the kernels'
share of the time."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_INSTR = 157.3e12 / 2          # fp32 VALU operations per second when every one is an FMA counted as two: 78.6e12 lanes-ops/s
PEAK_HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--cols", type=int, default=3360)
    ap.add_argument("--sigma-gauss", type=int, default=17)
    ap.add_argument("--zq", type=float, default=3.0)
    ap.add_argument("--cap", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth
    base = torch.from_numpy(np.ascontiguousarray(synth.scene_v1(3, 8)[0])).cuda()          # [8, 400, 3360]
    imgs = torch.zeros((a.batch, a.rows, a.cols), dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    imgs.random_(0, 24, generator=g)                                                         # noise floor, tail of wide sweeps
    c = min(a.cols, base.shape[2])
    r = min(a.rows, base.shape[1])
    for b0 in range(0, a.batch, 8):
        n = min(8, a.batch - b0)
        imgs[b0:b0 + n, :r, :c] = torch.roll(base[:n, :r, :c], shifts=b0 // 8, dims=1)      # every sweep differs
    torch.cuda.synchronize()
    ctx = api.default_context()
    kw = dict(zq=a.zq, sigma_gauss=a.sigma_gauss, cap_points=a.cap)
    for _ in range(a.warmup):
        res = api.filter_cen2018(imgs, **kw)
    torch.cuda.synchronize()
    if not a.no_profile:
        ctx.profile_enable(True)
        api.filter_cen2018(imgs, **kw)
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
    else:
        prof = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
    ev[0].record()
    for i in range(a.reps):
        res = api.filter_cen2018(imgs, **kw)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
    med = float(np.median(ms))
    fsize = 3 * a.sigma_gauss
    bins = a.batch * a.rows * a.cols
    tap_ops = 2.0 * bins * fsize                 # one multiply and one add per tap and bin (no FMA: the reference has none)
    image_bytes = float(bins)
    t_valu = tap_ops / PEAK_FP32_INSTR
    t_hbm = image_bytes / PEAK_HBM
    out = dict(batch=a.batch, rows=a.rows, cols=a.cols, sigma_gauss=a.sigma_gauss, ms_per_batch=med, ms_all=ms,
               sweeps_per_s=a.batch / (med * 1e-3), mean_points=float(res["n_points"].float().mean()),
               max_points=int(res["n_points"].max()), tap_ops=tap_ops, image_bytes=image_bytes,
               valu_bound_ms=t_valu * 1e3, hbm_bound_ms=t_hbm * 1e3,
               fraction_of_fp32_valu_issue=t_valu / (med * 1e-3), fraction_of_hbm_bandwidth=t_hbm / (med * 1e-3),
               kernel_event_ms={k: v[0] for k, v in prof.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
