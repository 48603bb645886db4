"""Timing probe of cfear_filter_cen2019 on device-resident sweeps: ms per batch and sweeps/s (device events around
back-to-back calls) at max_points 1000 and 10000, the library's own per-kernel event times, the bytes the kernels move, and
the yardstick nobody has measured this filter against yet: the time of four HBM reads of the batch (the sweep is read by
the range, hsum, fresh and mark kernels).

  python tools/cen2019_probe.py --batch 64 --reps 5
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rows", type=int, default=400)
    ap.add_argument("--cols", type=int, default=3360)
    ap.add_argument("--max-points", type=int, nargs="+", default=[1000, 10000])
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
    pixels = a.batch * a.rows * a.cols
    words = (a.cols + 63) // 64
    for mp in a.max_points:
        kw = dict(max_points=mp, cap_points=a.cap, want_counts=True)
        for _ in range(a.warmup):
            res = api.filter_cen2019(imgs, **kw)
        torch.cuda.synchronize()
        prof = {}
        if not a.no_profile:
            ctx.profile_enable(True)
            api.filter_cen2019(imgs, **kw)
            torch.cuda.synchronize()
            prof = ctx.profile_read()
            ctx.profile_enable(False)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
        ev[0].record()
        for i in range(a.reps):
            res = api.filter_cen2019(imgs, **kw)
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
        med = float(np.median(ms))
        cnt = res["counts"].cpu().numpy().astype(np.int64)
        fresh = int(cnt[:, 1].sum())
        bitmaps = a.batch * a.rows * words * 8
        # per kernel: bytes read + written.  select reads the fresh keys once per 11-bit pass (5 passes) when the cutoff binds.
        moved = dict(cen2019_range=pixels + a.batch * a.rows * 12, cen2019_hsum=pixels + a.batch * a.rows * 8,
                     cen2019_fresh=pixels + fresh * 8 + a.batch * a.rows * 8,
                     cen2019_select=fresh * 8 * 5 if fresh >= mp * a.batch else a.batch * a.rows * 4,
                     cen2019_mark=pixels + 2 * bitmaps + a.batch * a.rows * 12, cen2019_emit=5 * bitmaps,
                     cen2019_cloud=bitmaps + int(res["n_points"].sum()) * 16)
        four_reads_ms = 4.0 * pixels / PEAK_HBM * 1e3
        out = dict(batch=a.batch, rows=a.rows, cols=a.cols, max_points=mp, ms_per_batch=med, ms_all=ms,
                   sweeps_per_s=a.batch / (med * 1e-3), ms_per_sweep=med / a.batch, mean_points=float(res["n_points"].float().mean()),
                   candidates=int(cnt[:, 0].sum()), fresh=fresh, processed=int(cnt[:, 2].sum()),
                   image_bytes=float(pixels), four_hbm_reads_ms=four_reads_ms, times_four_hbm_reads=med / four_reads_ms,
                   bytes_moved=moved, bytes_moved_total=float(sum(moved.values())),
                   kernel_event_ms={k: v[0] for k, v in prof.items()})
        print(json.dumps(out))


if __name__ == "__main__":
    main()
