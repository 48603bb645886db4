"""Timing probe of cfear_polar_to_cartesian and cfear_cart_quality_batch: 400 x 3360 synthetic sweeps resident on the device,
W = 300 (the reference's geometry), at every batch size given; a quality job scores sweep k against sweep k - 1 at one of
scanEvaluator's three offsets.  ms per call from device events around back-to-back calls (median of --reps after --warmup),
the library's own kernel event times, and the NumPy definition (tests/cart_cpu.py) on ONE sweep and ONE job of the same
input for comparison (its maps are built once, outside the timed part, as the library's are).

  python tools/cart_probe.py --batch 1 64 1024 --reps 7"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(call, reps, warmup, torch):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        call()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth
    from tests import cart_cpu as R, p2p_cpu
    imgs, _gt, _ = synth.scene_v1(3, 8)
    base = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    ctx = api.default_context()
    vek = p2p_cpu.create_perturbations()
    out = dict(rows=int(base.shape[1]), cols=int(base.shape[2]), W=R.CART_PIXEL_WIDTH, batch={})
    for b in a.batch:
        sweeps = base[torch.arange(b, device="cuda") % base.shape[0]].contiguous()
        row = {}
        carts = api.polar_to_cartesian(sweeps, ctx=ctx)
        jobs = [(carts[k], carts[k - 1] if k else carts[b - 1], api.cart_pose_offset((0.0, 0.0, 0.0), vek[k % len(vek)])) for k in range(b)]
        calls = {"polar_to_cartesian": lambda: api.polar_to_cartesian(sweeps, ctx=ctx),
                 "cart_quality": lambda: api.cart_quality_batch(jobs, R.CART_RESOLUTION, ctx=ctx, device_out=True)}
        for name, call in calls.items():
            ms = _timed(call, a.reps, a.warmup, torch)
            ctx.profile_enable(True)
            call()
            torch.cuda.synchronize()
            prof = ctx.profile_read()
            ctx.profile_enable(False)
            row[name] = dict(ms_per_call=float(np.median(ms)), ms_all=ms, kernel_event_ms={k: v[0] for k, v in prof.items()})
        res = api.cart_quality_batch(jobs, R.CART_RESOLUTION, ctx=ctx)[0]
        row["failed"] = int((res["status"] != 0).sum())
        out["batch"]["%d" % b] = row
    if not a.no_cpu:
        t0 = time.perf_counter()
        maps = R.fixed_maps(imgs.shape[1], R.CART_PIXEL_WIDTH)
        t1 = time.perf_counter()
        c0, c1 = R.polar_to_cartesian(imgs[0], maps=maps), R.polar_to_cartesian(imgs[1], maps=maps)
        t2 = time.perf_counter()
        q = R.quality(c0, c1, *R.pose_offset((0.0, 0.0, 0.0), vek[1]), R.CART_RESOLUTION)[0]
        t3 = time.perf_counter()
        got = api.cart_quality_batch([(api.polar_to_cartesian(imgs[1], ctx=ctx), api.polar_to_cartesian(imgs[0], ctx=ctx),
                                       api.cart_pose_offset((0.0, 0.0, 0.0), vek[1]))], R.CART_RESOLUTION, ctx=ctx)[0]
        out["numpy_definition"] = dict(maps_ms=(t1 - t0) * 1e3, polar_to_cartesian_ms_per_sweep=(t2 - t1) * 5e2, quality_ms_per_job=(t3 - t2) * 1e3,
                                       abs_diff=q, abs_diff_gpu=float(got[0]["abs_diff"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
