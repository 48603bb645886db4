"""Timing probe of cfear_cen2019_order_audit beside cfear_filter_cen2019 on the same device-resident batch: ms per batch
(device events around back-to-back calls) and the library's own per-kernel event times, at max_points 1000 and 10000.  The
audit runs the filter's kernel chain twice (this library's order and the reversed witness) and a bracket pass of its own.

  python tools/cen2019_audit_probe.py --batch 64 --reps 5
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-points", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--cap", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth
    base = torch.from_numpy(np.ascontiguousarray(synth.scene_v1(3, 8)[0])).cuda()          # [8, 400, 3360]
    imgs = torch.cat([torch.roll(base, shifts=k, dims=1) for k in range((a.batch + 7) // 8)])[:a.batch].contiguous()   # every sweep differs
    torch.cuda.synchronize()
    ctx = api.default_context()

    def timed(call):
        for _ in range(a.warmup):
            res = call()
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        call()
        torch.cuda.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
        ev[0].record()
        for i in range(a.reps):
            res = call()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
        return res, float(np.median(ms)), ms, {k: v[0] for k, v in prof.items()}

    for mp in a.max_points:
        _, f_ms, f_all, f_prof = timed(lambda: api.filter_cen2019(imgs, max_points=mp, cap_points=a.cap, want_targets=True))
        _, r_ms, r_all, r_prof = timed(lambda: api.cen2019_order_audit(imgs, max_points=mp))
        res, t_ms, t_all, _ = timed(lambda: api.cen2019_order_audit(imgs, max_points=mp, cap_points=a.cap, want_targets=True, want_marks=True))
        rec = res["records"]
        print(json.dumps(dict(batch=a.batch, rows=int(imgs.shape[1]), cols=int(imgs.shape[2]), max_points=mp,
                              filter_ms=f_ms, filter_ms_all=f_all, audit_records_ms=r_ms, audit_records_ms_all=r_all,
                              audit_all_outputs_ms=t_ms, audit_all_outputs_ms_all=t_all, audit_over_filter=r_ms / f_ms,
                              clear=int((rec["n_marks_in"] == rec["n_marks_out"]).sum()), band=int(rec["n_band"].sum()),
                              targets=int(rec["n_targets"].sum()), certain=int(rec["n_targets_certain"].sum()),
                              filter_kernel_event_ms=f_prof, audit_kernel_event_ms=r_prof)))


if __name__ == "__main__":
    main()
