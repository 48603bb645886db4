"""Timing probe of cfear_p2p_quality_batch against coral_kernel on IDENTICAL jobs in one process: --jobs jobs built from the
peak clouds of consecutive synthetic sweeps (the clouds loop-closure verification scores, k = 40, z_min = 60) x the 13 TBV
perturbations, all clouds resident on the device, at every radius given.  ms per batch from device events around
back-to-back calls (median of --reps after --warmup), and the library's own kernel event times.

  python tools/p2p_probe.py --jobs 4096 --radius 3 1 --reps 7

Run it under `rocprofv3 --kernel-trace --stats -- python tools/p2p_probe.py ... --reps 2 --no-profile` for the kernels'
share of the time."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--radius", type=float, nargs="+", default=[3.0, 1.0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    from tbv_slam_public_amd import api, synth
    imgs, gt, _ = synth.scene_v1(3, a.frames)
    r = api.filter_kstrongest(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), 40, 60.0, 0.0438, 2.5, want_peaks=True)
    n = [int(v) for v in r["n_peaks"]]
    clouds = [r["xyzi_peaks"][b, :n[b]].contiguous() for b in range(a.frames)]
    vek = api.ScanLearningInterface().vek_perturbation_
    # every pair is a distinct pair of device clouds (copies), as the keyframe pairs of a sequence are
    jobs, keep = [], []
    while len(jobs) < a.jobs:
        k = 1 + (len(jobs) // len(vek)) % (a.frames - 1)
        ref, src = clouds[k - 1].clone(), clouds[k].clone()
        keep += [ref, src]
        for off in vek:
            if len(jobs) < a.jobs:
                jobs.append((ref, tuple(gt[k - 1]), src, tuple(gt[k]), off))
    torch.cuda.synchronize()
    ctx = api.default_context()
    out = dict(jobs=len(jobs), pairs=len(keep) // 2, mean_points=float(np.mean(n)), max_points=int(max(n)), radius={})
    for radius in a.radius:
        calls = {"p2p": lambda: api.p2p_quality_batch(jobs, radius, ctx=ctx), "coral": lambda: api.coral_quality_batch(jobs, radius, ctx=ctx)}
        row = {}
        for name, call in calls.items():
            for _ in range(a.warmup):
                res = call()[0]
            torch.cuda.synchronize()
            prof = {}
            if not a.no_profile:
                ctx.profile_enable(True)
                call()
                torch.cuda.synchronize()
                prof = ctx.profile_read()
                ctx.profile_enable(False)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
            ev[0].record()
            for i in range(a.reps):
                res = call()[0]
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
            row[name] = dict(ms_per_batch=float(np.median(ms)), ms_all=ms, kernel_event_ms={k: v[0] for k, v in prof.items()},
                             failed=int((res["status"] != 0).sum()))
        # the condition is on the kernels; the whole calls are dominated by the host marshalling the jobs
        row["call_p2p_over_coral"] = row["p2p"]["ms_per_batch"] / row["coral"]["ms_per_batch"]
        kp, kc = row["p2p"]["kernel_event_ms"].get("p2p_quality"), row["coral"]["kernel_event_ms"].get("coral_quality")
        row["kernel_p2p_over_coral"] = kp / kc if kp and kc else None
        out["radius"]["%g" % radius] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
