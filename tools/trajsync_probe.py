#!/usr/bin/env python
"""Times cfear_sync_trajectories (csrc/trajsync.hip) on device buffers, in chained mode, on two workloads:
  batch   4096 pairs x 2048 estimates (4 Hz) against 16 384 ground-truth poses each (32 Hz)
  long    one pair of 8865 estimates (4 Hz; Oxford's longest sequence) against 110 000 ground-truth poses (50 Hz)
The ground truth starts after the first sweep and ends before the last, so both ends drop estimates.  Times are host
clocks around the C call on torch tensors made beforehand (the call returns when the counts are in host memory); per
workload one warm-up call, then --reps calls; best, median and the whole list, and the device time of the kernels from
the context's hipEvent profile of one extra call.  The yardstick is the bytes the call must move -- per estimate its
stamp, per kept estimate its pose, the two ground-truth poses and stamps it interpolates, and the four output rows -- over
the HBM rate of bench.py's roofline entry (--hbm-tbs).  The range scratch the kernels pass between them is listed apart.
Pair 0's rows are compared with the serial restatement (tests/trajsync_cpu.py) while at it.
    python tools/trajsync_probe.py [--reps 7] [--pairs 4096] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import trajsync_cpu as M  # noqa: E402
from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api  # noqa: E402


def planar(x, y, th):
    z, o = torch.zeros_like(x), torch.ones_like(x)
    c, s = torch.cos(th), torch.sin(th)
    return torch.stack([c, -s, z, x, s, c, z, y, z, z, o, z], -1).reshape(-1, 12).contiguous()


def workload(n_pairs, n_est, n_gt, gt_step_ns, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    start = torch.randint(0, 10 ** 9, (n_pairs, 1), generator=g, device=dev, dtype=torch.int64) + M.T0
    es = (start + torch.arange(n_est, device=dev, dtype=torch.int64)[None, :] * 250_000_000).reshape(-1).contiguous()
    gs = (start + 300_000_000 + torch.arange(n_gt, device=dev, dtype=torch.int64)[None, :] * gt_step_ns).reshape(-1).contiguous()

    def path(n, dt):
        th = torch.cumsum(torch.randn((n_pairs, n), generator=g, device=dev, dtype=torch.float64) * 0.02 * dt ** 0.5, 1)
        x, y = torch.cumsum(10.0 * dt * torch.cos(th), 1), torch.cumsum(10.0 * dt * torch.sin(th), 1)
        return planar(x.reshape(-1), y.reshape(-1), th.reshape(-1))
    return path(n_est, 0.25), es, path(n_gt, gt_step_ns * 1e-9), gs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--hbm-tbs", type=float, default=5.68, help="HBM rate of bench.py's roofline entry, TB/s")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = api.default_context()
    lib = ctx._lib
    dev = torch.device("cuda:0")
    res = dict(reps=a.reps, hbm_tbs=a.hbm_tbs, workloads={})
    for name, (n_pairs, n_est, n_gt, step) in {"batch": (a.pairs, 2048, 16384, 31_250_000), "long": (1, 8865, 110000, 20_000_000)}.items():
        est, es, gt, gs = workload(n_pairs, n_est, n_gt, step, dev)
        n = n_pairs * n_est
        est_out, gt_out = torch.zeros((n, 12), dtype=torch.float64, device=dev), torch.zeros((n, 12), dtype=torch.float64, device=dev)
        s_out, rows = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros((n, 16), dtype=torch.uint8, device=dev)
        le, lg = np.full(n_pairs, n_est, np.int32), np.full(n_pairs, n_gt, np.int32)
        counts = np.zeros(n_pairs, np.int32)
        torch.cuda.synchronize()

        def call():
            t0 = time.perf_counter()
            ctx.check(lib.cfear_sync_trajectories(ctx.h, L.SYNC_MODE["chained"], est.data_ptr(), es.data_ptr(), None, le.ctypes.data, gt.data_ptr(),
                                                  gs.data_ptr(), None, lg.ctypes.data, n_pairs, est_out.data_ptr(), gt_out.data_ptr(),
                                                  s_out.data_ptr(), rows.data_ptr(), counts.ctypes.data))
            return (time.perf_counter() - t0) * 1e3

        call()                                                                 # warm-up: workspace allocation, code load
        times = [call() for _ in range(a.reps)]
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        call()
        prof = ctx.profile_read(reset=True)
        ctx.profile_enable(False)
        kern = {k: round(v[0], 4) for k, v in prof.items() if k.startswith("sync_")}
        kept = int(counts.sum())
        must = n * 8 + kept * (96 + 2 * 96 + 2 * 8 + 96 + 96 + 8 + 16)
        scratch = n * 32
        want = M.sync_pair(None, es[:n_est].cpu().numpy(), gt[:n_gt].cpu().numpy(), gs[:n_gt].cpu().numpy())
        got = rows[:counts[0]].cpu().numpy().view(L.SYNC_ROW_DTYPE).reshape(-1)
        r = dict(pairs=n_pairs, estimates=n_est, ground_truth=n_gt, kept=kept, call_ms_best=round(min(times), 3),
                 call_ms_median=round(statistics.median(times), 3), call_ms_all=[round(t, 3) for t in times], kernel_ms=kern,
                 kernel_ms_sum=round(sum(kern.values()), 4), must_move_bytes=must, scratch_bytes=scratch,
                 yardstick_ms=round(must / (a.hbm_tbs * 1e12) * 1e3, 4), rows_equal_restatement=bool(got.tobytes() == want["rows"].tobytes()))
        res["workloads"][name] = r
        print("%-5s %4d x %4d estimates, %6d ground truth: kept %d; call best %.3f ms, median %.3f ms over %d; kernels (ms) %s = %.4f; "
              "must move %.1f MB -> %.4f ms at %.2f TB/s (scratch %.1f MB); pair 0 equals the restatement: %s"
              % (name, n_pairs, n_est, n_gt, kept, r["call_ms_best"], r["call_ms_median"], a.reps, kern, r["kernel_ms_sum"], must / 1e6,
                 r["yardstick_ms"], a.hbm_tbs, scratch / 1e6, r["rows_equal_restatement"]), flush=True)
        del est, es, gt, gs, est_out, gt_out, s_out, rows
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
