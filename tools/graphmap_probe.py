#!/usr/bin/env python
"""Times cfear_graph_map_batch (csrc/graphfinish.hip) at a realistic size, everything in device memory:
  --graphs 64 x --nodes 2000 x --peaks 1500 points per node, every node with ground truth, skip_frames 1
once with the ground-truth map (48 bytes moved per point: one 16-byte load, two 16-byte stores) and once without (32).
Per variant one warm-up call, then --reps calls, each followed by the yardstick: torch's device-to-device copy of the cloud
into the map (and into the ground-truth map for the first variant: it reads the source twice, 64 bytes per point), so the two
alternate under the same conditions.  Reported: the device time of graph_map_kernel from the context's hipEvent profile, the
host clock around the whole call (has_gt read back, offset arithmetic, table upload, kernel, synchronise), the copies' device
time from torch events, the bytes each moves and the rate, and the fraction of the 8 TB/s HBM peak.  Graph 0's maps are
compared with the NumPy restatement (tests/graphfinish_cpu.py) while at it.
    python tools/graphmap_probe.py [--graphs 64] [--nodes 2000] [--peaks 1500] [--reps 5] [--json out.json]"""
import argparse
import ctypes as C
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

import graphfinish_cpu as G  # noqa: E402
from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api  # noqa: E402

PEAK_TBS = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--peaks", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = api.default_context()
    lib = ctx._lib
    dev = torch.device("cuda:0")
    n_nodes, n_points = a.graphs * a.nodes, a.graphs * a.nodes * a.peaks
    rng = np.random.default_rng(3)

    def random_poses(n):
        q = rng.normal(size=(n, 4)) * [0.05, 0.05, 1.0, 1.0]              # mostly yaw, some roll and pitch
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        return np.ascontiguousarray(np.concatenate([rng.uniform(-500, 500, (n, 2)), rng.uniform(-2, 2, (n, 1)), q], 1))
    poses, gt = random_poses(n_nodes), random_poses(n_nodes)
    d_poses, d_gt = torch.from_numpy(poses).to(dev), torch.from_numpy(gt).to(dev)
    d_has = torch.ones(n_nodes, dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(4)
    xyzi = (torch.rand((n_points, 4), generator=g, device=dev, dtype=torch.float32) - 0.5) * 300.0
    m = torch.zeros((n_points, 4), dtype=torch.float32, device=dev)
    mg = torch.zeros((n_points, 4), dtype=torch.float32, device=dev)
    off = (np.arange(a.graphs + 1, dtype=np.int64) * a.nodes)
    coff = (np.arange(n_nodes + 1, dtype=np.int64) * a.peaks)
    summ = np.zeros(a.graphs, L.GRAPH_MAP_SUMMARY_DTYPE)
    torch.cuda.synchronize()
    res = dict(graphs=a.graphs, nodes=a.nodes, peaks=a.peaks, points=n_points, reps=a.reps, peak_tbs=PEAK_TBS, variants={})
    for name, want_gt in (("with_gt_map", 1), ("map_only", 0)):
        par = L.GraphMapParams(1, want_gt)

        def call():
            t0 = time.perf_counter()
            ctx.check(lib.cfear_graph_map_batch(ctx.h, d_poses.data_ptr(), d_gt.data_ptr(), d_has.data_ptr(), off.ctypes.data, n_nodes, a.graphs,
                                                xyzi.data_ptr(), coff.ctypes.data, n_points, C.byref(par), m.data_ptr(), n_points,
                                                mg.data_ptr(), n_points, summ.ctypes.data))
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def copies():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.copy_(xyzi)
            if want_gt:
                mg.copy_(xyzi)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        call()                                                                 # warm-up: workspace, pinned staging, code load
        copies()
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        call_ms, kern_ms, copy_ms = [], [], []
        for _ in range(a.reps):
            call_ms.append(call())
            prof = ctx.profile_read(reset=True)
            kern_ms.append(prof["graph_map"][0])
            copy_ms.append(copies())
        ctx.profile_enable(False)
        call()                                                                 # the maps the check below reads: the copies overwrote them
        moved = n_points * (32 + 16 * want_gt)
        copied = n_points * 32 * (1 + want_gt)
        k, c = statistics.median(kern_ms), statistics.median(copy_ms)
        # graph 0's first and last node against the restatement
        ok = True
        for node in (0, a.nodes - 1):
            sl = slice(node * a.peaks, (node + 1) * a.peaks)
            cloud = xyzi[sl].cpu().numpy()
            ok = ok and m[sl].cpu().numpy().tobytes() == G.transform_cloud(G.to_rows(poses[node]), cloud).tobytes()
            if want_gt:
                ok = ok and mg[sl].cpu().numpy().tobytes() == G.transform_cloud(G.to_rows(gt[node]), cloud).tobytes()
        r = dict(kernel_ms_median=round(k, 4), kernel_ms_all=[round(x, 4) for x in kern_ms], call_ms_median=round(statistics.median(call_ms), 3),
                 call_ms_all=[round(x, 3) for x in call_ms], bytes_moved=moved, kernel_tbs=round(moved / k / 1e9, 3),
                 fraction_of_peak=round(moved / k / 1e9 / PEAK_TBS, 4), copy_ms_median=round(c, 4), copy_ms_all=[round(x, 4) for x in copy_ms],
                 copy_bytes_moved=copied, copy_tbs=round(copied / c / 1e9, 3), kernel_over_copy=round(k / c, 3),
                 map_points=int(summ["map_points"].sum()), map_gt_points=int(summ["map_gt_points"].sum()), equals_restatement=bool(ok))
        res["variants"][name] = r
        print("%-12s %d points: kernel %.3f ms (median of %d), %.2f GB moved -> %.2f TB/s = %.1f %% of %.0f TB/s; whole call %.2f ms; "
              "device-to-device copy %.3f ms for %.2f GB -> %.2f TB/s; kernel / copy %.2f; equals the restatement: %s"
              % (name, n_points, k, a.reps, moved / 1e9, r["kernel_tbs"], 100 * r["fraction_of_peak"], PEAK_TBS, r["call_ms_median"], c,
                 copied / 1e9, r["copy_tbs"], r["kernel_over_copy"], ok), flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
