#!/usr/bin/env python
"""Batched Scan Context (cfear_sc_detect_batch) against the calls it replaces, on synthetic graphs (synth.sc_graph, 600
landmark points per node, laps of a 120 m circle) with TBV's settings (40 x 120, augment_sc, odometry-coupled closure, 10
tree candidates, 3 kept), N_aggregate 1, every graph's last node not detected.  Host clocks around synchronous calls, after
one warm-up, best and median of --reps:
  cloud mode  one api.sc_detect_batch call against a loop of api.sc_detect_sequence calls over the same graphs, at
              64 graphs x 70 nodes (the demos' shape) and 8 x 512; at 1 x 4096 against the single sequence call.  The
              candidates of the two are compared and must be identical.
  raw mode    64 x 70 sweeps of 400 x 3360 (device memory) against the streaming RSCManagerNative loop (add_raw + detect).
Device times per kernel family come from the context's hipEvent profile of one extra call of each side.  The 4096-node call
is repeated once with CFEAR_OPT_HOST_TIMELINE = 1, which prints where the host spends it (stderr).
    python tools/sc_batch_probe.py [--reps 5] [--shapes 64x70,8x512,1x4096] [--no-raw] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api, synth  # noqa: E402


def _timed(fn, reps):
    fn()                                                           # warm-up: workspace, LDS attributes
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, round(min(times), 3), round(statistics.median(times), 3)


def _profile(ctx, fn):
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    fn()
    prof = ctx.profile_read(reset=True)
    ctx.profile_enable(False)
    return {k: round(v[0], 3) for k, v in prof.items() if k.startswith("sc_")}


def cloud_shape(ctx, G, n, reps):
    graphs = [synth.sc_graph(n, seed=100 + g) for g in range(G)]
    nd = [n - 1] * G
    flat = api.sc_flatten_graphs(graphs)

    def batch():
        return api.sc_detect_batch(flat=flat, n_aggregate=1, n_detect=nd, ctx=ctx)

    def loop():
        return [api.sc_detect_sequence(c, p, 1, n - 1, ctx=ctx) for c, p in graphs]

    t0 = time.perf_counter()
    api.sc_flatten_graphs(graphs)
    flatten_ms = round((time.perf_counter() - t0) * 1e3, 3)
    got, b_best, b_med = _timed(batch, reps)
    exp, l_best, l_med = _timed(loop, reps)
    assert got == exp, "the batch call and the per-graph calls disagree"
    res = dict(mode="cloud", graphs=G, nodes=n, candidates=sum(len(x) for g in got for x in g), flatten_ms=flatten_ms,
               batch_ms_best=b_best, batch_ms_median=b_med, sequence_loop_ms_best=l_best, sequence_loop_ms_median=l_med,
               ratio_median=round(l_med / b_med, 2), batch_kernels_ms=_profile(ctx, batch), sequence_kernels_ms=_profile(ctx, loop))
    if G == 1:
        ctx.set_option(L.OPT_HOST_TIMELINE, 1)
        try:
            batch()
        finally:
            ctx.set_option(L.OPT_HOST_TIMELINE, 0)
    return res


def raw_shape(ctx, G, n, reps):
    import torch
    torch.manual_seed(7)
    sweeps = torch.randint(0, 256, (G * n, 400, 3360), dtype=torch.uint8, device="cuda:%d" % ctx.device)
    poses = [synth.sc_graph(n, seed=100 + g, points=1)[1] for g in range(G)]
    raw = api.sc_raw_params(transpose=1)
    flat = api.sc_flatten_graphs([(sweeps[g * n:(g + 1) * n], poses[g]) for g in range(G)])
    flat["imgs"] = sweeps

    def batch():
        return api.sc_detect_batch(flat=flat, n_detect=[n - 1] * G, raw_par=raw, ctx=ctx)

    def stream():
        out = []
        for g in range(G):
            nat = api.RSCManagerNative(ctx=ctx, raw_par=raw)
            rows = []
            for i in range(n - 1):
                nat.makeAndSaveScancontextAndKeysRadarRaw(sweeps[g * n + i], poses[g][i])
                rows.append(nat.detectLoopClosureID())
            nat.close()
            out.append(rows)
        return out

    got, b_best, b_med = _timed(batch, reps)
    exp, s_best, s_med = _timed(stream, max(1, reps // 2))
    same = sum([c["nn_idx"] for c in a] == [c["nn_idx"] for c in b] and
               all(x["min_dist_sc"] == y["min_dist_sc"] and abs(x["min_dist"] - y["min_dist"]) <= 1e-12 for x, y in zip(a, b))
               for ga, gb in zip(got, exp) for a, b in zip(ga, gb))
    assert same == G * (n - 1), "the batch call and the streaming managers disagree"
    return dict(mode="raw", graphs=G, nodes=n, candidates=sum(len(x) for g in got for x in g), batch_ms_best=b_best,
                batch_ms_median=b_med, streaming_ms_best=s_best, streaming_ms_median=s_med, ratio_median=round(s_med / b_med, 2),
                streaming_ms_per_node=round(s_med / (G * (n - 1)), 4), batch_kernels_ms=_profile(ctx, batch))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="64x70,8x512,1x4096", help="cloud-mode shapes, graphs x nodes")
    ap.add_argument("--no-raw", action="store_true", help="skip the raw-mode comparison (64 x 70)")
    ap.add_argument("--json", default=None, help="also write the results to this file")
    a = ap.parse_args()
    ctx = api.default_context()
    results = []
    for shape in a.shapes.split(","):
        G, n = (int(v) for v in shape.split("x"))
        results.append(cloud_shape(ctx, G, n, a.reps))
        print(json.dumps(results[-1]), flush=True)
    if not a.no_raw:
        results.append(raw_shape(ctx, 64, 70, a.reps))
        print(json.dumps(results[-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
