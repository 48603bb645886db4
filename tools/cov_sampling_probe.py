#!/usr/bin/env python
"""Times covariance sampling for verified loop candidates: the device pass (api.verify_sample_covariances,
cfear_verify_sample_covariances) over the records api.verify_sc_rows left on the device, beside what sampling adds to the
host route.
  device pass    the call's total time over list and results in device memory, and its kernels by hipEvents (the context's
                 profile rows): "get_cost" = the matcher's sampling launch (27 GetCost evaluations per registered candidate),
                 "cov_fit" = cov_fit_kernel, "cov_glue" = the scan, fill, centre, expand and write kernels
  host route     the same candidates as cfear_verify_job records through cfear_verify_loop_candidates with
                 use_covariance_sampling 1 (verify_host_chain: the samples come back to the host, which fits them) and 0 (the
                 device chain); the difference is what sampling costs on that route
Candidates: those of tools/loop_closure_probe.py's case of --graphs x --nodes nodes (default 8 x 250).  Both routes see the same
candidates; their cov_sampled flags and sampled blocks are compared.
    python tools/cov_sampling_probe.py [--graphs 8] [--nodes 250] [--reps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import loop_closure_probe as P  # noqa: E402
from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api  # noqa: E402

BLOCK = np.ix_([0, 1, 5], [0, 1, 5])


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=250)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = api.default_context()
    scene = P.scene_nodes()
    par = api.loop_verify_params()
    graphs, rows, n_out, which = P.build(a.graphs, a.nodes, scene, 900 + a.nodes)
    d_rows = torch.from_numpy(rows.view(np.uint8).reshape(rows.shape[0], P.NC, 64)).cuda()
    d_n_out = torch.from_numpy(n_out).cuda()
    g_dev = dict(graphs, xyzi=torch.from_numpy(graphs["xyzi"]).cuda())
    out = api.verify_sc_rows(g_dev, d_rows, d_n_out, None, par, device_out=True)
    verified = out["results"].clone()
    torch.cuda.synchronize()

    def call():
        out["results"].copy_(verified)                                         # every repetition starts from the verified records
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.verify_sample_covariances(g_dev, out, par)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    call()                                                                     # warm-up: workspaces, code load
    runs = [call() for _ in range(a.reps)]
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    call()
    prof = {k: round(v[0], 4) for k, v in ctx.profile_read(reset=True).items()}
    ctx.profile_enable(False)
    got = out["results"].cpu().numpy().view(L.VERIFY_RESULT_DTYPE).copy()
    lst = out["list"].cpu().numpy().view(L.LOOP_VERIFY_CANDIDATE_DTYPE).copy()
    # ---- the host route over the same candidates ------------------------------------------------------------------------------
    node_off, poses = graphs["node_off"], graphs["poses"]
    jobs = []
    for c, r in zip(lst, got):
        kf, kt = node_off[c["graph"]] + c["from"], node_off[c["graph"]] + c["to"]
        jobs.append(dict(from_scan=scene[which[kf]]["scan"], to_scan=scene[which[kt]]["scan"], from_peaks=scene[which[kf]]["peaks"],
                         to_peaks=scene[which[kt]]["peaks"], from_pose=poses[kf], t_be_guess=c["guess_xyt"], sc_sim=float(c["sc_sim"]),
                         odom_bounds=float(r["odom_bounds"]), group=int(c["query"])))
    batch = api.prepare_verify_batch(jobs)
    host = {}
    for sampling in (1, 0):
        vp = api.verify_params(use_covariance_sampling=sampling)
        api.verify_loop_candidates(batch, vp)                                  # warm-up
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = api.verify_loop_candidates(batch, vp)
            times.append((time.perf_counter() - t0) * 1e3)
        host[sampling] = (res, times)
    href = host[1][0]
    both = (got["cov_sampled"] == 1) & (href["cov_sampled"] == 1)
    rel = [float((np.abs(g["cov"][BLOCK] - h["cov"][BLOCK]) / np.abs(h["cov"][BLOCK])).max()) for g, h in zip(got[both], href[both])]
    added = min(host[1][1]) - min(host[0][1])
    res = dict(graphs=a.graphs, nodes=a.nodes, reps=a.reps, candidates=int(len(lst)), registered=int((got["reg_ok"] == 1).sum()),
               sampled=int(got["cov_sampled"].sum()), device_pass_ms_best=round(min(runs), 3), device_pass_ms_median=round(statistics.median(runs), 3),
               device_kernels_ms=prof, host_route_sampling_1_ms_best=round(min(host[1][1]), 3), host_route_sampling_0_ms_best=round(min(host[0][1]), 3),
               host_route_sampling_adds_ms=round(added, 3),
               agreement=dict(cov_sampled_equal=bool((got["cov_sampled"] == href["cov_sampled"]).all()), block_max_rel_dev=max(rel) if rel else 0.0))
    print("%d x %d nodes: %d candidates, %d registered, %d with a sampled covariance" % (a.graphs, a.nodes, res["candidates"], res["registered"],
                                                                                          res["sampled"]))
    print("  device pass: call best %.3f ms, median %.3f ms; kernels (ms) %s" % (res["device_pass_ms_best"], res["device_pass_ms_median"], prof))
    print("  host route:  use_covariance_sampling 1: %.3f ms, 0: %.3f ms -> sampling adds %.3f ms" % (
        res["host_route_sampling_1_ms_best"], res["host_route_sampling_0_ms_best"], added))
    print("  agreement:   %s" % res["agreement"], flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
