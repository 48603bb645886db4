#!/usr/bin/env python
"""Times the step between loop detection and the solve on synthetic graphs of two lengths: detector rows on the device in,
verified candidates out.
  device route   api.verify_sc_rows (cfear_verify_sc_rows): the rows never leave the device; the call's total time, and the
                 time of the route's own kernels (profile row "verify_graph_fill": the two prefix sums, the row expansion,
                 verify_fill_kernel with its odometry walks, the list's finish) next to the chain's existing kernels
  host route     what the parent commit offers for the same rows: rows to the host, per candidate the motions between `to`
                 and `from` and one cfear_verify_by_odometry call, one cfear_verify_job, then cfear_verify_loop_candidates
                 (its marshalling, api.prepare_verify_batch, is part of the route and timed apart)
Graphs: --graphs laps of a wobbling circle with --nodes nodes each (default 8 x 250 and 8 x 2000), five scans and peak
clouds of a synthetic scene reused for all nodes, three candidates for every node past the first 20 whose `to` nodes are
spread over the whole graph behind it, so a candidate's odometry chain grows with the graph.  The rows are made on the host
and uploaded before the clock starts.  Both routes see the same candidates; their odom_bounds and records are compared.
    python tools/loop_closure_probe.py [--graphs 8] [--nodes 250 2000] [--reps 3] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api, synth  # noqa: E402

K, Z_MIN, MIN_DISTANCE, GATE, NC = 40, 60.0, 2.5, 20, 3


def scene_nodes():
    """Five scans with their peaks, from sweeps of synth.scene_v1 through the library's own filter and surface points."""
    imgs, gt, sc = synth.scene_v1(3, 5)
    out = []
    for f in range(5):
        r = api.filter_kstrongest(imgs[f], K, Z_MIN, float(sc.range_res), MIN_DISTANCE, want_peaks=True)
        cloud = np.ascontiguousarray(r["xyzi"][0, :r["n_points"][0]])
        peaks = np.ascontiguousarray(r["xyzi_peaks"][0, :r["n_peaks"][0]])
        out.append(dict(scan=api.MapPointNormal(cloud, radius=3.0, weight_intensity=True), peaks=peaks, T=gt[f]))
    return out


def build(n_graphs, n_nodes, scene, seed):
    rng = np.random.default_rng(seed)
    N = n_graphs * n_nodes
    node_off = (np.arange(n_graphs + 1) * n_nodes).astype(np.int32)
    poses = np.concatenate([synth.sc_graph(n_nodes, seed=seed + g, points=1, step=2.5, radius=120.0)[1] for g in range(n_graphs)])
    which = rng.integers(0, 5, N)
    graphs = dict(node_off=node_off, table=api.ScanTable([scene[w]["scan"] for w in which]),
                  xyzi=np.concatenate([scene[w]["peaks"] for w in which]),
                  point_off=np.concatenate([[0], np.cumsum([len(scene[w]["peaks"]) for w in which])]).astype(np.int64), poses=poses,
                  rel=api.loop_relative_motions(poses, node_off))
    rows = np.zeros((N, NC), L.SC_CANDIDATE_DTYPE)
    n_out = np.zeros(N, np.int32)
    for g in range(n_graphs):
        for i in range(GATE, n_nodes):
            d = g * n_nodes + i
            n_out[d] = NC
            for s in range(NC):
                to = int(rng.integers(0, i - 10))
                true = api._compose_xyt(_inverse(scene[which[d]]["T"]), scene[which[node_off[g] + to]]["T"])
                r = rows[d, s]
                r["nn_idx"], r["min_dist"], r["min_dist_odom"] = to, rng.uniform(0.05, 0.5), rng.uniform(0.0, 0.6)
                r["yaw_diff_rad"] = np.float32(true[2] + rng.normal(0.0, 0.02))
                r["Taug"] = (0.0, float(rng.choice([0.0, 2.0, -2.0])), 0.0)
    return graphs, rows, n_out, which


def _inverse(a):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([-(c * a[0] + s * a[1]), s * a[0] - c * a[1], -a[2]])


def host_route(graphs, scene, which, d_rows, d_n_out, par):
    """The parent commit's route, timed in its parts (ms) -> (records, odom_bounds, times)."""
    node_off, poses, rel = graphs["node_off"], graphs["poses"], graphs["rel"]
    t0 = time.perf_counter()
    rows = d_rows.cpu().numpy().view(L.SC_CANDIDATE_DTYPE)[:, :, 0]
    n_out = d_n_out.cpu().numpy()
    t1 = time.perf_counter()
    jobs, bounds = [], []
    n_nodes = int(node_off[1])
    for d in np.flatnonzero(n_out):
        g, i = divmod(int(d), n_nodes)
        for s in range(n_out[d]):
            r = rows[d, s]
            to = int(r["nn_idx"])
            guess = api._compose_xyt(_inverse(np.asarray(r["Taug"], np.float64)), np.array([0.0, 0.0, float(r["yaw_diff_rad"])]))
            ob = api.VerifyByOdometry(rel[node_off[g] + to:node_off[g] + i], par.odom_sigma_error)
            kf, kt = node_off[g] + i, node_off[g] + to
            bounds.append(ob)
            jobs.append(dict(from_scan=scene[which[kf]]["scan"], to_scan=scene[which[kt]]["scan"], from_peaks=scene[which[kf]]["peaks"],
                             to_peaks=scene[which[kt]]["peaks"], from_pose=poses[kf], t_be_guess=guess, sc_sim=float(np.float32(r["min_dist"])),
                             odom_bounds=ob, group=int(kf)))
    t2 = time.perf_counter()
    batch = api.prepare_verify_batch(jobs)
    t3 = time.perf_counter()
    res = api.verify_loop_candidates(batch, par.verify)
    t4 = time.perf_counter()
    ms = lambda a, b: round((b - a) * 1e3, 3)
    return res, np.array(bounds), dict(rows_to_host_ms=ms(t0, t1), odometry_and_jobs_ms=ms(t1, t2), marshal_ms=ms(t2, t3),
                                       verify_loop_candidates_ms=ms(t3, t4), total_ms=ms(t0, t4))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=8)
    ap.add_argument("--nodes", type=int, nargs="+", default=[250, 2000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = api.default_context()
    scene = scene_nodes()
    par = api.loop_verify_params()
    res = dict(graphs=a.graphs, reps=a.reps, candidates_per_node=NC, shapes={})
    for n_nodes in a.nodes:
        graphs, rows, n_out, which = build(a.graphs, n_nodes, scene, 900 + n_nodes)
        d_rows = torch.from_numpy(rows.view(np.uint8).reshape(rows.shape[0], NC, 64)).cuda()
        d_n_out = torch.from_numpy(n_out).cuda()
        g_dev = dict(graphs, xyzi=torch.from_numpy(graphs["xyzi"]).cuda())
        torch.cuda.synchronize()

        def call():
            t0 = time.perf_counter()
            out = api.verify_sc_rows(g_dev, d_rows, d_n_out, None, par)
            return (time.perf_counter() - t0) * 1e3, out

        call()                                                                 # warm-up: workspaces, code load
        runs = [call() for _ in range(a.reps)]
        ctx.profile_enable(True)
        ctx.profile_read(reset=True)
        _, out = call()
        prof = {k: round(v[0], 4) for k, v in ctx.profile_read(reset=True).items()}
        ctx.profile_enable(False)
        host_route(graphs, scene, which, d_rows, d_n_out, par)                   # warm-up of the host route's launches
        hosts = [host_route(graphs, scene, which, d_rows, d_n_out, par) for _ in range(a.reps)]
        href, hb, _ = hosts[0]
        best = min(hosts, key=lambda h: h[2]["total_ms"])[2]
        got = out["results"]
        chain = [int(c["from"]) - int(c["to"]) for c in out["list"]]
        same = dict(odom_bounds_max_dev=float(np.abs(got["odom_bounds"] - hb).max()),
                    t_be_max_dev=float(np.abs(got["t_be"] - href["t_be"]).max()),
                    accepted_equal=bool((got["accepted"] == href["accepted"]).all()))
        r = dict(nodes=n_nodes, candidates=int(out["n"]), chain_steps_mean=round(float(np.mean(chain)), 1), chain_steps_max=int(max(chain)),
                 device_call_ms_best=round(min(t for t, _ in runs), 3), device_call_ms_median=round(statistics.median(t for t, _ in runs), 3),
                 device_kernels_ms=prof, host_route_best=best, host_route_total_ms_all=[h[2]["total_ms"] for h in hosts], agreement=same)
        res["shapes"]["%dx%d" % (a.graphs, n_nodes)] = r
        print("%d x %d nodes, %d candidates (chains of %.1f steps on average, %d at most)" % (a.graphs, n_nodes, r["candidates"],
                                                                                              r["chain_steps_mean"], r["chain_steps_max"]))
        print("  device route: call best %.3f ms, median %.3f ms; kernels (ms) %s" % (r["device_call_ms_best"], r["device_call_ms_median"], prof))
        print("  host route:   %s" % best)
        print("  agreement:    %s" % same, flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
