#!/usr/bin/env python
"""Batched pose-graph optimisation (cfear_pgo_solve_batch) against the host solver it batches (cfear_pgo_solve looped over
the same graphs), on synthetic laps (synth.pgo_lap_graph) with TBV's defaults (loop_scaling 500000, identity replacement):
  --case small   4096 graphs of ~1000 nodes with 16 loops each
  --case large   256 graphs of ~5000 nodes (Oxford's keyframe count) with 64 loops each
--distinct graphs are generated (sizes within 5 % of the nominal one) and repeated to fill the batch: marshalling millions of
constraint dicts in Python is not what is timed, and a graph's result does not depend on its neighbours.  Times are host
clocks around the C calls on arrays marshalled beforehand:
  batch      one cfear_pgo_solve_batch call (it synchronises), best and median of --reps after one warm-up
  host x1    cfear_pgo_solve graph after graph on one thread, once
  host x16   the same loop spread over 16 threads (the solver needs no context; ctypes drops the GIL), once
--host-graphs N times the host loops on the first N graphs only and scales to the batch (stated in the output).
The kernel's share of the call comes from the context's hipEvent profile of one extra call (launches = chunks); for the
trace run it again with --no-host under rocprofv3 --kernel-trace --stats.
    python tools/pgo_batch_probe.py [--case small] [--graphs N] [--reps 3] [--no-host] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api, synth  # noqa: E402

CASES = {"small": dict(graphs=4096, nodes=1000, loops=16), "large": dict(graphs=256, nodes=5000, loops=64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), default="small")
    ap.add_argument("--graphs", type=int, default=None)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-graphs", type=int, default=None, help="time the host loops on this many graphs and scale")
    ap.add_argument("--no-host", action="store_true", help="time the batch call only")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    case = dict(CASES[a.case])
    n_graphs = a.graphs or case["graphs"]
    rng = np.random.default_rng(0)
    distinct = [api._pgo_graph_arrays(*synth.pgo_lap_graph(int(case["nodes"] * rng.uniform(0.95, 1.05)), rng, n_loops=case["loops"],
                                                           direction=("back", "forward", "mixed")[k % 3])[:3], "graph %d" % k)
                for k in range(min(a.distinct, n_graphs))]
    arrs = [distinct[g % len(distinct)] for g in range(n_graphs)]
    node_off = np.concatenate([[0], np.cumsum([x[0].shape[0] for x in arrs])]).astype(np.int64)
    con_off = np.concatenate([[0], np.cumsum([x[2].shape[0] for x in arrs])]).astype(np.int64)
    poses0 = np.ascontiguousarray(np.concatenate([x[0] for x in arrs], 0))
    ids = np.ascontiguousarray(np.concatenate([x[1] for x in arrs]))
    cons = np.ascontiguousarray(np.concatenate([x[2] for x in arrs]))
    par = L.PgoParams()
    lib = L.lib()
    lib.cfear_pgo_params_default(C.byref(par))
    ctx = api.default_context()
    summ = np.zeros(n_graphs, L.PGO_SUMMARY_DTYPE)

    def batch():
        poses = poses0.copy()
        bad = C.c_int32(-1)
        t0 = time.perf_counter()
        ctx.check(lib.cfear_pgo_solve_batch(ctx.h, poses.ctypes.data, ids.ctypes.data, node_off.ctypes.data, int(node_off[-1]),
                                            cons.ctypes.data, con_off.ctypes.data, int(con_off[-1]), n_graphs, C.byref(par),
                                            summ.ctypes.data, C.byref(bad)))
        return (time.perf_counter() - t0) * 1e3, poses

    batch()                                                                # warm-up: workspace allocation, code load
    times = [batch()[0] for _ in range(a.reps)]
    ctx.profile_enable(True)
    ctx.profile_read(reset=True)
    _, dev_poses = batch()
    prof = ctx.profile_read(reset=True)
    ctx.profile_enable(False)
    kern = {k: (round(v[0], 3), int(v[1])) for k, v in prof.items() if k.startswith("pgo_")}
    res = dict(case=a.case, graphs=n_graphs, nodes=int(node_off[-1]), constraints=int(con_off[-1]), distinct=len(distinct),
               batch_ms_best=round(min(times), 2), batch_ms_median=round(statistics.median(times), 2),
               batch_ms_all=[round(t, 2) for t in times], kernel_ms_and_chunks=kern,
               iterations_mean=float(summ["iterations"].mean()), linear_iterations_mean=float(summ["linear_iterations"].mean()))
    print("batch: %d graphs, %d nodes, %d constraints: best %.2f ms, median %.2f ms over %d calls (all: %s)" %
          (n_graphs, res["nodes"], res["constraints"], res["batch_ms_best"], res["batch_ms_median"], a.reps, res["batch_ms_all"]), flush=True)
    print("device time of the kernel (ms, launches = chunks):", kern, flush=True)
    if not a.no_host:
        nh = min(a.host_graphs or n_graphs, n_graphs)
        host_poses = poses0.copy()
        hs = np.zeros(n_graphs, L.PGO_SUMMARY_DTYPE)

        def solve(g):
            n0, n1, c0, c1 = int(node_off[g]), int(node_off[g + 1]), int(con_off[g]), int(con_off[g + 1])
            rc = lib.cfear_pgo_solve(host_poses[n0:n1].ctypes.data, ids[n0:n1].ctypes.data, n1 - n0, cons[c0:c1].ctypes.data, c1 - c0,
                                     C.byref(par), C.cast(hs[g:g + 1].ctypes.data, C.POINTER(L.PgoSummary)))
            assert rc == L.OK, rc

        t0 = time.perf_counter()
        for g in range(nh):
            solve(g)
        one = (time.perf_counter() - t0) * 1e3
        host_poses[:] = poses0
        t0 = time.perf_counter()
        with ThreadPoolExecutor(a.threads) as pool:
            list(pool.map(solve, range(nh)))
        many = (time.perf_counter() - t0) * 1e3
        scale = n_graphs / nh
        n1 = int(node_off[nh])
        res.update(host_graphs_timed=nh, host_1_thread_ms=round(one * scale, 1), host_threads=a.threads,
                   host_threads_ms=round(many * scale, 1), speedup_over_threads=round(many * scale / res["batch_ms_median"], 2),
                   counts_equal=bool((hs["iterations"][:nh] == summ["iterations"][:nh]).all() and (hs["usable"][:nh] == summ["usable"][:nh]).all()),
                   max_dp=float(np.abs(host_poses[:n1, :3] - dev_poses[:n1, :3]).max()), max_dq=float(np.abs(host_poses[:n1, 3:] - dev_poses[:n1, 3:]).max()))
        print("host: %d graphs timed%s: 1 thread %.1f ms, %d threads %.1f ms; batch speed-up over the threads x%.2f; counts equal %s; "
              "max |dp| %.2e m, max |dq| %.2e" % (nh, "" if nh == n_graphs else " (scaled x%.1f to the batch)" % scale, res["host_1_thread_ms"],
                                                 a.threads, res["host_threads_ms"], res["speedup_over_threads"], res["counts_equal"],
                                                 res["max_dp"], res["max_dq"]), flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
