"""Timing probe of cfear_association_ties_batch beside cfear_get_cost_batch on IDENTICAL jobs in one process: --jobs two-scan
jobs drawn from bench.py's loop-closure world (1024 cached surface-point sets, candidate pairs 2..6 frames apart, P2L, Huber
0.1, uniform weights), marshalled once.  ms per call from a host clock around calls that end in the read-back of their records
(median of --reps after --warmup), and the library's own kernel event times.

  python tools/tie_audit_probe.py --jobs 4096 --reps 7
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the probe measures on an MI355X; there is nothing to time without one"
    import bench
    from tbv_slam_public_amd import api
    W = bench.LoopClosureWorld(types.SimpleNamespace(local_rank=0, rank=0, world=1, dist=None, dev=torch.device("cuda:0")))
    ctx, reg = W.ctx, W.reg
    reg.par.itr = 1                                           # GetCost's radius follows itr_: the audit's itr = 1
    cands = W.candidates(a.jobs)
    jobs = [([W.scans[int(c["target"])], W.scans[int(c["source"])]], np.stack([c["target_xyt"], c["source_xyt"]])) for c in cands]
    batch = reg.PrepareBatch(jobs)
    calls = {"association_ties": lambda: api.association_ties(batch, reg, 1, ctx=ctx),
             "association_ties_per_query": lambda: api.association_ties(batch, reg, 1, want_queries=True, ctx=ctx)[0],
             "get_cost_batch": lambda: reg.GetCostBatch(batch)}
    out = dict(jobs=len(jobs), mean_cells=float(np.mean([s.GetSize() for s in W.scans])), calls={})
    for name, call in calls.items():
        for _ in range(a.warmup):
            res = call()
        ctx.synchronize()
        ctx.profile_enable(True)
        call()
        ctx.synchronize()
        prof = ctx.profile_read()
        ctx.profile_enable(False)
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = call()
            ctx.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out["calls"][name] = dict(ms_per_call=float(np.median(ms)), ms_all=ms, kernel_event_ms={k: v[0] for k, v in prof.items()},
                                  not_ok=int((res["status"] != 0).sum()))
    rec = calls["association_ties"]()
    out["records"] = dict(queries=int(rec["n_queries"].sum()), in_radius=int(rec["n_in_radius"].sum()), tied=int(rec["n_tied"].sum()),
                          tied_effective=int(rec["n_tied_effective"].sum()), jobs_with_effective_tie=int((rec["n_tied_effective"] > 0).sum()),
                          max_group=int(rec["max_group"].max()))
    cost = calls["get_cost_batch"]()
    out["n_associated_equals_get_cost_blocks"] = bool((rec["n_associated"] == cost["num_residuals"]).all())      # P2L: one residual per block
    out["status_equals_get_cost"] = bool((rec["status"] == cost["status"]).all())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
