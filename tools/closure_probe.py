#!/usr/bin/env python
"""Times cfear_closure_candidates_batch (GTVicinityClosure / MiniClosure candidates, csrc/closure.hip) on synthetic laps
(tests/closure_cpu.py's generator: a 100 m circle, 1 m steps) with the reference's default thresholds, in both modes:
  long    1 graph of 8192 nodes
  batch   256 graphs of 512 nodes (16 distinct laps repeated: a graph's result does not depend on its neighbours)
Times are host clocks around the C call on arrays marshalled beforehand; the call stages its inputs, runs both kernels and
returns when the records are in host memory.  Per shape and mode: one warm-up call, then --reps calls; best, median and the
whole list are printed, and the device time of the two kernels from the context's hipEvent profile of one extra call.
Next to them: the plain-Python model (tests/closure_cpu.py) on ONE 512-node graph, timed once -- there is no other
implementation to compare with.  The device records of that graph are checked against the model while at it.
    python tools/closure_probe.py [--reps 7] [--json out.json]"""
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

import closure_cpu as M  # noqa: E402
from tbv_slam_public_amd import _lib as L  # noqa: E402
from tbv_slam_public_amd import api  # noqa: E402

SHAPES = {"long": (1, 8192), "batch": (256, 512)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ctx = api.default_context()
    lib = ctx._lib
    res = dict(origins_per_workgroup=L.CLOSURE_ORIGINS, tile=L.CLOSURE_TILE, reps=a.reps, shapes={})
    for shape, (n_graphs, n) in SHAPES.items():
        laps = [M.lap(n, 1000 + k) for k in range(min(a.distinct, n_graphs))]
        graphs = [laps[g % len(laps)] for g in range(n_graphs)]
        pos, steps, rel = (np.ascontiguousarray(np.concatenate([g[k] for g in graphs])) for k in range(3))
        off = (np.arange(n_graphs + 1) * n).astype(np.int64)
        out = np.zeros(n_graphs * n, L.CLOSURE_CANDIDATE_DTYPE)
        for mode in ("gtvicinity", "mini"):
            par = api.closure_params(mode)

            def call():
                bad = C.c_int32(-1)
                t0 = time.perf_counter()
                ctx.check(lib.cfear_closure_candidates_batch(ctx.h, pos.ctypes.data, steps.ctypes.data, rel.ctypes.data, off.ctypes.data,
                                                             n_graphs * n, n_graphs, C.byref(par), out.ctypes.data, C.byref(bad)))
                return (time.perf_counter() - t0) * 1e3

            call()                                                             # warm-up: workspace allocation, code load
            times = [call() for _ in range(a.reps)]
            ctx.profile_enable(True)
            ctx.profile_read(reset=True)
            call()
            prof = ctx.profile_read(reset=True)
            ctx.profile_enable(False)
            kern = {k: round(v[0], 4) for k, v in prof.items() if k.startswith("closure_")}
            r = dict(graphs=n_graphs, nodes=n, call_ms_best=round(min(times), 3), call_ms_median=round(statistics.median(times), 3),
                     call_ms_all=[round(t, 3) for t in times], kernel_ms=kern, candidates=int((out["to"] >= 0).sum()),
                     exhausted=int(out["exhausted"].sum()))
            res["shapes"]["%s/%s" % (shape, mode)] = r
            print("%-5s %-10s %3d x %4d nodes: call best %.3f ms, median %.3f ms over %d (all: %s); kernels (ms) %s; %d candidates, %d exhausted"
                  % (shape, mode, n_graphs, n, r["call_ms_best"], r["call_ms_median"], a.reps, r["call_ms_all"], kern, r["candidates"],
                     r["exhausted"]), flush=True)
            if shape == "batch":
                t0 = time.perf_counter()
                rec = M.candidates(laps[0][0], laps[0][1], mode, **M.DEFAULTS[mode])
                model_ms = (time.perf_counter() - t0) * 1e3
                dev = out[:n]
                same = all(dev[f].tobytes() == rec[f].tobytes() for f in ("to", "exhausted", "eucl", "trav", "rel"))
                r.update(python_model_ms_one_graph=round(model_ms, 1), equals_model=bool(same))
                print("      %-10s the Python model on ONE %d-node graph: %.1f ms; device records equal the model's: %s" % (mode, n, model_ms, same),
                      flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
