#!/usr/bin/env python
"""Times cfear_logreg_fit_batch: ms per call, host rows (upload included) and device-resident rows, for
  single   one 58 071 x 6 model (the shape of the reference's combined.txt), synthetic rows
  three    the CorAl, CFEAR and combined models over one such table, one call
  batch    256 models of 4 390 x 3 (the shape of the loop classifier's rows)
next to sklearn (where it imports) and the NumPy restatement on the same rows, on this host's CPU.
    python tools/logreg_probe.py [--repeats 20] [--warmup 3] [--no-cpu]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rows_like_combined(seed, n=58071):
    """Six features with the spread of the reference's rows: three CorAl entropies / overlap of order 1, a cost of order 10,
    #residuals of order 200, and a count of order 300; 8 % aligned."""
    rng = np.random.RandomState(seed)
    y = (rng.rand(n) < 0.077).astype(np.float64)
    X = np.column_stack([rng.normal(-0.1 - 0.4 * y, 0.15), rng.normal(0.3 + 0.2 * y, 0.2), rng.uniform(0.2, 1.0, n),
                         rng.normal(12.0 - 5.0 * y, 4.0), rng.normal(180.0 + 40.0 * y, 50.0), rng.normal(300.0, 40.0, n)])
    return np.ascontiguousarray(np.column_stack([y, X]))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    from tbv_slam_public_amd import api
    from tests import logreg_cpu as R
    table = rows_like_combined(1)
    y = np.ascontiguousarray(table[:, 0])
    loop = [R.synthetic(100 + m, 4390, 3) for m in range(256)]
    cases = {
        "single": [dict(X=table, y=y, columns=[1, 2, 3, 4, 5, 6])],
        "three": [dict(X=table, y=y, columns=c) for c in ([1, 2, 3, 4, 5, 6], [1, 2, 3], [4, 5, 6])],
        "batch": [dict(X=X, y=yy) for X, yy in loop],
    }
    out = {}
    for name, jobs in cases.items():
        dev = {}

        def on_device(j):
            for k in ("X", "y"):
                if id(j[k]) not in dev:
                    dev[id(j[k])] = torch.from_numpy(j[k]).cuda()
            return dict(j, X=dev[id(j["X"])], y=dev[id(j["y"])])
        djobs = [on_device(j) for j in jobs]
        torch.cuda.synchronize()
        rec = api.logreg_fit_batch(jobs)
        assert (rec["status"] == 0).all(), rec["status"]
        assert api.logreg_fit_batch(djobs).tobytes() == rec.tobytes()
        out[name] = dict(models=len(jobs), iterations=[int(rec["iterations"].min()), int(rec["iterations"].max())],
                         host_rows=timed(lambda: api.logreg_fit_batch(jobs), a.warmup, a.repeats),
                         device_rows=timed(lambda: api.logreg_fit_batch(djobs), a.warmup, a.repeats))
    if not a.no_cpu:
        X6 = np.ascontiguousarray(table[:, 1:])
        cpu = {"restatement_single": timed(lambda: R.fit(X6, y), 1, 3),
               "restatement_batch": timed(lambda: [R.fit(X, yy) for X, yy in loop], 0, 1)}
        try:
            from sklearn.linear_model import LogisticRegression as SkLR
            cpu["sklearn_single"] = timed(lambda: SkLR(class_weight="balanced", max_iter=1000).fit(X6, y), 1, 3)
            cpu["sklearn_batch"] = timed(lambda: [SkLR(class_weight="balanced", max_iter=1000).fit(X, yy) for X, yy in loop], 0, 1)
        except ImportError:
            pass
        out["cpu"] = cpu
    print(json.dumps(out))


if __name__ == "__main__":
    main()
