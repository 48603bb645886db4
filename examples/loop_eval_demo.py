#!/usr/bin/env python
"""How good is the loop detector?  One synthetic lap with ground truth, scored the way the reference scores its runs.

  radar sweeps -> odometry -> GTVicinity candidates -> registration and verification      as examples/vicinity_closure_demo.py
  candidates   -> api.loop_stats: the ground-truth-labelled row of every candidate         posegraph.cpp:332-371
  rows         -> api.write_loop_csv: loop.csv as EvaluationManager writes it, read back as the reference's scripts would
  loop.csv     -> api.LoopClosureEval: settings 4) to 6) of the paper's ablation, their classifiers trained and their ROC /
                  precision-recall curves computed on the device, without pandas or sklearn   3_loop_closure.py

Only (odometry_coupled, raw, augment) = (0, 0, 1) and (1, 0, 1) are written, so settings 4), 5) (decoupled) and 6), 7), 8)
(coupled) are the ones a name exists for; 4) to 6) are printed.  The lap is short, so the figures say that the chain runs,
not how good the detector is.
    python examples/loop_eval_demo.py [--frames 68] [--out loop.csv]"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vicinity_closure_demo as lap_demo          # noqa: E402


def run(n_frames=68, out=None, log=None):
    from tbv_slam_public_amd import api
    lap = lap_demo.run(n_frames)
    gt = lap["gt"]
    tables = []
    for coupled in (0, 1):
        m = lap["modes"]["gtvicinity"]
        jobs, res = m["jobs"], m["results"]
        cands = [dict(graph=0, **{"from": j["from"]}, to=j["to"], guess_nr=0, guess_xyt=r["t_be"]) for j, r in zip(jobs, res)]
        rows = api.loop_stats([gt], cands, max_distance=6.0)
        quality = {api.ODOM_BOUNDS: res["odom_bounds"] if coupled else np.ones(len(res)), api.SC_SIM: res["sc_sim"],
                   api.COMBINED_COST: res["alignment_quality"]}
        tables.append(api.loop_table([gt], cands, rows, quality, **{api.LoopClosureEval.COUPLED: coupled, api.LoopClosureEval.RAW: 0,
                                                                     api.LoopClosureEval.AUGMENT: 1}))
    table = {k: np.concatenate([t[k] for t in tables]) for k in tables[0]}
    path = out or os.path.join(tempfile.mkdtemp(), "loop.csv")
    api.write_loop_csv(path, table, quality_names=(api.ODOM_BOUNDS, api.SC_SIM, api.COMBINED_COST))
    ev = api.LoopClosureEval(api.read_loop_csv(path))
    if log:
        t = ev.table
        log("%s: %d rows, %d loops, %d candidates close, %d usable for training" % (
            path, len(t["is loop"]), int(t["is loop"].sum()), int(t["candidate close"].sum()), int(t["prediction pos ok"].sum())))
    try:
        results = ev.evaluate()
    except ValueError as e:                       # a lap on which every training row has the same label cannot be scored
        if log:
            log("not scored: %s" % e)
        return dict(path=path, table=table, results=[])
    for r in results:
        if log and r["name"][0] in "456":
            rec = r["record"]
            log("%-32s AUC %s  (%d thresholds, %d ROC points)" % (
                r["name"], "%.3f" % rec["auc"] if rec["status"] == 0 else "n/a: one class only", rec["n_thresholds"], rec["n_roc"]))
    return dict(path=path, table=table, results=results)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=68)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.frames, a.out, log=print)
