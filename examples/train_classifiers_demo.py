#!/usr/bin/env python
"""Training the alignment classifier on the GPU, then closing loops with it: what the reference does with
alignment_checker's ScanLearningInterface and an embedded sklearn, without either.

  radar sweeps  -> CFEAR-3 odometry, graph nodes (peaks cloud + surface points)   as examples/loop_closure_demo.py
  node pairs    -> the 13 perturbations of AddTrainingData, CorAl and CFEAR quality of every pair in two launches
                   (ScanLearningInterface.AddTrainingDataBatch)
  rows          -> the combined classifier, fitted by Newton's method in one launch (FitModelsDevice, cfear_logreg_fit_batch)
  coefficients  -> cfear_verify_params (verify_params()), and the loop-candidate verification of loop_closure_demo with the
                   model just trained in place of the preset one

    python examples/train_classifiers_demo.py [--frames 68]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_closure_demo as demo               # noqa: E402


class TrainedBackend(demo.HipBackend):
    """HipBackend whose verifier carries coefficients fitted on the sequence's own keyframe pairs."""

    def __init__(self, log=None):
        super().__init__()
        self.log = log or (lambda *_: None)
        self.par = None

    def sequence(self, imgs):
        poses, nodes = super().sequence(imgs)
        sli = self.api.ScanLearningInterface()
        sli.AddTrainingDataBatch([dict(T=p, cldPeaks=nd["peaks"], CFEAR=nd["scan"]) for p, nd in zip(poses, nodes)])
        clf = sli.combined_class
        rec = sli.FitModelsDevice()[0]
        self.log("trained on %d rows (%d aligned): %d Newton steps, F = %.6g, |gradient| = %.2e, balanced accuracy %.4f, "
                 "confusion tn fp fn tp = %s" % (rec["n_used"], rec["n_pos"], rec["iterations"], rec["objective"], rec["grad_inf"],
                                                 rec["balanced_accuracy"], rec["confusion"].tolist()))
        self.log("intercept %.6g, coefficients %s" % (clf.intercept_, np.array2string(clf.coef_, precision=6)))
        self.sli, self.par = sli, sli.verify_params()
        return poses, nodes

    def verify(self, nodes, cands):
        jobs = [dict(from_scan=nodes[c["from"]]["scan"], to_scan=nodes[c["to"]]["scan"], from_peaks=nodes[c["from"]]["peaks"],
                     to_peaks=nodes[c["to"]]["peaks"], from_pose=c["from_pose"], t_be_guess=c["t_be_guess"], sc_sim=c["sc_sim"],
                     odom_bounds=c["odom_bounds"], group=c["from"]) for c in cands]
        r = self.api.verify_loop_candidates(jobs, self.par)
        return [dict(t_be=r["t_be"][i].copy(), probability=float(r["probability"][i]), accepted=bool(r["accepted"][i]),
                     reg_ok=bool(r["reg_ok"][i]), alignment_quality=float(r["alignment_quality"][i])) for i in range(len(cands))]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=68)
    a = ap.parse_args()
    out = demo.run(TrainedBackend(print), a.frames, log=print)
    acc = sum(r["accepted"] for r in out["results"])
    print("%d candidates verified with the trained model, %d loop constraints accepted" % (len(out["candidates"]), acc))
