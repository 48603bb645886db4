"""Which Cen2019 landmarks of a lap's sweeps hang on the order among equal h in cen2019features' unstable std::sort.

The reference sorts every pixel with h > mean_h by descending h with std::sort, which leaves the order among equal h open; this
library takes ascending row * cols + bin (DESIGN.md sections 3 and 4.20).  The demo drives one synthetic lap and audits all
its sweeps in one device call per max_points (api.cen2019_order_audit): per sweep, a bracket R_in <= R(order) <= R_out of the
marks under EVERY order of equal h, the targets every order emits, and a witness -- the same sweep filtered with the ties
reversed.

    python examples/cen2019_order_demo.py [--seed 0] [--frames 48]

Prints, at max_points 1000 and 10000, the share of clear sweeps (no order changes a mark), the band sizes, the share of
certified targets and what the reversed order changes.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frames", type=int, default=48)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "the demo runs on an MI355X; the library has no CPU path"
    from tbv_slam_public_amd import api, synth
    imgs = torch.from_numpy(np.ascontiguousarray(synth.scene_v1(a.seed, a.frames, circle_frames=a.frames)[0])).cuda()
    for mp in (1000, 10000):
        rec = api.cen2019_order_audit(imgs, max_points=mp)["records"]
        n = len(rec)
        clear = rec["n_marks_in"] == rec["n_marks_out"]
        print("max_points %d: %d sweeps, %d .. %d candidates, %d .. %d targets each"
              % (mp, n, rec["n_candidates"].min(), rec["n_candidates"].max(), rec["n_targets"].min(), rec["n_targets"].max()))
        print("  clear (no order of equal h changes a mark): %d sweeps (%.0f %%)" % (clear.sum(), 100.0 * clear.mean()))
        print("  fresh candidates: %d sure, %d possible, %d under this library's order (sums over the lap)"
              % (rec["n_sure_fresh"].sum(), rec["n_possibly_fresh"].sum(), rec["n_fresh"].sum()))
        print("  band (candidates whose processing the order decides): 0 in %d sweeps, median %d, worst %d; rows with a tied "
              "straddling run: %d" % ((rec["n_band"] == 0).sum(), np.median(rec["n_band"]), rec["n_band"].max(), rec["n_rows_straddle_tied"].sum()))
        print("  marks the order can move (R_out - R_in): median %d, worst %d of %d"
              % (np.median(rec["n_marks_out"] - rec["n_marks_in"]), (rec["n_marks_out"] - rec["n_marks_in"]).max(),
                 rec["n_marks_out"][(rec["n_marks_out"] - rec["n_marks_in"]).argmax()]))
        print("  certified targets: %d of %d (%.1f %%); sweeps with every target certified: %d"
              % (rec["n_targets_certain"].sum(), rec["n_targets"].sum(), 100.0 * rec["n_targets_certain"].sum() / max(1, rec["n_targets"].sum()),
                 (rec["n_targets_certain"] == rec["n_targets"]).sum()))
        print("  witness (ties reversed): changes a mark in %d sweeps (%d marks), a target in %d sweeps (%d targets); in a clear sweep: %d"
              % ((rec["n_marks_changed_reversed"] > 0).sum(), rec["n_marks_changed_reversed"].sum(), (rec["n_targets_changed_reversed"] > 0).sum(),
                 rec["n_targets_changed_reversed"].sum(), (clear & (rec["n_marks_changed_reversed"] > 0)).sum()))


if __name__ == "__main__":
    main()
