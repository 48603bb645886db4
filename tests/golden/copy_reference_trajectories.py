#!/usr/bin/env python
"""Builds tests/golden/ref_kitti_eval.npz (job_0) and ref_kitti_eval_job4.npz (job_4: one file per job keeps each below the
largest fixture already here) from the reference's recorded evaluation DATA
(/root/reference/evaluation/data/oxford_all_tbv_model_8/job_N/; no code is read): the inputs and the outputs of its own
`eval_odom.py --align 6dof` run (radar_kitti_benchmark/python/kitti_odometry.py, step_size 10).

  job                  the job number (job_0: the ground truth starts at the identity; job_4: it does not, so the
                       normalisation by the first pose is part of what the record pins)
  est, gt              [n][6] int32: columns (0, 1, 3, 4, 5, 7) of est/00.txt and gt/00.txt in units of 1e-6 -- the files
                       print 6 decimals, and int / 1e6 is the double float() parses (asserted below); the other six columns
                       are the constants 0 0 1 0 of a planar pose (asserted below)
  rows                 [m][5] float64: est/errors/00.txt -- first_frame, r_err / len, t_err / len, len, speed, as printed
                       (17 significant digits: float() of the text is the double the devkit held)
  result               the 12 lines of est/result.txt, as text: the 11 figures as write_result formats them

    python tests/golden/copy_reference_trajectories.py        (needs /root/reference)"""
import os

import numpy as np

SRC = "/root/reference/evaluation/data/oxford_all_tbv_model_8"
HERE = os.path.dirname(os.path.abspath(__file__))
JOBS = {0: "ref_kitti_eval.npz", 4: "ref_kitti_eval_job4.npz"}
KEEP = (0, 1, 3, 4, 5, 7)
CONST = {2: 0.0, 6: 0.0, 8: 0.0, 9: 0.0, 10: 1.0, 11: 0.0}


def _poses(path):
    a = np.array([[float(t) for t in ln.split()] for ln in open(path) if ln.strip()], np.float64)
    assert a.shape[1] == 12, path
    for c, v in CONST.items():
        assert (a[:, c] == v).all(), (path, c)
    q = np.rint(a[:, KEEP] * 1e6).astype(np.int64)
    assert (q / 1e6 == a[:, KEEP]).all() and np.abs(q).max() < 2 ** 31, path
    return q.astype(np.int32)


if __name__ == "__main__":
    for j, name in JOBS.items():
        d = os.path.join(SRC, "job_%d" % j)
        out = {"job": np.array(j, np.int32)}
        out["est"] = _poses(os.path.join(d, "est", "00.txt"))
        out["gt"] = _poses(os.path.join(d, "gt", "00.txt"))
        out["rows"] = np.array([[float(t) for t in ln.split()] for ln in open(os.path.join(d, "est", "errors", "00.txt"))], np.float64)
        out["result"] = np.array(open(os.path.join(d, "est", "result.txt")).read())
        dst = os.path.join(HERE, name)
        np.savez_compressed(dst, **out)
        print("wrote", dst, os.path.getsize(dst), {k: getattr(v, "shape", None) for k, v in out.items()})
