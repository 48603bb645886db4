"""CPU: the NumPy restatement of the tie audit (tests/tieaudit_cpu.py) against the oracle -- its lowest winner is
O.closest_idx, its associated set the blocks of O.associate -- on the constructed cases and on natural scans; the seeds the
GPU test audits do hold a tie at their guess pose; the record's size and the C++ mirror's syntax."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as O
from tbv_slam_public_amd import synth
from tests import tieaudit_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# scene_v1 seeds, from 1000 upward, whose pair holds at least one tied in-radius query at the fixture's guess pose
# (test_natural_seeds_hold_a_tie asserts it here; tests/test_gpu_tieaudit.py audits the same seeds on the device)
NATURAL_SEEDS = (1000, 1001, 1002, 1003, 1004)
RADIUS = 2.0                    # registration.h:122


def natural_inputs(seed):
    """Images and poses of one pair, built as tests/test_oracle_order_robustness.py::pairs builds them."""
    imgs, gt, _ = synth.scene_v1(seed, 2)
    c, s = np.cos(gt[0][2]), np.sin(gt[0][2])
    d = gt[1][:2] - gt[0][:2]
    guess = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], gt[1][2] - gt[0][2]]) + [0.3, -0.2, 0.01]
    return imgs, np.array([[0.0, 0.0, 0.0], guess])


def natural_pair(seed):
    imgs, poses = natural_inputs(seed)
    cells = []
    for f in range(2):
        sr, si, sc = O.kstrongest(imgs[f], 40, 60)
        cells.append(O.surface_points(O.kstrongest_cloud(sr, si, sc, 0.0438, 2.5), 3.0, 1.0, (0, 0), True))
    return cells, poses


@pytest.fixture(scope="module")
def natural():
    return {seed: natural_pair(seed) for seed in NATURAL_SEEDS}


def _check_against_oracle(scans, poses, itr):
    par = O.reg_params(radius=RADIUS)
    rec, pq, assoc = R.audit(scans, poses, RADIUS, itr)
    pairs, _ = O.associate(scans, poses, par, itr)
    assert assoc == {tuple(int(v) for v in p) for p in pairs}
    assert rec["n_associated"] == len(pairs) and rec["n_queries"] == (len(scans) - 1) * len(scans[-1]) == pq.shape[0]
    # the lowest winner is the oracle's GetClosestIdx, for the queries the association makes (the transformed source means)
    r = 2 * RADIUS if itr == 1 else RADIUS
    src = scans[-1]
    for t in range(len(scans) - 1):
        T = R.src_to_tar(poses[t], poses[-1])
        q = np.column_stack([T[0] * src["mean"][:, 0] + T[1] * src["mean"][:, 1] + T[4],
                             T[2] * src["mean"][:, 0] + T[3] * src["mean"][:, 1] + T[5]])
        assert (pq[t * len(src):(t + 1) * len(src), 0] == O.closest_idx(scans[t], q, r)).all()
    return rec, pq


def test_closest_case_matches_the_oracle():
    cells, queries = R.closest_case()
    lo, hi, cnt = R.closest_ties(cells, queries, R.CLOSEST_D)
    assert (lo == O.closest_idx(cells, queries, R.CLOSEST_D)).all()
    assert (lo[0], hi[0], cnt[0]) == (5, 8, 4) and (lo[1], hi[1], cnt[1]) == (0, 2, 3) and (lo[2], hi[2], cnt[2]) == (3, 4, 2)
    assert (lo[3], hi[3], cnt[3]) == (-1, -1, 0) and (lo[4], hi[4], cnt[4]) == (9, 9, 1)      # exactly d: out; an ulp inside: in
    assert cnt[5] == 0 and cnt[6] == 0 and (lo[7], cnt[7]) == (3, 2) and cnt[10] == 0


def test_constructed_jobs_match_the_oracle_and_hold_every_case():
    jobs = R.constructed_jobs()
    assert [(len(s), len(s[-1])) for s, _ in jobs] == [(2, 1), (3, 63), (4, 64), (2, 65), (3, 257), (4, 300), (2, 65)]
    assert all((np.abs(p[:, :2]) > 1e-3).all() and (np.abs(p[:, 2]) > 1e-3).all() for _, p in jobs)      # no identity pose
    for scans, poses in jobs:
        r1, q1 = _check_against_oracle(scans, poses, 1)
        r2, q2 = _check_against_oracle(scans, poses, 2)
        n = len(scans[-1])
        assert r1["n_tied"] >= 1 and q1[0, 2] >= 2                       # source 0: the bitwise copy
        if len(scans[0]) == R.TILE + 1:                                  # the group that spans the two LDS tiles
            assert tuple(q1[0]) == (5, R.TILE, 2) and r1["n_tied_effective"] >= 1
            continue
        if n < 5:
            assert r1["n_tied_effective"] == 0 and r1["status"] == R.ERR_TOO_FEW_RESIDUALS
            continue
        last = len(scans) - 1
        assert r1["n_tied"] > r1["n_tied_effective"] >= 3 * last         # sources 1, 2, 3 of every fixed scan
        for t in range(last):
            assert q1[t * n + 3, 0] == 0 and q1[t * n + 3, 2] == 2       # the group whose lowest cell fails the direction test
            assert (t, 0, 3) not in R.audit(scans, poses, RADIUS, 1)[2]
            assert q1[t * n + 4, 2] == 1 and q2[t * n + 4, 2] == 0       # 3 m: inside 2 * radius, outside radius
        assert r1["n_in_radius"] > r2["n_in_radius"] and r1["status"] == R.OK


def test_natural_seeds_hold_a_tie(natural):
    for seed, (cells, poses) in natural.items():
        r1, _ = _check_against_oracle(cells, poses, 1)
        _check_against_oracle(cells, poses, 2)
        assert r1["n_tied"] >= 1, seed


def test_tie_record_is_32_bytes():
    from tbv_slam_public_amd import _lib as L
    assert C.sizeof(L.TieRecord) == 32 == L.TIE_RECORD_DTYPE.itemsize
    assert tuple(L.TIE_RECORD_DTYPE.names) == R.RECORD_FIELDS and L.TIE_TILE == R.TILE
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    assert "#define CFEAR_TIE_TILE %d " % R.TILE in hdr and "} cfear_tie_record;" in hdr
    assert hasattr(L.lib(), "cfear_association_ties_batch") and hasattr(L.lib(), "cfear_scan_closest_ties")


def test_cpp_mirror_compiles_against_the_stand_ins(tmp_path):
    """include/cfear_hip.hpp (MapPointNormal::GetClosestTies, AssociationTies) is syntactically sound with the reference-side
    stand-ins; without a GPU the program reports the missing device and exits 2."""
    exe = str(tmp_path / "tieaudit_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "tieaudit_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2 and r.stdout.decode().split() == ["32"]
