"""CPU: what the end of a pose-graph run (cfear_graph_align_batch, cfear_graph_map_batch, cfear_graph_string_write,
cfear_graph_output_write; csrc/graphfinish.hip) needs no device for -- the NumPy restatement the GPU results are compared with
(tests/graphfinish_cpu.py) pinned by properties, the two host writers through the C-ABI against lines written out by hand, the
ABI, and the refusals that are made before a context is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import graphfinish_cpu as G
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_graph_align_batch", "cfear_graph_map_batch", "cfear_graph_string_write", "cfear_graph_output_write"]


# ---- the restatement against itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [True, False])
def test_a_rigidly_moved_trajectory_is_aligned_back(planar):
    """est = X * gt exactly (no noise): Align must find Tgtalign = X^-1 and put every node back on its ground truth, within
    the bound of check_alignment (tests/test_gpu_kitti_eval.py) as alignment_bound restates it: one NumPy-summed H against
    the exact one."""
    _, gt = G.lap(90, 5, planar)
    X = G.to_rows(G.euler_pose(6.0, -4.0, 0.0 if planar else 1.5, 0.0 if planar else 0.03, 0.0 if planar else -0.04, 0.4))
    est = np.array([G.from_rows(G.mul_rows(X, G.to_rows(g))) for g in gt])
    new, row, ate = G.align(est, gt, np.ones(len(gt), bool))
    want = G.affine_inverse(X).reshape(3, 4)
    b_r, b_t = G.alignment_bound(gt[:, :3], est[:, :3], 2 * G.NUMPY_DEPTH)
    got = row.reshape(3, 4)
    # est.p carries the rounding of X * gt (a few 2^-53 of 50 m per node): it moves H like a summation error of depth 1 more
    assert np.abs(got[:, :3] - want[:, :3]).max() <= b_r and np.abs(got[:, 3] - want[:, 3]).max() <= b_t
    assert abs(np.linalg.det(got[:, :3]) - 1.0) <= max(b_r, 16 * 2.0 ** -53)
    # a node is moved by at most |dR| |p| + |dt|
    assert np.abs(new[:, :3] - gt[:, :3]).max() <= b_r * np.abs(est[:, :3]).max() * 3 + b_t + 1e-13
    assert ate <= b_r * np.abs(est[:, :3]).max() * 3 + b_t + 1e-13
    assert np.abs(np.abs((new[:, 3:] * gt[:, 3:]).sum(1)) - 1.0).max() <= 1e-12          # the same rotations (q and -q are one)


def test_a_planar_reflected_configuration_yields_a_rotation():
    """Planar data whose unconstrained best fit is a reflection: det(V U^T) < 0 and the third row of V^T is negated."""
    rng = np.random.default_rng(3)
    A = np.concatenate([rng.normal(0, 10, (40, 2)), np.zeros((40, 1))], 1)
    B = A * [1.0, -1.0, 1.0] + [3.0, 2.0, 0.0]                       # mirrored in y
    cA, cB, H = G.fit_terms(A, B)
    U, _, Vt = np.linalg.svd(H)
    row = G.best_fit_transform(A, B).reshape(3, 4)
    assert abs(np.linalg.det(row[:, :3]) - 1.0) <= 1e-12
    assert np.abs(row[:, :3] @ row[:, :3].T - np.eye(3)).max() <= 1e-12
    # and a proper planar rotation comes back as itself whichever sign LAPACK gave the null vector
    c, s = np.cos(0.7), np.sin(0.7)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    row = G.best_fit_transform(A, A @ Rz.T + [1.0, 2.0, 0.0]).reshape(3, 4)
    assert np.abs(row[:, :3] - Rz).max() <= 1e-12 and np.abs(row[:, 3] - [1.0, 2.0, 0.0]).max() <= 1e-11


def test_zero_and_one_ground_truth_node_give_the_identity_rotation():
    est, gt = G.lap(6, 1)
    row = G.best_fit_transform(np.zeros((0, 3)), np.zeros((0, 3))).reshape(3, 4)
    assert (row == np.eye(3, 4)).all()                               # centroids 0 / max(0, 1)
    row = G.best_fit_transform(gt[2:3, :3], est[2:3, :3]).reshape(3, 4)
    assert (row[:, :3] == np.eye(3)).all() and (row[:, 3] == est[2, :3] - gt[2, :3]).all()
    new, arow, ate = G.align(est, gt, [0, 0, 1, 0, 0, 0])
    assert (arow.reshape(3, 4)[:, :3] == np.eye(3)).all()
    assert np.abs(new[2, :3] - gt[2, :3]).max() <= 1e-14 and ate <= 1e-14        # the one node lands on its ground truth
    new, arow, ate = G.align(est, gt, np.zeros(6, bool))
    assert (arow == G.IDENTITY).all() and ate == 0.0
    # the rewrite happens under the identity too: q is re-derived from the matrix and normalised
    assert np.abs(new - est).max() <= 4e-16 and new.shape == est.shape


def test_the_quaternion_conversion_round_trips_through_all_four_branches():
    cases = {3: G.euler_pose(0, 0, 0, 0.1, -0.2, 0.3),                # trace > 0
             0: G.euler_pose(0, 0, 0, np.pi - 0.05, 0.02, 0.01),      # a half turn about x
             1: G.euler_pose(0, 0, 0, 0.02, np.pi - 0.04, 0.01),      # ... about y
             2: G.euler_pose(0, 0, 0, 0.01, 0.03, np.pi - 0.02)}      # ... about z
    for branch, pose in cases.items():
        m = G.to_rows(pose)
        assert G.quat_branch(m) == branch
        back = G.from_rows(m)
        sign = 1.0 if np.dot(back[3:], pose[3:]) > 0 else -1.0
        assert np.abs(sign * back[3:] - pose[3:]).max() <= 4e-16, branch
        assert abs(np.linalg.norm(back[3:]) - 1.0) <= 2.3e-16
        assert np.abs(G.to_rows(back) - m).max() <= 1e-15
    # Eigen's index choice on ties: m11 > m00 is strict, so equal leading entries keep i = 0; m22 > m(i,i) likewise
    tie = np.array([-1.0 / 3, 0, 0, 0, 0, -1.0 / 3, 0, 0, 0, 0, -1.0 / 3, 0])
    assert G.quat_branch(tie) == 0


def test_the_inverse_inverts_a_block_that_is_not_orthonormal():
    m = np.array([0.9, -0.5, 0.1, 3.0, 0.45, 0.8, -0.05, -2.0, 0.02, 0.07, 1.1, 0.5])
    inv = G.affine_inverse(m)
    assert np.abs(G.mul_rows(inv, m) - G.IDENTITY).max() <= 1e-15
    assert np.abs(inv.reshape(3, 4)[:, :3] - m.reshape(3, 4)[:, :3].T).max() > 0.05      # not the transpose


def test_the_map_restatement_rounds_as_pcl_does():
    pose = G.euler_pose(100.0, -50.0, 2.0, 0.1, -0.2, 1.0)
    cloud = np.array([[1.5, 2.25, -0.5, 77.0], [1e-3, 33.3, 4.0, 1.0]], np.float32)
    out = G.transform_cloud(G.to_rows(pose), cloud)
    assert out.dtype == np.float32 and (out[:, 3] == cloud[:, 3]).all()
    m = G.to_rows(pose)
    x, y, z = (float(v) for v in cloud[1, :3])
    assert out[1, 2] == np.float32(((m[8] * x + m[9] * y) + m[10] * z) + m[11])
    mm, mg = G.graph_map([pose] * 5, [pose] * 5, [0, 1, 1, 1, 0], [cloud] * 5, skip_frames=2)
    assert mm.shape == (6, 4) and mg.shape == (2, 4)                 # ordinals 0, 2 and 4; of those only node 2 has ground truth


# ---- the two writers through the C-ABI ---------------------------------------------------------------------------------------
IDQ = [0.0, 0.0, 0.0, 1.0]
HALF = [0.0, 0.0, 1.0, 0.0]          # a half turn about z: the matrix is diag(-1, -1, 1) with exact zeros off the diagonal


def test_graph_string_lines_are_the_reference_s(tmp_path):
    # 2.0000005 is the double 2.000000500000000069...: the sixth decimal rounds up; 0.1234565 is 0.12345649999...: down.
    # -0.0 as a translation prints with its sign under std::fixed.  The stamp is std::to_string of an unsigned long.
    poses = np.array([[2.0000005, -0.0, 0.1234565] + IDQ,
                      [-7.5, 1e9, 0.0] + HALF])
    stamps = [1547131046353776000, 18446744073709551615]
    path = str(tmp_path / "graph.txt")
    api.SaveGraphString(path, poses, stamps)
    want = ("1.000000 0.000000 0.000000 2.000001 0.000000 1.000000 0.000000 -0.000000 0.000000 0.000000 1.000000 0.123456 1547131046353776000\n"
            "\n"
            "-1.000000 0.000000 0.000000 -7.500000 0.000000 -1.000000 0.000000 1000000000.000000 0.000000 0.000000 1.000000 0.000000 18446744073709551615\n"
            "\n")
    assert open(path).read() == want
    assert len("1547131046353776000") == 19
    api.SaveGraphString(path, np.zeros((0, 7)), [])
    assert open(path).read() == ""


def test_output_graph_writes_the_nodes_with_ground_truth(tmp_path):
    poses = np.array([[1.0, 2.0, 0.0] + IDQ, [3.0, 4.0, 0.5] + HALF, [5.0, 6.0, 0.0] + IDQ])
    gt = np.array([[1.5, 2.5, 0.0] + IDQ, [9.0, 9.0, 9.0] + IDQ, [5.25, 6.25, -0.0] + HALF])
    est_path, gt_path = str(tmp_path / "est.txt"), str(tmp_path / "gt.txt")
    api.OutputGraph(est_path, gt_path, poses, gt, [1, 0, 1])           # a subset: node 1 is in neither file
    assert open(est_path).read() == ("1.000000 0.000000 0.000000 1.000000 0.000000 1.000000 0.000000 2.000000 0.000000 0.000000 1.000000 0.000000\n"
                                     "1.000000 0.000000 0.000000 5.000000 0.000000 1.000000 0.000000 6.000000 0.000000 0.000000 1.000000 0.000000\n")
    # the estimate file holds the poses, the ground-truth file Tgt: the reference's swapped local names do not swap the files
    assert open(gt_path).read() == ("1.000000 0.000000 0.000000 1.500000 0.000000 1.000000 0.000000 2.500000 0.000000 0.000000 1.000000 0.000000\n"
                                    "-1.000000 0.000000 0.000000 5.250000 0.000000 -1.000000 0.000000 6.250000 0.000000 0.000000 1.000000 -0.000000\n")
    api.OutputGraph(est_path, gt_path, poses, gt, [0, 0, 0])           # no ground truth at all: every pose, and an empty gt file
    assert len(open(est_path).read().splitlines()) == 3 and open(est_path).read().splitlines()[1].split(" ")[3] == "3.000000"
    assert os.path.exists(gt_path) and open(gt_path).read() == ""
    api.OutputGraph(est_path, gt_path, poses)                          # ... likewise when none was ever given
    assert len(open(est_path).read().splitlines()) == 3 and open(gt_path).read() == ""


def test_writers_refuse_and_report(tmp_path):
    lib = L.lib()
    p = np.array([[0.0, 0, 0] + IDQ])
    s = np.array([1], np.uint64)
    assert lib.cfear_graph_string_write(None, p.ctypes.data, s.ctypes.data, 1) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_graph_string_write(os.fsencode(str(tmp_path / "x")), None, s.ctypes.data, 1) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_graph_string_write(os.fsencode(str(tmp_path / "no" / "x")), p.ctypes.data, s.ctypes.data, 1) == L.ERR_IO
    h = np.array([1], np.uint8)
    assert lib.cfear_graph_output_write(os.fsencode(str(tmp_path / "e")), os.fsencode(str(tmp_path / "g")), p.ctypes.data, None,
                                        h.ctypes.data, 1) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_graph_output_write(os.fsencode(str(tmp_path / "e")), os.fsencode(str(tmp_path / "no" / "g")), p.ctypes.data, p.ctypes.data,
                                        h.ctypes.data, 1) == L.ERR_IO
    with pytest.raises(L.CfearError):
        api.SaveGraphString(str(tmp_path / "x"), p, [1, 2])


# ---- the ABI and the refusals that need no context ---------------------------------------------------------------------------
def test_the_abi_declares_and_exports_the_new_calls():
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert lib.cfear_abi_version() == 1
    assert "#define CFEAR_GRAPH_MAP_TILE %d" % L.GRAPH_MAP_TILE in hdr
    assert re.search(r"\}\s*cfear_graph_align_summary;\s*/\* %d bytes \*/" % L.GRAPH_ALIGN_SUMMARY_DTYPE.itemsize, hdr)
    assert re.search(r"\}\s*cfear_graph_map_summary;\s*/\* %d bytes \*/" % L.GRAPH_MAP_SUMMARY_DTYPE.itemsize, hdr)


def test_refusals_before_a_context_is_needed():
    lib = L.lib()
    poses = np.zeros((3, 7))
    poses[:, 6] = 1.0
    has = np.ones(3, np.uint8)
    xyzi = np.zeros((5, 4), np.float32)
    summ = np.zeros(1, L.GRAPH_MAP_SUMMARY_DTYPE)
    out = np.zeros((5, 4), np.float32)
    good_nodes, good_clouds = np.array([0, 3], np.int64), np.array([0, 2, 2, 5], np.int64)

    def call(skip=1, nodes=good_nodes, clouds=good_clouds, n_points=5):
        par = L.GraphMapParams(skip, 1)
        return lib.cfear_graph_map_batch(None, poses.ctypes.data, poses.ctypes.data, has.ctypes.data, nodes.ctypes.data, 3, 1, xyzi.ctypes.data,
                                         clouds.ctypes.data, n_points, C.byref(par), out.ctypes.data, 5, out.ctypes.data, 5, summ.ctypes.data)
    for kw, what in ((dict(skip=0), "skip_frames"), (dict(skip=-2), "skip_frames"), (dict(nodes=np.array([1, 3], np.int64)), "node_offsets"),
                     (dict(nodes=np.array([0, 2], np.int64)), "node_offsets"), (dict(clouds=np.array([0, 3, 2, 5], np.int64)), "cloud_offsets"),
                     (dict(clouds=np.array([0, 2, 2, 4], np.int64)), "cloud_offsets"), (dict(clouds=np.array([1, 2, 2, 5], np.int64)), "cloud_offsets"),
                     (dict(), "null context")):
        assert call(**kw) == L.ERR_INVALID_ARGUMENT, kw
        assert what in lib.cfear_last_error(None).decode(), (kw, lib.cfear_last_error(None))
    asum = np.zeros(1, L.GRAPH_ALIGN_SUMMARY_DTYPE)
    bad = np.array([0, 4], np.int64)
    assert lib.cfear_graph_align_batch(None, poses.ctypes.data, poses.ctypes.data, has.ctypes.data, bad.ctypes.data, 3, 1, asum.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert "node_offsets" in lib.cfear_last_error(None).decode()
    assert lib.cfear_graph_align_batch(None, poses.ctypes.data, None, has.ctypes.data, good_nodes.ctypes.data, 3, 1, asum.ctypes.data) == L.ERR_INVALID_ARGUMENT


def test_the_mirror_marshals_graphs_of_every_form():
    est, gt = G.lap(4, 2)
    a = api._finish_graph_arrays((est, gt, [1, 0, 1, 1]), "t")
    nodes = [dict(T=est[k], Tgt=gt[k], has_Tgt=bool(h), stamp=7 + k, cloud_peaks=dict(xyzi=np.zeros((k, 4), np.float32)))
             for k, h in enumerate([1, 0, 1, 1])]
    b = api._finish_graph_arrays(nodes, "t")
    g = api.PoseGraph(nodes=nodes)
    for x, y, z in zip(a, b, (g.poses, g.gt, g.has_gt)):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert g.stamps.tolist() == [7, 8, 9, 10] and [c.shape[0] for c in g.clouds] == [0, 1, 2, 3] and g.size() == 4
    planar = api._finish_graph_arrays((np.array([[1.0, 2.0, 0.5]]),), "t")
    assert planar[0].shape == (1, 7) and planar[2].tolist() == [0] and abs(planar[0][0, 5] - np.sin(0.25)) < 1e-15
    with pytest.raises(L.CfearError):
        api._finish_graph_arrays((est, gt[:2]), "t")


def test_signature_program_writes_the_files(tmp_path):
    import subprocess
    exe = str(tmp_path / "graphfinish_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "graphfinish_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    subprocess.run([exe, "write", str(tmp_path)], check=True, timeout=120)
    lines = open(tmp_path / "graph.txt").read().split("\n")
    assert len(lines) == 13 and lines[1] == "" and lines[0].endswith(" 10") and lines[10].endswith(" 60")
    # node 4 has no ground truth: five lines in both files; the second graph has none at all
    assert len(open(tmp_path / "est.txt").read().splitlines()) == len(open(tmp_path / "gt.txt").read().splitlines()) == 5
    assert open(tmp_path / "gt.txt").read().splitlines()[4].split(" ")[7] == "6.000000"
    assert len(open(tmp_path / "est_only.txt").read().splitlines()) == 3 and open(tmp_path / "gt_empty.txt").read() == ""
