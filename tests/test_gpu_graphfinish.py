"""GPU: the end of a pose-graph run (cfear_graph_align_batch, cfear_graph_map_batch; csrc/graphfinish.hip) against the NumPy
restatement tests/graphfinish_cpu.py (pinned by tests/test_graphfinish_cpu.py).

Exact, no tolerance: every bit of both maps and of their ranges; the poses Align rewrites, given the library's own Tgtalign
(behind the SVD both sides run one fp64 operation sequence without contraction); a graph's results whatever batch it is in.
Bounded, with the bound derived where it is used: Tgtalign itself (the two sides sum H in different orders, check_align) and
the ATE (a split sum against a serial one)."""
import os
import subprocess

import numpy as np
import pytest

import graphfinish_cpu as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _api():
    from tbv_slam_public_amd import api
    return api


def _L():
    from tbv_slam_public_amd import _lib as L
    return L


T = None    # the kernel's tile, read from the library's mirror (CFEAR_GRAPH_MAP_TILE); set by map_batch()


# ---- the map ----------------------------------------------------------------------------------------------------------------
_MAP = {}


def map_batch():
    """4 graphs of 1, 2, 5 and 7 nodes; cloud sizes 0, 1, T - 1, T, T + 1 and 2 T + 3; poses with roll, pitch and z; ground
    truth on every node (graphs 0 and 3), on no node (graph 1) and on a strict subset (graph 2).  Built once."""
    global T
    if _MAP:
        return _MAP
    T = _L().GRAPH_MAP_TILE
    rng = np.random.default_rng(7)
    sizes = [[T + 1], [2 * T + 3, 0], [T, 1, T - 1, 2 * T + 3, 0], [T - 1, T, 0, T + 1, 1, 2 * T + 3, T]]
    has = [[1], [0, 0], [1, 0, 1, 0, 0], [1] * 7]
    graphs = []
    for g, ns in enumerate(sizes):
        pose = lambda: G.euler_pose(*rng.uniform(-80, 80, 2), rng.uniform(-3, 3), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-3.1, 3.1))
        poses, gt = np.array([pose() for _ in ns]), np.array([pose() for _ in ns])
        clouds = []
        for n in ns:
            c = rng.uniform(-150, 150, (n, 4)).astype(np.float32)
            c[:, 2] = rng.uniform(-2, 2, n)
            c[:, 3] = rng.integers(0, 255, n)
            clouds.append(c)
        graphs.append(dict(poses=poses, gt=gt, has=np.array(has[g], np.uint8), clouds=clouds))
    _MAP.update(graphs=graphs, want={})
    return _MAP


def map_want(order, skip, want_gt):
    """The restatement's maps and ranges for the graphs `order` of map_batch(), computed once per combination."""
    b = map_batch()
    key = (tuple(order), skip, want_gt)
    if key not in b["want"]:
        maps = [G.graph_map(g["poses"], g["gt"], g["has"], g["clouds"], skip, want_gt) for g in (b["graphs"][k] for k in order)]
        summ = np.zeros(len(order), _L().GRAPH_MAP_SUMMARY_DTYPE)
        summ["map_points"], summ["map_gt_points"] = [len(m[0]) for m in maps], [len(m[1]) for m in maps]
        summ["map_offset"][1:], summ["map_gt_offset"][1:] = np.cumsum(summ["map_points"])[:-1], np.cumsum(summ["map_gt_points"])[:-1]
        b["want"][key] = (np.concatenate([m[0] for m in maps]), np.concatenate([m[1] for m in maps]), summ)
    return b["want"][key]


def flat(order):
    gs = [map_batch()["graphs"][k] for k in order]
    off = np.concatenate([[0], np.cumsum([len(g["poses"]) for g in gs])]).astype(np.int64)
    clouds = [c for g in gs for c in g["clouds"]]
    coff = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return (np.ascontiguousarray(np.concatenate([g["poses"] for g in gs])), np.ascontiguousarray(np.concatenate([g["gt"] for g in gs])),
            np.ascontiguousarray(np.concatenate([g["has"] for g in gs])), off, np.ascontiguousarray(np.concatenate(clouds)), coff)


def run_map(order, skip, want_gt, in_dev=False, out_dev=False, cap=None, cap_gt=None, off=None, coff=None, pattern=None):
    """cfear_graph_map_batch on caller-owned buffers -> (rc, map, map_gt, summaries); the maps as host arrays, as the call left
    them (pre-filled with `pattern` when given)."""
    import ctypes as C
    import torch
    L, api = _L(), _api()
    poses, gt, has, off0, xyzi, coff0 = flat(order)
    off, coff = off0 if off is None else off, coff0 if coff is None else coff
    want = map_want(order, max(skip, 1), want_gt)
    cap = len(want[0]) if cap is None else cap
    cap_gt = len(want[1]) if cap_gt is None else cap_gt
    m, mg = np.zeros((cap, 4), np.float32), np.zeros((cap_gt, 4), np.float32)
    if pattern is not None:
        m[:], mg[:] = pattern, pattern
    ctx = api.default_context()
    keep = []

    def dev(a):
        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.zeros(16, dtype=torch.uint8).cuda()
        keep.append(t)
        return t
    ins = [dev(a) if in_dev else a for a in (poses, gt, has, xyzi)]
    outs = [dev(a) if out_dev else a for a in (m, mg)]
    ptr = lambda x: x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data
    summ = np.zeros(len(order), L.GRAPH_MAP_SUMMARY_DTYPE)
    par = L.GraphMapParams(skip, int(want_gt))
    rc = ctx._lib.cfear_graph_map_batch(ctx.h, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), off.ctypes.data, len(poses), len(order), ptr(ins[3]),
                                        coff.ctypes.data, len(xyzi), C.byref(par), ptr(outs[0]) if cap else None, cap,
                                        ptr(outs[1]) if cap_gt and want_gt else None, cap_gt, summ.ctypes.data)
    if out_dev:
        torch.cuda.synchronize()
        m = outs[0].cpu().numpy()[:cap * 16].view(np.float32).reshape(-1, 4)
        mg = outs[1].cpu().numpy()[:cap_gt * 16].view(np.float32).reshape(-1, 4)
    return rc, m, mg, summ


@pytest.mark.parametrize("skip", [1, 2, 3])
def test_map_every_bit_equals_the_restatement(skip):
    """skip_frames 2 ends on the last node of the 5- and 7-node graphs (an empty cloud in the former) and before the last of
    the 2-node graph; 3 ends on the last node of the 7-node graph and before the last of the 5-node graph, where it takes one
    node with ground truth and one without."""
    order = [0, 1, 2, 3]
    for want_gt in (True, False):
        want_m, want_g, want_s = map_want(order, skip, want_gt)
        assert len(want_m) > 2 * T and (not want_gt or 0 < len(want_g) < len(want_m))
        for in_dev in (False, True):
            for out_dev in (False, True):
                rc, m, mg, s = run_map(order, skip, want_gt, in_dev, out_dev)
                where = (skip, want_gt, in_dev, out_dev)
                assert rc == 0, where
                assert s.tobytes() == want_s.tobytes(), (where, s, want_s)
                assert m.tobytes() == want_m.tobytes(), (where, np.argwhere(m != want_m)[:4])
                if want_gt:
                    assert mg.tobytes() == want_g.tobytes(), (where, np.argwhere(mg != want_g)[:4])
    assert map_want(order, skip, False)[2]["map_gt_points"].sum() == 0


def test_map_ranges_do_not_depend_on_the_batch():
    """The same graphs in reversed batch order, and each graph alone: every graph's two ranges hold the same bits."""
    skip = 2
    _, m, mg, s = run_map([0, 1, 2, 3], skip, True)
    cut = lambda a, o, n: a[int(o):int(o) + int(n)].tobytes()
    _, mr, mgr, sr = run_map([3, 2, 1, 0], skip, True, in_dev=True)
    for g in range(4):
        a, b = s[g], sr[3 - g]
        assert a["map_points"] == b["map_points"] and a["map_gt_points"] == b["map_gt_points"]
        assert cut(m, a["map_offset"], a["map_points"]) == cut(mr, b["map_offset"], b["map_points"])
        assert cut(mg, a["map_gt_offset"], a["map_gt_points"]) == cut(mgr, b["map_gt_offset"], b["map_gt_points"])
        rc, m1, mg1, s1 = run_map([g], skip, True)
        assert rc == 0 and s1[0]["map_offset"] == 0 and s1[0]["map_gt_offset"] == 0
        assert m1.tobytes() == cut(m, a["map_offset"], a["map_points"]) and mg1.tobytes() == cut(mg, a["map_gt_offset"], a["map_gt_points"])


def test_map_capacity_and_refusals():
    L = _L()
    order = [0, 1, 2, 3]
    want_m, want_g, want_s = map_want(order, 1, True)
    for out_dev in (False, True):
        for cap, cap_gt in ((len(want_m) - 1, len(want_g)), (len(want_m), len(want_g) - 1), (0, 0)):
            rc, m, mg, s = run_map(order, 1, True, out_dev=out_dev, cap=cap, cap_gt=cap_gt, pattern=-7.25)
            assert rc == L.ERR_CAPACITY
            assert s.tobytes() == want_s.tobytes()                       # the full counts: the caller can size the buffers
            assert (m == -7.25).all() and (mg == -7.25).all()            # nothing was written
    # without the ground-truth map its capacity does not matter
    rc, m, _, s = run_map(order, 1, False, cap_gt=0)
    assert rc == 0 and m.tobytes() == map_want(order, 1, False)[0].tobytes()
    rc, m, _, _ = run_map(order, 0, True, pattern=3.5)                   # the reference would compute % 0
    assert rc == L.ERR_INVALID_ARGUMENT and (m == 3.5).all()
    _, _, _, off, _, coff = flat(order)
    for bad_off, bad_coff in ((off + 1, None), (np.concatenate([off[:-1], [off[-1] - 1]]), None), (off[[0, 2, 1, 3, 4]], None),
                              (None, coff + 1), (None, np.concatenate([coff[:-1], [coff[-1] + 1]])), (None, coff[::-1].copy())):
        rc, m, _, _ = run_map(order, 1, True, off=bad_off, coff=bad_coff, pattern=3.5)
        assert rc == L.ERR_INVALID_ARGUMENT and (m == 3.5).all()
    # host and device buffers mixed among the inputs
    import ctypes as C
    import torch
    api = _api()
    ctx = api.default_context()
    poses, gt, has, off, xyzi, coff = flat(order)
    d = torch.from_numpy(poses).cuda()
    summ = np.zeros(4, L.GRAPH_MAP_SUMMARY_DTYPE)
    par = L.GraphMapParams(1, 1)
    out = np.zeros((len(want_m), 4), np.float32)
    rc = ctx._lib.cfear_graph_map_batch(ctx.h, d.data_ptr(), gt.ctypes.data, has.ctypes.data, off.ctypes.data, len(poses), 4, xyzi.ctypes.data,
                                        coff.ctypes.data, len(xyzi), C.byref(par), out.ctypes.data, len(out), out.ctypes.data, len(out),
                                        summ.ctypes.data)
    assert rc == L.ERR_INVALID_ARGUMENT


def test_map_through_the_mirror():
    import torch
    api = _api()
    gs = map_batch()["graphs"]
    want_m, want_g, want_s = map_want([0, 1, 2, 3], 2, True)
    tri = [(g["poses"], g["gt"], g["has"]) for g in gs]
    m, mg, s = api.graph_map_batch(tri, [g["clouds"] for g in gs], skip_frames=2)
    assert m.tobytes() == want_m.tobytes() and mg.tobytes() == want_g.tobytes() and s.tobytes() == want_s.tobytes()
    dm, dmg, s = api.graph_map_batch(tri, [[torch.from_numpy(c).cuda() for c in g["clouds"]] for g in gs], skip_frames=2, device_out=True)
    assert dm.is_cuda and dm.cpu().numpy().tobytes() == want_m.tobytes() and dmg.cpu().numpy().tobytes() == want_g.tobytes()
    pg = api.PoseGraph(poses=gs[2]["poses"], gt=gs[2]["gt"], has_gt=gs[2]["has"], clouds=gs[2]["clouds"])
    one = map_want([2], 3, True)
    m, mg = pg.Map(skip_frames=3)
    assert m.tobytes() == one[0].tobytes() and mg.tobytes() == one[1].tobytes()
    m, mg = pg.Map(skip_frames=3, want_gt_map=False)
    assert m.tobytes() == one[0].tobytes() and mg is None


# ---- Align ------------------------------------------------------------------------------------------------------------------
KERNEL_TREE = 10      # graph_align_sums' tree behind a thread's strided serial sum: 4 butterfly levels in a 16-lane row, the 4 rows
                      # of a wave in order (3 additions), the 4 waves in order (3 additions)
_ALIGN = {}


def align_cases():
    if _ALIGN:
        return _ALIGN
    rng = np.random.default_rng(12)
    est, gt = G.lap(300, 1, planar=True)                              # more than one node per thread: 300 > 256
    _ALIGN["planar lap"] = (est, gt, np.ones(300, np.uint8))
    est, gt = G.lap(70, 2, planar=False)
    _ALIGN["3-D lap"] = (est, gt, np.ones(70, np.uint8))
    est, gt = G.lap(41, 3, planar=False)
    has = (rng.uniform(size=41) < 0.5).astype(np.uint8)
    has[:3] = [1, 0, 1]
    _ALIGN["ground truth on a subset"] = (est, gt, has)
    est, gt = G.lap(9, 4)
    _ALIGN["no ground truth"] = (est, gt, np.zeros(9, np.uint8))
    one = np.zeros(9, np.uint8)
    one[5] = 1
    _ALIGN["one ground-truth node"] = (est, gt, one)
    # all ground-truth positions on one line (and one node off it that has none): H has rank 1
    line = np.array([G.euler_pose(1.5 * k, 0.5 * 1.5 * k, 0.0, 0, 0, 0.1 * k) for k in range(12)])
    off_line = line.copy()
    off_line[:, :2] += rng.normal(0, 0.1, (12, 2))
    line[7, :3] = [3.0, -8.0, 1.0]
    has = np.ones(12, np.uint8)
    has[7] = 0
    _ALIGN["collinear"] = (off_line, line, has)
    # the edges of the sums' workgroup of 256 threads: one node per thread, one node more, two nodes (one with ground truth:
    # two are always collinear), and a 300-node graph in which one whole wavefront of the workgroup counts nothing
    for n, seed in ((256, 5), (257, 6)):
        est, gt = G.lap(n, seed, planar=False)
        _ALIGN["%d nodes" % n] = (est, gt, np.ones(n, np.uint8))
    est, gt = G.lap(2, 7)
    _ALIGN["two nodes"] = (est, gt, np.array([0, 1], np.uint8))
    est, gt = G.lap(300, 8, planar=False)
    has = np.ones(300, np.uint8)
    has[64:128] = 0
    _ALIGN["a wavefront without ground truth"] = (est, gt, has)
    return _ALIGN


def run_align(names, device=False):
    """cfear_graph_align_batch on the cases `names` -> (poses per case as the call left them, summaries)."""
    import torch
    L, api = _L(), _api()
    cs = [align_cases()[k] for k in names]
    poses, gt, has = (np.ascontiguousarray(np.concatenate([c[k] for c in cs])) for k in range(3))
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in cs])]).astype(np.int64)
    summ = np.zeros(len(cs), L.GRAPH_ALIGN_SUMMARY_DTYPE)
    ctx = api.default_context()
    if device:
        d = [torch.from_numpy(a).cuda() for a in (poses, gt, has)]
        ptrs = [t.data_ptr() for t in d]
    else:
        ptrs = [a.ctypes.data for a in (poses, gt, has)]
    ctx.check(ctx._lib.cfear_graph_align_batch(ctx.h, ptrs[0], ptrs[1], ptrs[2], off.ctypes.data, len(poses), len(cs), summ.ctypes.data))
    if device:
        torch.cuda.synchronize()
        poses = d[0].cpu().numpy()
    return [poses[off[k]:off[k + 1]] for k in range(len(cs))], summ


def check_align(name, s, est, gt, has):
    """Tgtalign against the restatement's own, with check_alignment's bound (tests/test_gpu_kitti_eval.py) as
    graphfinish_cpu.alignment_bound restates it.  Its depth constant is adapted to this kernel's reduction: a thread sums
    ceil(n / 256) nodes serially, then the KERNEL_TREE levels above; NumPy's side keeps its 22."""
    has = has.astype(bool)
    depth = (len(est) + 255) // 256 + KERNEL_TREE + G.NUMPY_DEPTH
    b_r, b_t = G.alignment_bound(gt[has, :3], est[has, :3], depth)
    want = G.align(est, gt, has)[1].reshape(3, 4)
    got = s["align"].reshape(3, 4)
    d_r, d_t = np.abs(got[:, :3] - want[:, :3]).max(), np.abs(got[:, 3] - want[:, 3]).max()
    print("%-28s |dR| %.3e (bound %.3e)  |dt| %.3e (bound %.3e)" % (name, d_r, b_r, d_t, b_t))
    assert d_r <= b_r and d_t <= b_t, (name, d_r, b_r, d_t, b_t)
    r = got[:, :3]
    u = 2.0 ** -53
    assert np.abs(r @ r.T - np.eye(3)).max() <= max(b_r, 16 * u) and abs(np.linalg.det(r) - 1.0) <= max(b_r, 16 * u), name


def check_ate(name, s, poses, gt, has):
    """The library splits the sum over its lanes, the restatement adds serially: n * 2^-53 * sum |terms| bounds the two."""
    terms = G.ate_terms(poses, gt, has)
    want = G.ate_of(poses, gt, has)
    bound = len(terms) * 2.0 ** -53 * sum(terms)
    print("%-28s ate %.6e  |d| %.3e (bound %.3e)" % (name, s["ate"], abs(s["ate"] - want), bound))
    assert abs(s["ate"] - want) <= bound, (name, s["ate"], want, bound)
    assert s["n_gt"] == len(terms)


def test_align_against_the_restatement():
    L = _L()
    names = list(align_cases())
    new, summ = run_align(names)
    for k, name in enumerate(names):
        est, gt, has = align_cases()[name]
        s = summ[k]
        if name == "collinear":
            assert s["status"] == L.ERR_SOLVER
            assert new[k].tobytes() == est.tobytes()                  # untouched: not even the identity's rewrite
            assert (s["align"] == G.IDENTITY).all()
            check_ate(name, s, est, gt, has)
            continue
        assert s["status"] == L.OK, name
        if has.sum() >= 3:
            check_align(name, s, est, gt, has)
        else:                                                         # H is exactly zero: R = I, t = cB - cA on both sides
            want = G.align(est, gt, has)[1]
            assert (s["align"].reshape(3, 4)[:, :3] == np.eye(3)).all()
            assert np.abs(s["align"] - want).max() <= 2.0 ** -52 * np.abs(est[:, :3]).max(), name
        # behind the SVD: the restatement, given the library's own Tgtalign, is one fixed fp64 sequence
        want_poses = G.align_apply(est, s["align"])
        assert new[k].tobytes() == want_poses.tobytes(), (name, np.argwhere(new[k] != want_poses)[:4])
        assert np.abs(np.linalg.norm(new[k][:, 3:], axis=1) - 1.0).max() <= 4.5e-16
        check_ate(name, s, new[k], gt, has)
    k = names.index("no ground truth")
    assert (summ[k]["align"] == G.IDENTITY).all() and summ[k]["ate"] == 0.0 and summ[k]["n_gt"] == 0
    k = names.index("one ground-truth node")
    assert summ[k]["n_gt"] == 1 and summ[k]["ate"] <= 1e-13
    for name in ("planar lap", "3-D lap", "ground truth on a subset"):
        assert summ[names.index(name)]["ate"] < 0.2                    # the laps' noise is 0.05 m per axis


def test_align_does_not_depend_on_the_batch_or_the_memory():
    names = list(align_cases())
    new, summ = run_align(names)
    rev, srev = run_align(names[::-1], device=True)
    assert srev[::-1].tobytes() == summ.tobytes()
    for k in range(len(names)):
        assert rev[len(names) - 1 - k].tobytes() == new[k].tobytes(), names[k]
        one, s1 = run_align([names[k]])
        assert one[0].tobytes() == new[k].tobytes() and s1.tobytes() == summ[k:k + 1].tobytes(), names[k]


def test_align_through_the_mirror():
    api = _api()
    names = ["3-D lap", "collinear", "no ground truth"]
    new, summ = run_align(names)
    out = api.graph_align_batch([align_cases()[k] for k in names])
    for k in range(3):
        assert out[k][0].tobytes() == new[k].tobytes()
        assert out[k][1]["align"].tobytes() == summ[k]["align"].tobytes() and out[k][1]["status"] == summ[k]["status"]
    assert api.graph_align_batch([]) == []
    empty = api.graph_align_batch([(np.zeros((0, 7)), np.zeros((0, 7)), [])])
    assert empty[0][0].shape == (0, 7) and empty[0][1]["status"] == 0 and empty[0][1]["ate"] == 0.0


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_align_output_and_evaluate(tmp_path):
    """PoseGraph: Align, OutputGraph, kitti_read of both files, eval_trajectories(alignment="none").  The evaluator's ATE is the
    RMS of the distances between the (normalised) positions in the two files; the mean of the same distances cannot exceed it
    (nor can the RMS exceed the largest).  And the mean distance between the files' own positions is Align's ate, up to the
    6 decimals of the files."""
    import kitti_eval_cpu as K
    from test_gpu_kitti_eval import TOL
    api = _api()
    est, gt, has = align_cases()["ground truth on a subset"]
    pg = api.PoseGraph(poses=est, gt=gt, has_gt=has, stamps=np.arange(len(est)) + 1547131046353776000,
                       est_output_dir=str(tmp_path / "est"), gt_output_dir=str(tmp_path / "gt"))
    s = pg.Align()
    assert s["status"] == 0 and s["n_gt"] == has.sum() and pg.ate == s["ate"]
    pg.OutputGraph()
    pg.SaveGraphString(str(tmp_path / "graph.txt"))
    e, g = api.kitti_read(str(tmp_path / "est" / "00.txt")), api.kitti_read(str(tmp_path / "gt" / "00.txt"))
    assert len(e) == len(g) == has.sum()
    lines = open(tmp_path / "graph.txt").read().split("\n")
    assert len(lines) == 2 * len(est) + 1 and all(ln == "" for ln in lines[1::2]) and lines[0].endswith(" 1547131046353776000")
    # the files hold the aligned poses of the nodes with ground truth, at 6 decimals
    rows = np.array([G.to_rows(p) for p in pg.poses[has.astype(bool)]])
    assert np.abs(e - rows).max() <= 0.5e-6 + 1e-13
    d_files = np.linalg.norm(e[:, 3::4] - g[:, 3::4], axis=1)
    assert abs(d_files.mean() - s["ate"]) <= 2 * np.sqrt(3) * 0.5e-6
    summ, _ = api.eval_trajectories([e], [g], alignment="none", want_rows=False)
    d = np.linalg.norm(K.normalise(e)[:, 3::4] - K.normalise(g)[:, 3::4], axis=1)
    rms = np.sqrt((d * d).mean())
    print("Align's ate %.6f m; files: mean %.6f m; evaluator (normalised): ATE %.6f m, NumPy RMS %.6f, mean %.6f, max %.6f"
          % (s["ate"], d_files.mean(), summ[0]["ate"], rms, d.mean(), d.max()))
    assert summ[0]["status"] == 0 and abs(summ[0]["ate"] - rms) <= 100 * TOL
    assert d.mean() <= summ[0]["ate"] + 100 * TOL and summ[0]["ate"] <= d.max() + 100 * TOL


def test_cpp_wrapper_runs(tmp_path):
    exe = str(tmp_path / "graphfinish_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "graphfinish_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    out = subprocess.run([exe, "run", str(tmp_path)], check=True, capture_output=True, text=True, timeout=120).stdout.split()
    # graph 0: an exact rigid motion of its ground truth, 5 of 6 nodes with ground truth; graph 1: three nodes on one line
    assert out[:4] == ["0", str(_L().ERR_SOLVER), "5", "3"], out
    assert float(out[4]) <= 1e-13 and abs(float(out[5]) - 1.0) <= 1e-13, out
    # skip_frames 2: nodes 0, 2, 4 of graph 0 hold 1 + 3 + 5 points, node 4 has no ground truth; graph 1 adds 2 + 2 to both maps
    assert out[6:] == ["9", "4", "9", "8"], out
    assert len(open(tmp_path / "graph.txt").read().split("\n")) == 13
    assert len(open(tmp_path / "est.txt").read().splitlines()) == len(open(tmp_path / "gt.txt").read().splitlines()) == 5
    assert len(open(tmp_path / "est_only.txt").read().splitlines()) == 3 and open(tmp_path / "gt_empty.txt").read() == ""
