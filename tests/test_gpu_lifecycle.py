"""GPU: the life cycle of the long-lived handles (OdometryKeyframeFuser, ScanTable, CandidatePipe, CeresCost,
RSCManagerNative) in one private context: each is created and closed without being used, and created, used, closed and
created again -- the second object, which gets memory the first one gave back, must return what the first one returned,
bit for bit.  The context is closed last, with slabs on its free list and workspaces grown by everything before."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_FRAMES = 3


@pytest.fixture(scope="module")
def ctx():
    from tbv_slam_public_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _odometry_run(ctx, frames):
    """-> (frame infos, the scans of stream 0's last two frames) of a fresh two-stream odometry that is closed again"""
    from tbv_slam_public_amd import api
    od = api.OdometryKeyframeFuser(2, frames.shape[2], frames.shape[3], ctx=ctx)
    infos, scans = [], []
    for f in range(N_FRAMES):
        infos.append(od.process(frames[f]))                        # host images: the staging buffer is allocated on first use
        if f > 0:
            scans.append(od.node(0)["scan"])
    od.close()
    return infos, scans


@pytest.fixture(scope="module")
def world(ctx):
    """Two odometry streams over the smallest synth sweep, run once: the frames, what the run returned, and two scans of it
    (stream 0, frames 1 and 2) with the pose of the second in the first."""
    from tbv_slam_public_amd import synth
    seqs = [synth.scene_v1(sd, N_FRAMES)[0] for sd in (0, 1)]
    frames = np.stack([np.stack([s[f] for s in seqs]) for f in range(N_FRAMES)])
    infos, scans = _odometry_run(ctx, frames)
    a, b = infos[1]["pose"][0], infos[2]["pose"][0]
    c, s = np.cos(a[2]), np.sin(a[2])
    d = b[:2] - a[:2]
    rel = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], b[2] - a[2]])
    assert all(sc.GetSize() > 100 for sc in scans)
    return dict(frames=frames, infos=infos, scans=scans, rel=rel)


def _reg(ctx):
    from tbv_slam_public_amd import api
    reg = api.n_scan_normal_reg("P2L", ctx=ctx)
    reg.SetParameters(4, 10)
    return reg


def _cands(world):
    """scan 1 against scan 0 and the other way round, each from a guess beside the odometry's answer"""
    from tbv_slam_public_amd import api
    x, y, t = world["rel"]
    back = np.array([-np.cos(t) * x - np.sin(t) * y, np.sin(t) * x - np.cos(t) * y, -t])
    return api.ScanTable.candidates([0, 1], [1, 0], np.stack([world["rel"], back]) + [0.2, -0.1, 0.01])


def test_odometry(ctx, world):
    from tbv_slam_public_amd import api
    api.OdometryKeyframeFuser(2, 400, 3360, ctx=ctx).close()                          # never used: no staging buffer yet
    # [range bins][azimuths] input: the rotated-image buffer is allocated by the first frame that needs it -- none here
    api.OdometryKeyframeFuser(2, 3360, 400, api.odometry_params(rotate_ccw=1), ctx=ctx).close()
    api.OdometryKeyframeFuser(1, 400, 3360, api.odometry_params(keep_nodes=1, estimate_cov_by_sampling=1), ctx=ctx).close()
    infos, scans = _odometry_run(ctx, world["frames"])
    for f in range(N_FRAMES):
        assert infos[f].tobytes() == world["infos"][f].tobytes(), f
    assert (world["infos"][2]["reg_status"] == 0).all() and (world["infos"][2]["n_cells"] > 100).all()
    for mine, first in zip(scans, world["scans"]):
        assert mine.GetCells().tobytes() == first.GetCells().tobytes()
    for s in scans:
        s.close()


def test_scan_table(ctx, world):
    from tbv_slam_public_amd import api
    reg, cands = _reg(ctx), _cands(world)
    api.ScanTable(world["scans"], ctx=ctx).close()
    table = api.ScanTable(world["scans"], ctx=ctx)
    assert len(table) == 2
    first = reg.RegisterCandidates(table, cands)
    assert (first["status"] == 0).all()
    table.close()                                                                     # before the scans it names
    assert world["scans"][0].GetSize() > 100
    copies = [api.MapPointNormal(cells=s.GetCells(), ctx=ctx) for s in world["scans"]]
    table = api.ScanTable(copies, ctx=ctx)
    for s in copies:                                                                  # after the scans it names: it keeps them alive
        s.close()
    other = api.MapPointNormal(cells=world["scans"][0].GetCells()[:50], ctx=ctx)       # a new scan must not get one of their slabs
    assert reg.RegisterCandidates(table, cands).tobytes() == first.tobytes()
    table.close()
    other.close()


@pytest.mark.parametrize("graph", [False, True])
def test_candidate_pipe(ctx, world, graph):
    from tbv_slam_public_amd import api
    reg, cands = _reg(ctx), _cands(world)
    table = api.ScanTable(world["scans"], ctx=ctx)
    ref = reg.RegisterCandidates(table, cands)
    api.CandidatePipe(reg, table, 2, None, 0, 1, depth=2, graph=graph).close()
    for _ in range(2):
        pipe = api.CandidatePipe(reg, table, 2, None, 0, 1, depth=2, graph=graph, timing=True)
        assert pipe.collect(pipe.submit(cands)).tobytes() == ref.tobytes()
        if graph:                                   # the other slot captures too, then another size replaces the first slot's capture
            assert pipe.collect(pipe.submit(cands)).tobytes() == ref.tobytes()
            assert pipe.collect(pipe.submit(cands[:1])).tobytes() == ref[:1].tobytes()
            assert pipe.stats()["graph_slots"] == 2
        tickets = [pipe.submit(cands), pipe.submit(cands[1:])]                         # both slots in flight (replays, with graph)
        assert pipe.collect(tickets[1]).tobytes() == ref[1:].tobytes()
        assert pipe.collect(tickets[0]).tobytes() == ref.tobytes()
        pipe.close()
    table.close()


def test_ceres_cost(ctx, world):
    from tbv_slam_public_amd import api
    reg = _reg(ctx)
    poses = np.stack([np.zeros(3), world["rel"]])
    api.CeresCost(reg, world["scans"], poses, itr=1).close()
    x = world["rel"] + [0.05, -0.02, 0.003]
    got = []
    for _ in range(2):
        cc = api.CeresCost(reg, world["scans"], poses, itr=1)
        pairs, w = cc.blocks()
        H, g, cost = cc.normal_eq(x)
        r, J = cc.evaluate(x)
        cc.close()
        got.append(b"".join(np.ascontiguousarray(v).tobytes() for v in (pairs, w, H, g, np.float64(cost), r, J)))
        assert pairs.shape[0] > 50
    assert got[0] == got[1]
    ok, score, res = reg.GetCost(world["scans"], poses)                               # cfear_get_cost makes and drops a cost of its own
    assert ok and reg.GetCost(world["scans"], poses)[1] == score


def test_sc_manager_grows_its_database(ctx):
    """More than 256 nodes at the smallest descriptor geometry: the database is allocated by the first node and grows once,
    at node 256.  The candidates of every node, before and after, are those of the Python manager (rtol 1e-12 on the one
    sum the two compute separately, as in test_gpu_sc_managers)."""
    from tbv_slam_public_amd import api, synth
    n = 264
    clouds, poses = synth.sc_graph(n, seed=5, points=250)
    par = api.sc_params(num_ring=1, num_sector=8)
    api.RSCManagerNative(par=par, ctx=ctx).close()                                    # no database yet
    runs = []
    for _ in range(2):
        nat = api.RSCManagerNative(par=par, ctx=ctx)
        out = []
        for c, T in zip(clouds[:40], poses[:40]):
            nat.makeAndSaveScancontextAndKeysRadarCloud(c, T)
            out.append(nat.detectLoopClosureID())
        runs.append(out)
        if len(runs) == 2:
            break
        nat.close()
    bits = [[[{k: np.asarray(v).tobytes() for k, v in c.items()} for c in node] for node in run] for run in runs]
    assert bits[0] == bits[1] and sum(len(o) for o in runs[0]) > 20
    py = api.RSCManager(par=par, ctx=ctx)
    exp = []
    for c, T in zip(clouds, poses):
        py.makeAndSaveScancontextAndKeysRadarCloud(c, T)
        exp.append(py.detectLoopClosureID())
    got = runs[1]
    for c, T in zip(clouds[40:], poses[40:]):                                         # the second manager goes on past 256 nodes
        nat.makeAndSaveScancontextAndKeysRadarCloud(c, T)
        got.append(nat.detectLoopClosureID())
    assert nat.size() == n
    nat.close()
    assert sum(len(e) for e in exp[:256]) > 100 and all(len(e) > 0 for e in exp[256:])
    for i, (g, e) in enumerate(zip(got, exp)):
        for k in ("nn_idx", "argmin_shift", "min_dist_sc"):
            assert [c[k] for c in g] == [c[k] for c in e], (i, k)
        np.testing.assert_allclose([c["min_dist"] for c in g], [c["min_dist"] for c in e], rtol=1e-12, atol=1e-15, err_msg=str(i))


def test_scans_go_last(ctx, world):
    """The scans of the first odometry run outlived everything made from them; they go just before the context."""
    for s in world["scans"]:
        assert s.GetSize() > 100
        s.close()
