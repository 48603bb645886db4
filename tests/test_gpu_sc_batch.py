"""GPU: Scan Context for a batch of graphs in one call (cfear_sc_detect_batch).  Cloud mode against cfear_sc_detect_sequence of
every graph alone, byte for byte, over the manager's modes, query chunks that end inside graphs and on their boundaries,
host and device inputs and outputs; both modes against the streaming cfear_sc_manager fed node by node and, in cloud mode,
the oracle-driven restatement tests/sc_manager_ref.py; the refusals; the demos that call it.

The graphs are the smallest that reach every branch: an empty graph, graphs that never pass the gate (n <= 3), one whose
first detection is node 7 (odometry) or 5 (vanilla), a lap of 75 nodes that is revisited, and more than 100 gate-passing
calls, so the vanilla tree is rebuilt twice per graph and a counter that is not reset per graph would show.  Nodes 20 and 21
of the long graph see the same cloud, so lists hold equal min_dist and the ranking kernel's tie rule is exercised."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from tests import sc_manager_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

NODES = [0, 1, 2, 3, 9, 40, 120]
N_DETECT = [0, 1, 2, 3, 8, 40, 119]
KWS = [dict(), dict(odometry_coupled_closure=False), dict(augment_sc=False, n_candidates=5, num_candidates_from_tree=2),
       dict(n_candidates=1)]


@functools.lru_cache(None)
def _graphs():
    from tbv_slam_public_amd import synth
    out = []
    for g, n in enumerate(NODES):
        clouds, poses = synth.sc_graph(n, seed=40 + g, points=120, step=2.5, radius=30.0)
        if n == 120:
            clouds[21] = clouds[20].copy()
        out.append((clouds, poses))
    return out


def _ids():
    """0, 1, ... in every graph (the same ids in all of them), but offset and gapped in the 40-node graph."""
    ids = [np.arange(n, dtype=np.int32) for n in NODES]
    ids[5] = ids[5] + 100
    ids[5][25:] += 2
    return ids


def _sequence_records(clouds, poses, ids, n_agg, n_detect, **kw):
    """cfear_sc_detect_sequence of one graph into zeroed rows -> (records [n_detect, n_candidates], counts)."""
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    ctx = api.default_context()
    p = api.sc_manager_params(None, **kw)
    arr, keep = api._sc_nodes(clouds, poses, None, ids)
    out = np.zeros((max(n_detect, 1), p.n_candidates), L.SC_CANDIDATE_DTYPE)
    n_out = np.zeros(max(n_detect, 1), np.int32)
    ctx.check(ctx._lib.cfear_sc_detect_sequence(ctx.h, C.byref(p), arr, len(clouds), n_agg, n_detect, out.ctypes.data, n_out.ctypes.data))
    del keep
    return out[:n_detect], n_out[:n_detect]


def _batch_records(n_agg=1, chunk=0, flat=None, device_out=False, **kw):
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    ctx = api.default_context()
    flat = flat or api.sc_flatten_graphs(_graphs(), _ids())
    ctx.set_option(L.OPT_SC_QUERY_CHUNK, chunk)
    try:
        out, n_out, row = api.sc_detect_batch(flat=flat, n_aggregate=n_agg, n_detect=N_DETECT, ctx=ctx, records=not device_out,
                                              device_out=device_out, **kw)
    finally:
        ctx.set_option(L.OPT_SC_QUERY_CHUNK, 0)
    if device_out:
        assert out.is_cuda and n_out.is_cuda
        out, n_out = out.cpu().numpy().view(L.SC_CANDIDATE_DTYPE)[:, :, 0], n_out.cpu().numpy()
    return out, n_out, row


def _has_tie_of_20_and_21(rec, cnt):
    for r, c in zip(rec, cnt):
        idx = list(r["nn_idx"][:c])
        if 20 in idx and 21 in idx and r["min_dist"][idx.index(20)] == r["min_dist"][idx.index(21)]:
            return True
    return False


@pytest.mark.parametrize("n_agg", [1, 0])
@pytest.mark.parametrize("kw", KWS, ids=["default", "vanilla", "noaug_k2_c5", "c1"])
def test_cloud_mode_equals_the_sequence_call_byte_for_byte(kw, n_agg):
    out, n_out, row = _batch_records(n_agg, **kw)
    assert list(row) == list(np.concatenate([[0], np.cumsum(N_DETECT)]))
    ids = _ids()
    for g, (clouds, poses) in enumerate(_graphs()):
        rec, cnt = _sequence_records(clouds, poses, ids[g], n_agg, N_DETECT[g], **kw)
        got, gcnt = out[row[g]:row[g + 1]], n_out[row[g]:row[g + 1]]
        np.testing.assert_array_equal(gcnt, cnt, err_msg="graph %d" % g)
        assert got.tobytes() == rec.tobytes(), "graph %d" % g      # the zeroed tails included
    big, bcnt = out[row[6]:row[7]], n_out[row[6]:row[7]]
    # the restatement alone (tests/sc_manager_ref.py, tree="linear") finds 339 (odometry) and 345 (vanilla) candidates in the 120
    # nodes, 3 of them at node 119, which n_detect = 119 leaves out here; the next test asserts the full counts
    if kw == dict():
        assert int(bcnt.sum()) == 339 - 3
        if n_agg == 0:
            assert _has_tie_of_20_and_21(big, bcnt)
    if kw == dict(odometry_coupled_closure=False):
        assert int(bcnt.sum()) == 345 - 3
        tied = sum(len(set(r["min_dist"][:c])) < c for g in (5, 6) for r, c in zip(out[row[g]:row[g + 1]], n_out[row[g]:row[g + 1]]))
        assert tied >= 10                                          # the padded node 0, repeated
    # the graphs that never pass the gate, and the rows before a graph's first detection, are empty
    assert not n_out[:row[4]].any()
    first = 5 if kw.get("odometry_coupled_closure", True) is False else 7
    assert not n_out[row[4]:row[4] + first].any() and n_out[row[4] + first] > 0     # the 9-node graph's first detection


@pytest.mark.parametrize("kw", [dict(), dict(odometry_coupled_closure=False)], ids=["default", "vanilla"])
def test_chunks_inputs_and_outputs_give_the_same_bytes(kw):
    import torch
    from tbv_slam_public_amd import api
    ref = _batch_records(1, **kw)
    assert ref[1].sum() > 300
    for chunk in (7, 40, 1000):                                    # inside graphs and on their boundaries; inside the 40; one chunk
        out, n_out, _ = _batch_records(1, chunk=chunk, **kw)
        np.testing.assert_array_equal(n_out, ref[1], err_msg=str(chunk))
        assert out.tobytes() == ref[0].tobytes(), chunk
    flat = api.sc_flatten_graphs(_graphs(), _ids())
    flat["xyzi"] = torch.from_numpy(flat["xyzi"]).cuda()             # one device buffer
    # (chunk, the cloud buffer, the rows): device clouds to host rows, device to device, host clouds to device rows
    for chunk, f, dev_out in ((0, flat, False), (7, flat, True), (0, None, True)):
        out, n_out, _ = _batch_records(1, chunk=chunk, flat=f, device_out=dev_out, **kw)
        np.testing.assert_array_equal(n_out, ref[1])
        assert out.tobytes() == ref[0].tobytes(), (chunk, dev_out)


def _streaming(clouds, poses, ids, n_agg, n_detect, **kw):
    from tbv_slam_public_amd import api
    from tests.test_gpu_sc_sequence import _merge
    nat = api.RSCManagerNative(**kw)
    out = []
    for i in range(n_detect):
        nat.makeAndSaveScancontextAndKeysRadarCloud(_merge(clouds, poses, ids, i, n_agg), poses[i])
        out.append(nat.detectLoopClosureID())
    nat.close()
    return out


@functools.lru_cache(None)
def _restatement(g, odometry):
    clouds, poses = _graphs()[g]
    return M.reference_manager_run(M.local_maps(clouds, poses, 1, _ids()[g]), poses, odometry=odometry, tree="linear")


@pytest.mark.parametrize("odometry", [True, False], ids=["odometry", "vanilla"])
def test_cloud_mode_equals_the_streaming_manager_and_the_restatement(odometry):
    from tbv_slam_public_amd import api
    from tests.test_gpu_sc_sequence import _assert_same
    kw = dict(odometry_coupled_closure=odometry)
    got = api.sc_detect_batch(_graphs(), n_aggregate=1, ids=_ids(), **kw)          # every node detected
    assert [len(g) for g in got] == NODES
    ids = _ids()
    shifts = [0.0, -2.0, 2.0, -4.0, 4.0]
    for g in (4, 5, 6):
        clouds, poses = _graphs()[g]
        found = _assert_same(got[g], _streaming(clouds, poses, ids[g], 1, NODES[g], **kw))
        assert found > (0 if g == 4 else 50)
        exp = _restatement(g, odometry)
        for i, (a, e) in enumerate(zip(got[g], exp)):
            assert [c["nn_idx"] for c in a] == [c[2] for c in e], (g, i)
            assert [c["argmin_shift"] for c in a] == [c[3] for c in e], (g, i)
            assert [c["Taug"][1] for c in a] == [shifts[c[4]] for c in e], (g, i)
    # the figures of the restatement alone, so that the comparison is not one of empty lists: the lap is revisited
    assert sum(len(e) for e in _restatement(6, odometry)) == sum(len(a) for a in got[6]) == (339 if odometry else 345)
    assert sum(c["nn_idx"] < i - 60 for i, a in enumerate(got[6]) for c in a) == (177 if odometry else 48)


# ---- raw mode ------------------------------------------------------------------------------------------------------------
RAW_NODES = [0, 3, 40, 120]


def _sweep(cloud, azimuths, bins):
    """The node's cloud as a raw sweep uint8 [azimuths][bins]: bin = range / 0.8 m, azimuth from atan2, value = intensity."""
    img = np.zeros((azimuths, bins), np.uint8)
    r = np.hypot(cloud[:, 0], cloud[:, 1])
    b = np.floor(r / 0.8).astype(int)
    a = np.floor((np.arctan2(cloud[:, 1], cloud[:, 0]) % (2 * np.pi)) / (2 * np.pi) * azimuths).astype(int) % azimuths
    ok = b < bins
    img[a[ok], b[ok]] = cloud[ok, 3].astype(np.uint8)
    return img


@functools.lru_cache(None)
def _raw_graphs(azimuths, bins):
    from tbv_slam_public_amd import synth
    out = []
    for g, n in enumerate(RAW_NODES):
        clouds, poses = synth.sc_graph(n, seed=40 + g, points=120, step=2.5, radius=30.0)
        out.append((np.stack([_sweep(c, azimuths, bins) for c in clouds]) if n else np.zeros((0, azimuths, bins), np.uint8), poses))
    return out


def _num_exclude_recent(poses, cur):
    """ExcludeAndUpdateLikelihood's recent-node count (RadarScancontext.cpp:181-200), the policy alone."""
    if cur + 1 <= 2:
        return 2
    dist, n_ex, i = 0.0, 0, cur
    while i >= 0 and dist < 10.0:
        dist += 0.0 if i == cur else float(np.hypot(*(poses[i, :2] - poses[i + 1, :2])))
        n_ex += 1
        i -= 1
    return n_ex


@pytest.mark.parametrize("augment", [True, False], ids=["augment_ignored", "no_augment"])
@pytest.mark.parametrize("shape", [(300, 100), (360, 120)], ids=["scale2.5_area", "scale3_integer"])
def test_raw_mode_equals_the_streaming_manager(shape, augment):
    import torch
    from tbv_slam_public_amd import api
    from tests.test_gpu_sc_sequence import _assert_same
    graphs = _raw_graphs(*shape)
    raw = api.sc_raw_params(transpose=1)
    kw = dict(augment_sc=augment)
    got = api.sc_detect_batch(graphs, raw_par=raw, **kw)
    assert [len(g) for g in got] == RAW_NODES
    for g, (sweeps, poses) in enumerate(graphs):
        nat = api.RSCManagerNative(raw_par=raw, **kw)
        exp = []
        for img, T in zip(sweeps, poses):
            nat.makeAndSaveScancontextAndKeysRadarRaw(img, T)
            exp.append(nat.detectLoopClosureID())
        nat.close()
        _assert_same(got[g], exp)
        assert all(c["Taug"] == (0.0, 0.0, 0.0) for node in got[g] for c in node)
        # by the policy alone: a node past the gate whose eligible prefix holds n_candidates nodes returns that many
        for i in range(len(poses)):
            nex = _num_exclude_recent(poses, i)
            if i + 1 >= nex + 1 and max(i - 1 - nex, 0) >= 3:
                assert len(got[g][i]) == 3, (g, i)
    assert sum(len(node) for node in got[3]) > 300
    # host and device sweeps, host and device rows: the same bytes
    flat = api.sc_flatten_graphs(graphs)
    host = api.sc_detect_batch(flat=flat, raw_par=raw, records=True, **kw)
    flat["imgs"] = torch.from_numpy(flat["imgs"]).cuda()
    dev = api.sc_detect_batch(flat=flat, raw_par=raw, device_out=True, **kw)
    np.testing.assert_array_equal(dev[1].cpu().numpy(), host[1])
    assert dev[0].cpu().numpy().tobytes() == host[0].tobytes()
    assert api.sc_detect_batch(flat=flat, raw_par=raw, **kw) == got


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_graph_and_node_and_leave_the_rows_and_the_context_alone():
    import torch
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    ctx = api.default_context()
    lib = ctx._lib
    graphs = [_graphs()[g] for g in (1, 0, 3, 4)]                  # 1, 0, 3 and 9 nodes: graph 3 is the 9-node graph
    good = api.sc_detect_batch(graphs, records=True)
    assert good[1].sum() > 0
    flat = api.sc_flatten_graphs(graphs, [np.arange(len(p), dtype=np.int32) for _, p in graphs])
    p = api.sc_manager_params()
    keep = {k: np.ascontiguousarray(v) for k, v in flat.items()}
    nd = np.array([1, 0, 3, 9], np.int32)
    D = int(nd.sum())
    out = np.full((D, 3 * 64), 0xA5, np.uint8)
    n_out = np.full(D, -7, np.int32)
    b = L.ScBatch()
    b.n_graphs, b.mode, b.n_aggregate, b.n_detect = 4, L.SC_NODES_CLOUD, 1, nd.ctypes.data
    for name in ("node_off", "ids", "T", "Tinv", "xyzi", "point_off"):
        setattr(b, name, keep[name].ctypes.data)

    def call(o=out.ctypes.data, no=n_out.ctypes.data):
        rc = lib.cfear_sc_detect_batch(ctx.h, C.byref(p), C.byref(b), o, no)
        return rc, lib.cfear_last_error(ctx.h).decode()

    INV, CAP = L.ERR_INVALID_ARGUMENT, L.ERR_CAPACITY
    bad = []

    def with_(arr, idx, val, status, word):
        old = arr[idx]
        arr[idx] = val
        rc, msg = call()
        arr[idx] = old
        assert rc == status and word in msg, (rc, msg, word)
        bad.append(rc)

    with_(keep["ids"], 4 + 5, 3, INV, "graph 3, node 5")           # one bad node of graph 3: named
    with_(keep["point_off"], 4 + 6, 0, INV, "graph 3, node 5")
    with_(keep["node_off"], 2, 0, INV, "graph 1")
    with_(nd, 3, 10, INV, "graph 3: n_detect 10")
    with_(nd, 2, -1, INV, "graph 2: n_detect -1")
    b.mode = 7
    assert call()[0] == INV and "mode" in call()[1]
    b.mode = L.SC_NODES_CLOUD
    for name in ("node_off", "T", "Tinv", "point_off", "xyzi"):
        old = getattr(b, name)
        setattr(b, name, None)
        assert call()[0] == INV, name
        setattr(b, name, old)
    assert call(o=None)[0] == INV and call(no=None)[0] == INV
    dev_rows = torch.zeros(D * 3 * 64, dtype=torch.uint8, device="cuda")
    dev_cnt = torch.zeros(D, dtype=torch.int32, device="cuda")
    for o, no in ((dev_rows.data_ptr(), n_out.ctypes.data), (out.ctypes.data, dev_cnt.data_ptr())):
        rc, msg = call(o, no)
        assert rc == INV and "host or device" in msg               # mixed outputs
    # what cfear_sc_detect_sequence refuses: K > 64, the cell and LDS limits, bad ratios and manager parameters
    p.num_candidates_from_tree = 65
    assert call()[0] == CAP
    p.num_candidates_from_tree = 10
    for kw, status in [(dict(num_ring=41, num_sector=125), CAP), (dict(num_ring=2, num_sector=2560), CAP), (dict(num_ring=1, num_sector=5120), CAP),
                       (dict(num_ring=0), CAP), (dict(search_ratio=float("nan")), INV), (dict(search_ratio=float("inf")), INV)]:
        p.sc = api.sc_params(**kw)
        assert call()[0] == status, kw
    p.sc = api.sc_params()
    # what cfear_sc_raw_descriptors refuses: normalize, another interpolation, a 2 x 2 scale, an upscale, a sweep count
    sweeps = np.zeros((13, 240, 80), np.uint8)
    d, ptr, _k = api._image_desc(sweeps)
    raw = api.sc_raw_params(transpose=1)
    b.mode, b.imgs, b.desc, b.raw = L.SC_NODES_RAW, ptr, C.pointer(d), C.pointer(raw)
    assert call()[0] == INV and "2 x 2" in call()[1]
    small = np.zeros((13, 100, 30), np.uint8)
    d2, ptr2, _k2 = api._image_desc(small)
    b.imgs, b.desc = ptr2, C.pointer(d2)
    assert call()[0] == INV and "downscaled" in call()[1]
    ok_sweeps = np.zeros((13, 300, 100), np.uint8)
    d3, ptr3, _k3 = api._image_desc(ok_sweeps)
    b.imgs, b.desc = ptr3, C.pointer(d3)
    raw.normalize = 1
    assert call()[0] == INV and "normalize" in call()[1]
    raw.normalize, raw.interpolation = 0, 1
    assert call()[0] == INV and "INTER_AREA" in call()[1]
    raw.interpolation = L.SC_INTER_AREA
    d3.batch = 12
    assert call()[0] == INV and "12 sweeps for 13 nodes" in call()[1]
    d3.batch = 13
    # no refusal wrote a byte, here or on the device
    assert (out == 0xA5).all() and (n_out == -7).all() and not dev_rows.any() and not dev_cnt.any()
    # the raw batch is good now, and so is the cloud batch: the context is usable and the good call repeats its bytes
    assert call()[0] == L.OK and (n_out[:4] == 0).all()
    b.mode = L.SC_NODES_CLOUD
    assert call()[0] == L.OK
    np.testing.assert_array_equal(n_out, good[1])
    assert out.tobytes() == good[0].tobytes()
    again = api.sc_detect_batch(graphs, records=True)
    assert again[0].tobytes() == good[0].tobytes()
    # nothing to detect: CFEAR_OK, nothing written
    nd[:] = 0
    out[:] = 0xA5
    assert call()[0] == L.OK and call(o=None, no=None)[0] == L.OK and (out == 0xA5).all()
    b.n_graphs = 0
    assert call(o=None, no=None)[0] == L.OK


# ---- the demos -----------------------------------------------------------------------------------------------------------
def test_slam_batch_demo_finds_the_per_lap_candidates_and_loops():
    import slam_batch_demo as demo
    a = demo.run(2, per_lap_scan_context=True)
    b = demo.run(2)
    assert len(a["candidates"]) > 50 and a["candidates"] == b["candidates"]
    for la, lb in zip(a["loops"], b["loops"]):
        assert [(c["id_begin"], c["id_end"]) for c in la] == [(c["id_begin"], c["id_end"]) for c in lb]
    assert sum(len(l) for l in a["loops"]) > 0


def test_demo_batched_raw_scan_context_equals_the_raw_run():
    import loop_closure_demo as demo
    a = demo.run(demo.HipBackend(), raw_scan_context=True)
    b = demo.run(demo.HipBackend(), raw_scan_context=True, batched_scan_context=True)
    assert len(a["candidates"]) > 50
    assert [(c["from"], c["to"], c["sc_yaw"]) for c in a["candidates"]] == [(c["from"], c["to"], c["sc_yaw"]) for c in b["candidates"]]
    for ca, cb in zip(a["candidates"], b["candidates"]):
        assert abs(ca["sc_sim"] - cb["sc_sim"]) <= 1e-12
        np.testing.assert_array_equal(ca["t_be_guess"], cb["t_be_guess"])
    for ra, rb in zip(a["results"], b["results"]):
        assert ra["accepted"] == rb["accepted"] and ra["reg_ok"] == rb["reg_ok"]
        np.testing.assert_allclose(ra["t_be"], rb["t_be"], rtol=0, atol=1e-12)
        assert abs(ra["probability"] - rb["probability"]) <= 1e-9
