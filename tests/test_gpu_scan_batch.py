"""GPU: cfear_scan_create_batch -- N clouds, N scans, one call -- against cfear_scan_create on the same clouds.  The batch
runs the SAME surface-point kernels, so a served scan's cells and route word are compared bit for bit; what the batch adds
is plumbing: one arena, per-scan statuses, borrowed handles, staging, chunks.  Radius 3, factor 1, seeded clouds of
tests/surface_routes.py."""
import ctypes as C

import numpy as np
import pytest

from tests import surface_routes as R

pytestmark = pytest.mark.gpu

MAX_CELLS = 1200
EMPTY, OVER, BIG = 1, 2, 3            # the indices of the empty cloud, the one beyond MAX_CELLS cells, the one beyond 16 384 points
_CACHE = {}


def _moved(c, x, y, t):
    out = c.copy()
    out[:, 0] = np.float32(x) + np.cos(t) * c[:, 0] - np.sin(t) * c[:, 1]
    out[:, 1] = np.float32(y) + np.sin(t) * c[:, 0] + np.cos(t) * c[:, 1]
    return out


def _clouds():
    """Six clouds of different sizes: cells 804 | empty | several thousand cells (> MAX_CELLS) | 16 385 points, 975 cells
    (the 64-points-per-thread instantiation) | 557 points | the first 2 711 points of cloud 0, moved a little (a
    registration partner)."""
    if "clouds" not in _CACHE:
        a = R.uniform(1, 3000, 120)
        _CACHE["clouds"] = [a, np.zeros((0, 4), np.float32), R.uniform(23, 8000, 220), R.walls(6, 16385, 240), R.uniform(21, 557, 60),
                            _moved(a[:2711], 0.3, -0.1, 0.01)]
    return _CACHE["clouds"]


def _mots():
    return np.array([[1.5, -0.2, 0.05], [0, 0, 0], [0.4, 0.1, -0.02], [-1.0, 0.3, 0.03], [0.2, 0.2, 0.2], [2.0, 0.0, -0.04]])


def _single(i, comp):
    """cfear_scan_create on cloud i (on the device, compensated in place when comp): the MapPointNormal, its route word, its
    cells; made once."""
    import torch
    from tbv_slam_public_amd import api
    key = ("single", i, comp)
    if key not in _CACHE:
        t = torch.from_numpy(_clouds()[i].copy()).cuda()
        m = api.MapPointNormal(t, 3.0, (0.0, 0.0), True, compensate=tuple(_mots()[i]) if comp else None, ccw=False)
        _CACHE[key] = (m, m.path, m.GetCells())
    return _CACHE[key]


def _batch(comp, device, **kw):
    import torch
    from tbv_slam_public_amd import api
    clouds = [c.copy() for c in _clouds()]
    if device:
        clouds = [torch.from_numpy(c).cuda() for c in clouds]
    b = api.scan_create_batch(clouds, 3.0, (0.0, 0.0), True, compensate=_mots() if comp else None, max_cells=MAX_CELLS, **kw)
    return b, clouds


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("comp", [False, True], ids=["plain", "compensated"])
def test_batch_equals_single_scans(comp, device):
    from tbv_slam_public_amd import _lib as L
    b, clouds = _batch(comp, device)
    assert len(b) == 6
    want = [L.OK] * 6
    want[EMPTY], want[OVER] = L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY
    assert list(b.status) == want
    assert b[EMPTY] is None and b[OVER] is None
    for i in range(6):
        if i in (EMPTY, OVER):
            continue
        _, path, cells = _single(i, comp)
        assert b[i].GetSize() == len(cells) > 0
        assert b[i].path == path, (i, R.describe(b[i].path), R.describe(path))
        assert b[i].GetCells().tobytes() == cells.tobytes(), i
        after = clouds[i].cpu().numpy() if device else clouds[i]
        assert after.tobytes() == _clouds()[i].tobytes()                  # the caller's points stay as they are
    assert b[BIG].path & R.K64 and not b[0].path & R.K64                  # the two instantiations ran side by side in one launch
    # the cloud that failed really holds more cells than the slab: cfear_scan_create serves it
    assert _single(OVER, comp)[0].GetSize() > MAX_CELLS
    b.close()


def test_scattered_clouds_in_place():
    """The (xyzi, offsets, lengths) form with the clouds out of order and far apart in one buffer: the staging goes cloud
    by cloud instead of in one piece (host, compensated), and a device buffer without compensation is used in place."""
    import torch
    from tbv_slam_public_amd import api
    cl = _clouds()
    order = [5, 4, 0]
    gap = 40000
    lengths = np.array([len(cl[i]) for i in order], np.int32)
    offsets = np.array([2 * gap, gap, 0], np.int64)
    buf = np.zeros((2 * gap + len(cl[5]), 4), np.float32)
    for o, i in zip(offsets, order):
        buf[o:o + len(cl[i])] = cl[i]
    b = api.scan_create_batch((buf, offsets, lengths), 3.0, (0.0, 0.0), True, compensate=_mots()[order], max_cells=MAX_CELLS)
    for k, i in enumerate(order):
        assert b[k].path == _single(i, True)[1] and b[k].GetCells().tobytes() == _single(i, True)[2].tobytes(), i
    d = api.scan_create_batch((torch.from_numpy(buf).cuda(), offsets, lengths), 3.0, (0.0, 0.0), True, max_cells=MAX_CELLS)
    for k, i in enumerate(order):
        assert d[k].path == _single(i, False)[1] and d[k].GetCells().tobytes() == _single(i, False)[2].tobytes(), i


def test_register_batch_mixes_borrowed_and_own_handles():
    """One cfear_register_batch whose jobs name borrowed and individually created handles side by side gives the records
    of the all-individual batch, bit for bit; so does a candidate batch over a scan table of borrowed handles."""
    from tbv_slam_public_amd import api
    b, _ = _batch(False, True)
    own = {i: _single(i, False)[0] for i in (0, 4, 5)}
    reg = api.n_scan_normal_reg("P2L")
    poses2, poses3 = np.zeros((2, 3)), np.zeros((3, 3))
    ref = reg.RegisterBatch([([own[0], own[5]], poses2), ([own[5], own[0]], poses2), ([own[0], own[4], own[5]], poses3)])
    mix = reg.RegisterBatch([([b[0], own[5]], poses2), ([own[5], b[0]], poses2), ([own[0], b[4], b[5]], poses3)])
    bor = reg.RegisterBatch([([b[0], b[5]], poses2), ([b[5], b[0]], poses2), ([b[0], b[4], b[5]], poses3)])
    assert ref["status"][0] == 0 and ref["num_residuals"][0] > 100          # the partner cloud registers: the jobs are not empty
    assert abs(ref["pose"][0][0] + 0.3) < 0.05 and abs(ref["pose"][0][2] + 0.01) < 0.005
    assert mix.tobytes() == ref.tobytes() and bor.tobytes() == ref.tobytes()
    cands = api.ScanTable.candidates([0], [1], np.zeros((1, 3)))
    t_own, t_bor = api.ScanTable([own[0], own[5]]), api.ScanTable([b[0], b[5]])
    assert reg.RegisterCandidates(t_bor, cands).tobytes() == reg.RegisterCandidates(t_own, cands).tobytes()
    q = np.array([[10.0, 10.0], [60.0, 60.0]])
    assert np.array_equal(b[0].GetClosestIdx(q, 5.0), own[0].GetClosestIdx(q, 5.0))
    lo, hi, cnt = b[0].GetClosestTies(q, 5.0)
    assert np.array_equal(lo, own[0].GetClosestTies(q, 5.0)[0])


def test_borrowed_handles_are_not_destroyed_one_by_one():
    """cfear_scan_destroy on a borrowed handle is refused and frees nothing; a scan table keeps the arena alive beyond the
    batch; create, destroy, create serves the same bits again (the context has no allocation counter to read)."""
    from tbv_slam_public_amd import _lib as L, api
    ctx = api.default_context()
    b, _ = _batch(False, False)
    h = b[0]._h
    assert ctx._lib.cfear_scan_destroy(h) == L.ERR_INVALID_ARGUMENT
    assert b"borrowed" in ctx._lib.cfear_last_error(ctx.h)
    assert ctx._lib.cfear_scan_destroy(h) == L.ERR_INVALID_ARGUMENT         # again: still refused, still alive
    assert b[0].GetCells().tobytes() == _single(0, False)[2].tobytes()
    table = api.ScanTable([b[0], b[5]])
    assert ctx._lib.cfear_scan_destroy(h) == L.ERR_INVALID_ARGUMENT         # a table names it now: still not the caller's to destroy
    reg = api.n_scan_normal_reg("P2L")
    cands = api.ScanTable.candidates([0], [1], np.zeros((1, 3)))
    before = reg.RegisterCandidates(table, cands)
    b.close()                                                               # the table's views stay valid: it holds references
    assert reg.RegisterCandidates(table, cands).tobytes() == before.tobytes()
    table.close()
    for _ in range(2):
        b2, _ = _batch(False, False)
        assert b2[0].GetCells().tobytes() == _single(0, False)[2].tobytes()
        b2.close()
    s = C.c_void_p()
    b3, _ = _batch(False, False)
    assert ctx._lib.cfear_scan_batch_get(b3._h, 6, C.byref(s)) == L.ERR_INVALID_ARGUMENT
    assert ctx._lib.cfear_scan_batch_get(b3._h, -1, C.byref(s)) == L.ERR_INVALID_ARGUMENT


def test_refusals():
    from tbv_slam_public_amd import _lib as L, api
    cl = _clouds()
    with pytest.raises(L.CfearError) as e:
        api.scan_create_batch([cl[0]], max_cells=0)
    assert e.value.status == L.ERR_INVALID_ARGUMENT
    with pytest.raises(L.CfearError):
        api.scan_create_batch([cl[0]], max_cells=16385)
    with pytest.raises(L.CfearError) as e:
        api.scan_create_batch((cl[0], np.array([0, -4], np.int64), np.array([10, 10], np.int32)), max_cells=100)
    assert "scan 1" in str(e.value)
    with pytest.raises(L.CfearError):
        api.scan_create_batch([], max_cells=100)
    only_failures = api.scan_create_batch([cl[EMPTY], cl[EMPTY]], max_cells=100)     # served: two statuses, no handle
    assert list(only_failures.status) == [L.ERR_EMPTY_CLOUD] * 2 and only_failures[0] is None


def test_more_scans_than_one_launch_holds():
    """520 small clouds: their surface scratch (2.1 MiB per scan) exceeds what one launch sequence may take, so the batch runs
    as two; every scan equals cfear_scan_create on its cloud.  A context of its own, so that the scratch goes with it."""
    from tbv_slam_public_amd import api
    ctx = api.Context(0)
    try:
        protos = [R.uniform(30 + k, 150 + 37 * k, 30) for k in range(5)]
        singles = []
        for p in protos:
            m = api.MapPointNormal(p.copy(), 3.0, (0.0, 0.0), True, ctx=ctx)
            singles.append((m.path, m.GetCells().tobytes()))
            m.close()
        n = 520
        b = api.scan_create_batch([protos[i % 5] for i in range(n)], 3.0, (0.0, 0.0), True, max_cells=128, ctx=ctx)
        assert len(b) == n and not b.status.any()
        for i in list(range(0, n, 37)) + [n - 6, n - 5, n - 4, n - 3, n - 2, n - 1]:
            assert (b[i].path, b[i].GetCells().tobytes()) == singles[i % 5], i
        b.close()
    finally:
        ctx.close()
