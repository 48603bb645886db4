"""GPU: the surface-point kernels on every route they can take.  The thresholds between the routes are LDS arithmetic inside
surface.hip, so every case asserts the route word the kernels report (cfear_scan_surface_path, MapPointNormal.path) against
tests/surface_routes.predict -- which only guards the branch -- and the cells against the CPU oracle, with the tolerances
of tests/test_gpu_surface.py.  Radius 3, factor 1, integer intensities in 61..255 and seeded clouds unless stated."""
import numpy as np
import pytest

from tests import surface_routes as R

pytestmark = pytest.mark.gpu

MOT = (1.5, -0.2, 0.05)


def _clusters(seed, n, side, per=40, x0=0.0, y0=0.0):
    """n points in clusters of `per` (sigma 1 m) at uniform centres of a side x side box: cells even in a sparse grid."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(2, side - 2, ((n + per - 1) // per, 2))[np.arange(n) // per]
    xy = np.clip(c + rng.normal(0, 1.0, (n, 2)), 0, side)
    return R._cloud(x0 + xy[:, 0], y0 + xy[:, 1], rng)


def _with(cloud, **intensity):
    c = cloud.copy()
    for k, v in intensity.items():
        c[int(k[1:]), 3] = v
    return c


def _float_weights(cloud):
    c = cloud.copy()
    c[:, 3] = np.random.default_rng(77).uniform(50, 200, len(c))
    return c


def _tier(count):
    return np.concatenate([R.blob(20 + count, count, 0.0, 0.0), R.blob(19, 4, 30.0, 30.0)])


# ---- 1. the route matrix: name -> (cloud builder, factor, rotation of a compensation, features the case is there for) ------
# Final shapes: each is the smallest round size that crosses its threshold by the kernel's arithmetic (surface_routes.predict).
MATRIX = {
    "one_slab": (lambda: R.uniform(1, 3000, 120), 1.0, None, ("fast", "one_slab", "wbyte", "k32")),
    "slabs_bytes": (lambda: R.walls(2, 12000, 240), 1.0, None, ("slabs",)),                       # 9 n > staging area
    "slabs_voxels": (lambda: np.concatenate([R.uniform(3, 4000, 300), _clusters(4, 1000, 300)]), 1.0, None, ("slabs",)),   # V > 2048
    "float_weights": (lambda: _float_weights(R.uniform(1, 3000, 120)), 1.0, None, ("wfloat",)),
    "weight_400": (lambda: _with(R.uniform(1, 3000, 120), i7=400.0), 1.0, None, ("wfloat",)),
    "weight_below_60": (lambda: _with(R.uniform(1, 3000, 120), i7=30.0), 1.0, None, ("wbyte",)),   # clamps to 0: still a byte
    "second_read": (lambda: _clusters(5, 3000, 800), 1.0, None, ("read2",)),                         # 267 x 267 cells
    "k64_lower_edge": (lambda: R.walls(6, 16385, 240), 1.0, None, ("k64",)),
    "k64_upper_edge": (lambda: R.walls(7, 32768, 240), 1.0, None, ("k64",)),
    "k32_upper_edge": (lambda: R.walls(8, 16384, 240), 1.0, None, ("k32",)),
    "tier_5": (lambda: _tier(5), 1.0, None, ("fast",)),
    "tier_6": (lambda: _tier(6), 1.0, None, ("tier1",)),
    "tier_16": (lambda: _tier(16), 1.0, None, ("tier1",)),
    "tier_17": (lambda: _tier(17), 1.0, None, ("tier4",)),
    "tier_64": (lambda: _tier(64), 1.0, None, ("tier4",)),
    "tier_65": (lambda: _tier(65), 1.0, None, ("tier16",)),
    "top_bucket": (lambda: np.concatenate([R.blob(9, 6000, 30.0, 30.0, 1.2), R.uniform(10, 500, 60)]), 1.0, None, ("top_bucket",)),
    "scratch_centroids": (lambda: R.walls(11, 14000, 150), 1.0, None, ("cen_scratch", "slabs")),
    "handover_cells": (lambda: _clusters(12, 3000, 1600), 1.0, None, ("single", "reason_cells", "prepared")),         # 534 x 534 cells
    "handover_order": (lambda: _clusters(13, 16384, 1500), 1.0, None, ("single", "reason_order", "prepared")),
    "handover_rows3": (lambda: R.uniform(14, 16000, 1500, 8.9), 1.0, None, ("single", "reason_rows3", "prepared")),
    "handover_reach_2": (lambda: R.uniform(1, 3000, 120), 2.0, None, ("single", "reason_reach", "unprepared")),
    "handover_reach_1_5": (lambda: R.uniform(1, 3000, 120), 1.5, None, ("single", "reason_reach", "unprepared")),
    "handover_rotation": (lambda: R.uniform(15, 3000, 120, x0=-60, y0=-60), 1.0, 3e5, ("single", "reason_rotation", "unprepared")),
    "global_memory": (lambda: R.walls(16, 32769, 240), 1.0, None, ("global", "reason_points", "unprepared")),
}
_RESULTS = {}


def _scan(cloud, factor=1.0, compensate=None, radius=3.0):
    """-> (route word, cells, the cloud as the device left it)."""
    import torch
    from tbv_slam_public_amd import api
    old = api.MapPointNormal.downsample_factor
    api.MapPointNormal.downsample_factor = factor
    try:
        t = torch.from_numpy(np.ascontiguousarray(cloud)).cuda()
        m = api.MapPointNormal(t, radius, (0.0, 0.0), True, compensate=compensate, ccw=False)
        return m.path, m.GetCells(), t.cpu().numpy()
    finally:
        api.MapPointNormal.downsample_factor = old


def _run(name):
    """One matrix case, run once: (route word, predicted word, cells, oracle cells)."""
    if name not in _RESULTS:
        from oracle import pyoracle as O
        build, factor, rot, _ = MATRIX[name]
        cloud = build()
        path, got, dev = _scan(cloud, factor, None if rot is None else (MOT[0], MOT[1], rot))
        _RESULTS[name] = (path, R.predict(dev, 3.0, factor, rot), got, O.surface_points(dev, 3.0, factor, (0, 0), True))
    return _RESULTS[name]


@pytest.mark.parametrize("name", sorted(MATRIX))
def test_route_matrix(name):
    path, want, got, exp = _run(name)
    print(name, "n =", len(MATRIX[name][0]()), R.describe(path), "cells", exp.shape[0])
    assert path == want, (R.describe(path), R.describe(want))
    for f in MATRIX[name][3]:
        assert R.FEATURES[f](path), (f, R.describe(path))               # the case sits on the branch it is there for
    if name != "tier_5":
        assert exp.shape[0] >= 1
    R.cmp_cells(got, exp)
    if name == "tier_64":
        assert not path & R.TIER16                                      # C = 64 is the 4-lane tier's last count
    if name == "tier_16":
        assert not path & R.TIER4


def test_route_matrix_covers_every_route_bit():
    seen = {f for name in MATRIX for f, hit in R.FEATURES.items() if hit(_run(name)[0])}
    print("seen:", sorted(seen))
    assert seen >= set(R.FEATURES) - {"rows"}, sorted(set(R.FEATURES) - seen)      # (rows mode: the odometry tests below)


# ---- 2. the order of the points inside a voxel -----------------------------------------------------------------------------
ORDER_PADS = {
    "one_slab": (lambda: None, ("fast", "one_slab")),
    "slabs": (lambda: R.walls(30, 12000, 240, x0=700.0), ("fast", "slabs")),
    "k64": (lambda: R.walls(31, 16000, 240, x0=700.0), ("k64",)),
    "single": (lambda: R.blob(32, 20, -700.0, 1500.0), ("single",)),
    "global": (lambda: R.walls(33, 32000, 240, x0=700.0), ("global",)),
}


@pytest.mark.parametrize("route", sorted(ORDER_PADS))
def test_in_voxel_order_decides_cells(route):
    """The float voxel centroid is a sequential sum in input order; only candidates within an ulp of the radius see its
    last bit.  order_blocks() holds such candidates (and asserts that the reversed cloud gives other cells), so a rank
    pass that returned another permutation of a voxel's points fails here."""
    from oracle import pyoracle as O
    pad, feats = ORDER_PADS[route]
    cloud = R.order_blocks(40, pad())
    path, got, _ = _scan(cloud)
    assert path == R.predict(cloud), (R.describe(path), R.describe(R.predict(cloud)))
    for f in feats:
        assert R.FEATURES[f](path), (f, R.describe(path))
    R.cmp_cells(got, O.surface_points(cloud, 3.0, 1.0, (0, 0), True))


def test_rank_pass_every_run_length_at_every_offset():
    from oracle import pyoracle as O
    cloud = R.run_lengths(41)
    path, got, _ = _scan(cloud)
    assert path == R.predict(cloud) and path & R.KIND_MASK == R.FAST
    R.cmp_cells(got, O.surface_points(cloud, 3.0, 1.0, (0, 0), True))


# ---- 3. grid edges ---------------------------------------------------------------------------------------------------------
def _lattice():
    g = (np.arange(-20, 21) * 0.75).astype(np.float32)                  # every fourth value is k * 3.0f, k = -5 .. 5: the bounding
    x, y = np.meshgrid(g, g)                                            # box minimum itself lies on a voxel boundary
    return R._cloud(x.ravel(), y.ravel(), np.random.default_rng(50))


def _voxel_block(seed, nvox):
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(nvox), 8)
    return R._cloud(3.0 * (i % 16) + rng.uniform(0.1, 2.9, len(i)), 3.0 * (i // 16) + rng.uniform(0.1, 2.9, len(i)), rng)


EDGES = {
    "on_voxel_boundaries": _lattice,
    "all_negative": lambda: R.uniform(51, 3000, 120, x0=-500.0, y0=-300.0),
    "one_grid_row": lambda: R.uniform(52, 2000, 600, 2.5, y0=0.2),
    "one_grid_column": lambda: R.uniform(53, 2000, 2.5, 600, x0=0.2),
    "4096_grid_rows": lambda: np.concatenate([R.blob(54, 200, 0.0, 0.0), R.blob(55, 200, 0.0, 3.0 * 4095)]),
    "V_256": lambda: _voxel_block(56, 256),                             # the finish kernel's rounds of 256 voxels
    "V_257": lambda: _voxel_block(57, 257),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_grid_edges(name):
    from oracle import pyoracle as O
    cloud = EDGES[name]()
    L = R.layout(cloud)
    assert {"one_grid_row": L["dby"] == 1, "one_grid_column": L["dbx"] == 1, "4096_grid_rows": L["dby"] == 4096,
            "V_256": L["V"] == 256, "V_257": L["V"] == 257}.get(name, True), (L["dbx"], L["dby"], L["V"])
    path, got, _ = _scan(cloud)
    assert path == R.predict(cloud), (R.describe(path), R.describe(R.predict(cloud)))
    exp = O.surface_points(cloud, 3.0, 1.0, (0, 0), True)
    assert exp.shape[0] >= 2
    R.cmp_cells(got, exp)


def test_4097_grid_rows_are_refused():
    from tbv_slam_public_amd import _lib as L
    cloud = np.concatenate([R.blob(54, 200, 0.0, 0.0), R.blob(55, 200, 0.0, 3.0 * 4096)])
    assert R.layout(cloud)["dby"] == 4097 and R.predict(cloud) is None
    with pytest.raises(L.CfearError) as e:
        _scan(cloud)
    assert e.value.status == L.ERR_CAPACITY


# ---- 4. motion compensation x hand-over ------------------------------------------------------------------------------------
COMPENSATED = {
    "fast": (lambda: R.uniform(60, 3000, 120, x0=-60.0, y0=-60.0), 1.0, ("fast",)),
    "prepared_handover": (lambda: _clusters(61, 3000, 1600, x0=-800.0, y0=-800.0), 1.0, ("single", "prepared", "reason_cells")),
    "unprepared_handover": (lambda: R.uniform(62, 3000, 120, x0=-60.0, y0=-60.0), 2.0, ("single", "unprepared", "reason_reach")),
    "global_memory": (lambda: R.walls(63, 32769, 240, x0=-120.0, y0=-120.0), 1.0, ("global", "unprepared")),
}


@pytest.mark.parametrize("name", sorted(COMPENSATED))
def test_compensation_happens_once_on_every_route(name):
    """The `prepared` flag of a hand-over decides whether the single-kernel path compensates again: the cloud left in
    place must be the oracle's compensated cloud (the ulp allowance of test_compensate_matches_oracle) and the cells the
    oracle's cells of that cloud; a second compensation would show as metres."""
    from oracle import pyoracle as O
    build, factor, feats = COMPENSATED[name]
    cloud = build()
    path, got, dev = _scan(cloud, factor, MOT)
    assert path == R.predict(dev, 3.0, factor, MOT[2]), (R.describe(path), R.describe(R.predict(dev, 3.0, factor, MOT[2])))
    for f in feats:
        assert R.FEATURES[f](path), (f, R.describe(path))
    exp_cloud = O.compensate(cloud, MOT, False)
    d = np.abs(dev[:, :2] - exp_cloud[:, :2])
    assert d.max() <= 2e-5 and (d > 0).mean() < 1e-3, (d.max(), (d > 0).mean())
    np.testing.assert_array_equal(dev[:, 2:], exp_cloud[:, 2:])
    exp = O.surface_points(dev, 3.0, factor, (0, 0), True)
    assert exp.shape[0] >= 20
    R.cmp_cells(got, exp)


# ---- 5. batches and rows mode through the odometry ---------------------------------------------------------------------------
BATCH = ("one_slab", "handover_cells", "handover_order", "handover_rows3", "k64_lower_edge", "global_memory", None, "slabs_bytes")


def test_batch_of_mixed_routes_through_process_clouds():
    """Eight streams in one launch sequence, created with CA-CFAR parameters (65 536 points per stream: the mixed sort kernel):
    three hand-overs of different reasons side by side in the work list, a 64-points-per-thread scan, a global-memory scan
    and an empty cloud.  Every stream's cells and route word equal the single-scan result and the oracle; a second call
    with the routes permuted across the streams shows that the work list resets and the scratch is reused."""
    from tbv_slam_public_amd import api, _lib as L
    par = api.odometry_params(filter_type=1, compensate=0)
    od = api.OdometryKeyframeFuser(len(BATCH), 400, 3360, par)
    empty = np.zeros((0, 4), np.float32)
    for shift in (0, 3):
        names = BATCH[shift:] + BATCH[:shift]
        info = od.process_clouds([empty if nm is None else MATRIX[nm][0]() for nm in names])
        for b, nm in enumerate(names):
            if nm is None:
                assert info["reg_status"][b] == L.ERR_EMPTY_CLOUD and info["n_cells"][b] == 0
                continue
            path, want, single, exp = _run(nm)
            assert info["reg_status"][b] not in (L.ERR_EMPTY_CLOUD, L.ERR_CAPACITY) and info["n_cells"][b] == exp.shape[0], (shift, nm)
            scan = od.node(b)["scan"]
            assert scan.path == path == want, (shift, nm, R.describe(scan.path), R.describe(want))
            got = scan.GetCells()
            R.cmp_cells(got, exp)
            for field in got.dtype.names:
                np.testing.assert_array_equal(got[field], single[field], err_msg="%s %s" % (nm, field))
    od.close()


@pytest.mark.parametrize("factor", [1.0, 2.0])
def test_rows_mode_cells_and_route_word(factor):
    """Rows mode (the fused filter hands surface_prep_kernel<true> per-row key lists): two frames of a 400 x 3360 synthetic
    sweep -- the size every odometry test uses -- through process(), k-strongest preset, on the fast pipeline and with a
    downsample factor that leaves it.  The cells equal the oracle's cells of the cloud the stage left behind."""
    import torch
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api, synth
    imgs = [synth.scene_v1(sd, 2)[0] for sd in (70, 71)]
    od = api.OdometryKeyframeFuser(2, 400, 3360, api.odometry_params(downsample_factor=factor))
    for f in range(2):
        info = od.process(torch.from_numpy(np.stack([s[f] for s in imgs])).cuda())
        for b in range(2):
            node = od.node(b)
            exp = O.surface_points(node["cloud"], 3.0, factor, (0, 0), True)
            path = node["scan"].path
            want = R.predict(node["cloud"], 3.0, factor, rows=True)
            assert path == want and path & R.ROWS, (R.describe(path), R.describe(want))
            assert path & R.KIND_MASK == (R.FAST if factor == 1.0 else R.SINGLE)
            assert info["n_cells"][b] == exp.shape[0] > 50
            R.cmp_cells(node["scan"].GetCells(), exp)
    od.close()
