"""GPU: coral_kernel against the CPU oracle on every sort, storage and lookup path it can take, on the neighbourhood edges
the reference defines, over radii 0.25 .. 8, in uneven and split batches, and at its refusals (tests/coral_geometry.py
holds the inputs).  The kernel reports the path that served a job in cfear_coral_result.pad (CFEAR_CORAL_PATH_*); every
path test asserts those bits, so a moved threshold cannot silently move a test onto another branch.  Comparisons are
tests/test_gpu_coral.py::_check's: integer outcomes identical, per-point entropies to 1e-6 (above radius 1:
coral_geometry.per_point_atol), aggregates to rtol 1e-8."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import coral_geometry as G                       # noqa: E402
from tests.test_gpu_coral import _check                     # noqa: E402
from tests.test_oracle_coral import _peaks, _rel            # noqa: E402

Z = np.zeros(3)


@pytest.fixture(scope="module")
def matrix():
    return G.matrix_jobs()


def _raw_batch(jobs, radius=1.0, want_per_point=False):
    """cfear_coral_quality_batch without api.coral_quality_batch's exception: (return code, records, per-point)."""
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.default_context()
    n = len(jobs)
    arr, keep, sizes = (L.CoralJob * n)(), [], []
    for i, (rc_, rp, sc, sp, off) in enumerate(jobs):
        pr, nr, kr = api._cloud_ptr(rc_)
        ps, ns, ks = api._cloud_ptr(sc)
        keep += [kr, ks]
        arr[i].ref_xyzi, arr[i].src_xyzi, arr[i].n_ref, arr[i].n_src = pr, ps, nr, ns
        for k in range(3):
            arr[i].ref_pose[k], arr[i].src_pose[k], arr[i].offset[k] = float(rp[k]), float(sp[k]), float(off[k])
        sizes.append(nr + ns)
    par = L.CoralParams()
    ctx._lib.cfear_coral_params_default(C.byref(par))
    par.radius = float(radius)
    out = np.full(n, -77, L.CORAL_RESULT_DTYPE)
    pp = np.zeros((sum(sizes), 3), np.float64) if want_per_point else None
    rc = ctx._lib.cfear_coral_quality_batch(ctx.h, arr, n, C.byref(par), out.ctypes.data, pp.ctypes.data if want_per_point else None)
    return rc, out, pp


def _assert_record(r, ref, src, rp, sp, off=(0, 0, 0), radius=1.0):
    from oracle import pyoracle as O
    ok, eq, pp = O.coral_quality(ref, src, rp, sp, off, radius)
    assert r["status"] == 0
    np.testing.assert_allclose([r["joint"], r["sep"], r["overlap"]], eq, rtol=1e-8, atol=1e-12)
    assert bool(r["valid"]) == ok and r["count_valid"] == int(pp[:, 2].sum())
    return pp


# ---- a. the path matrix -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lds_bitmap_rows", "lds_bitmap_radix", "lds_bsearch_rows", "lds_bsearch_radix",
                                  "lds_bsearch_bitonic", "scratch_bitmap_rows", "scratch_bitmap_radix",
                                  "scratch_bitmap_bitonic_16384", "scratch_bsearch_rows", "scratch_bsearch_radix",
                                  "scratch_bsearch_bitonic", "lds_edge", "scratch_edge", "radix_all_ones_key"])
def test_path_matrix(matrix, name):
    """Every {LDS, scratch} x {bitmap, binary search} combination with every sort that can occur with it, per point.  The
    large grids come from a small far cluster of both clouds, whose points are valid too.  `radix_all_ones_key` fails
    without the padding test by position in grid_sort_block: its last point has the key the padding has."""
    ref, src, want = matrix[name]
    q = _check(ref, src, Z, Z, (0, 0, 0))
    assert q.path == want, "%s ran on %s" % (name, G.describe(q.path))
    assert q.GetQualityMeasure()[2] > 0.3 and q.count_valid >= 100
    far = np.concatenate([src[:, 0] > 1000, ref[:, 0] > 1000])
    if far.any():
        assert q.per_point[far, 2].sum() >= 4               # the far cluster contributes valid points


def test_path_matrix_covers_every_combination(matrix):
    bits = {w for _, _, w in matrix.values()}
    assert {b & 3 for b in bits} == {0, 1, 2, 3} and {b >> 2 for b in bits} == {0, 1, 2}


# ---- b. radius sweep ------------------------------------------------------------------------------------------------------------
def _wall_pair():
    ref = np.concatenate([G.wall(30, 900, -60, 60, 0.0), G.wall(31, 300, -60, 60, 7.0)])
    src = np.concatenate([G.wall(32, 800, -60, 60, 0.1), G.wall(33, 200, -60, 60, 7.1)])
    return ref, src


@pytest.mark.parametrize("radius", [0.25, 0.6, 1.0, 2.5, 5.0, 8.0])
def test_radius_sweep_scene_and_wall_at_5_km(radius):
    """World poses at +-5 km (float coordinates with a 5e-4 m ulp; the reference rounds the same way), weighting on and
    off.  A weighted per-point value is intensity x entropy, so above radius 1 its tolerance carries the largest
    intensity (255); up to radius 1 it stays at the 1e-6 of tests/test_gpu_coral.py."""
    clouds, gt = _peaks(10, [0, 1])
    far = np.array([5000.0, -5000.0, 0.0])
    wr, ws = _wall_pair()
    atol = G.per_point_atol(radius)
    paths = set()
    for weight in (False, True):
        a = atol if (radius <= 1.0 or not weight) else atol * 255.0
        q = _check(clouds[0], clouds[1], gt[0] + far, gt[1] + far, (0.2, -0.1, 0.01), radius, weight, atol=a)
        paths.add(q.path)
        q = _check(wr, ws, -far, np.array([0.2, 0.05, 0.003]) - far, (0, 0, 0), radius, weight, atol=a)
        paths.add(q.path)
        assert q.count_valid >= 100
    print("radius %g: paths %s" % (radius, sorted(G.describe(p) for p in paths)))


# ---- c. neighbourhood edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.edge_cases()))
def test_neighbourhood_edges(name):
    """Hand-placed dyadic lattices (tests/test_oracle_coral.py checks them on the CPU): against the oracle and against the
    exact restatement.  `d2 <= r2` in place of `d2 < r2` fails at_radius_* (count_valid 0 -> 2) and the lattices."""
    ref, src = G.edge_cases()[name]
    q = _check(ref, src, Z, Z, (0, 0, 0))
    e = G.exact_coral(ref, src, Z, Z)
    assert not e["marginal"].any()
    np.testing.assert_array_equal(q.per_point[:, 2].astype(bool), e["valid"])
    v = e["valid"]
    np.testing.assert_allclose(q.per_point[v, 0], e["joint"][v], rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(q.per_point[v, 1], e["sep"][v], rtol=1e-9, atol=1e-6)
    np.testing.assert_allclose(q.GetQualityMeasure(), e["quality"], rtol=1e-8, atol=1e-12)
    assert q.path == G.path_bits(0, 0, G.SORT_ROWS)
    if name.startswith("at_radius"):
        assert q.count_valid == 0
    if name.startswith("inside_radius"):
        assert q.count_valid == 2
    if name == "duplicates":
        np.testing.assert_allclose(q.per_point[:, :2], 0.5 * np.log(1e-8), rtol=1e-14)


# ---- d. batches -------------------------------------------------------------------------------------------------------------------
def _uneven_jobs(matrix):
    e = G.edge_cases()
    clouds, gt = _peaks(11, [0, 1])
    js = [(*e["own_2_and_3"], Z), (*matrix["scratch_bsearch_rows"][:2], Z), (clouds[0], clouds[1], _rel(gt[0], gt[1])),
          (*e["single_source_point"], Z), (*matrix["lds_bsearch_radix"][:2], Z), (*e["lattice_borders"], Z)]
    return [(ref, Z, src, sp, (0.0, 0.0, 0.0)) for ref, src, sp in js]


def test_batch_of_uneven_jobs_per_point_and_order(matrix):
    """Jobs from 9 to 8040 points in one call with per-point output (rows padded to the largest job on the device,
    compacted on the host); the same jobs in another order give bit-identical records and rows."""
    from tbv_slam_public_amd import api
    jobs = _uneven_jobs(matrix)
    out, pps = api.coral_quality_batch(jobs, want_per_point=True)
    for (ref, rp, src, sp, off), r, pp in zip(jobs, out, pps):
        exp = _assert_record(r, ref, src, rp, sp, off)
        assert pp.shape == exp.shape
        np.testing.assert_array_equal(pp[:, 2], exp[:, 2])
        v = exp[:, 2] > 0
        np.testing.assert_allclose(pp[v, :2], exp[v, :2], rtol=1e-9, atol=1e-6)
        np.testing.assert_array_equal(pp[~v, :2], 100.0)
    assert out["pad"][1] == matrix["scratch_bsearch_rows"][2] and out["pad"][4] == matrix["lds_bsearch_radix"][2]
    order = [3, 1, 5, 0, 4, 2]
    out2, pps2 = api.coral_quality_batch([jobs[i] for i in order], want_per_point=True)
    for k, i in enumerate(order):
        assert out2[k].tobytes() == out[i].tobytes()
        np.testing.assert_array_equal(pps2[k], pps[i])


def test_batch_split_into_several_launches(matrix):
    """One 16 384-point job and enough small ones that the per-job scratch exceeds the 1 GiB a launch may use: the batch
    runs as two launches over one scratch.  Records and per-point rows on both sides of the split and of the last job
    against the oracle; equal jobs give equal bytes wherever they ran."""
    from tbv_slam_public_amd import api
    big_ref, big_src, big_bits = matrix["scratch_bitmap_bitonic_16384"]
    stride = G.scratch_bytes(G.MAX_POINTS)
    per_launch = (1 << 30) // stride
    n_jobs = per_launch + 40
    assert n_jobs * stride > (1 << 30) and per_launch * stride <= (1 << 30)
    sr, ss = G.cluster_pair(40, 160, 150, (0, 9, 0, 9))
    offs = [(0.05 * k, -0.03 * k, 0.002 * k) for k in range(8)]
    jobs = [(big_ref, Z, big_src, Z, (0.0, 0.0, 0.0))] + [(sr, Z, ss, Z, offs[(j - 1) % 8]) for j in range(1, n_jobs)]
    out, pps = api.coral_quality_batch(jobs, want_per_point=True)
    assert (out["status"] == 0).all() and out["pad"][0] == big_bits
    for j in (0, 1, per_launch - 1, per_launch, per_launch + 1, n_jobs - 1):
        ref, rp, src, sp, off = jobs[j]
        exp = _assert_record(out[j], ref, src, rp, sp, off)
        np.testing.assert_array_equal(pps[j][:, 2], exp[:, 2])
        v = exp[:, 2] > 0
        np.testing.assert_allclose(pps[j][v, :2], exp[v, :2], rtol=1e-9, atol=1e-6)
    assert out["count_valid"][1] >= 100
    for j in range(9, n_jobs):                                  # the same job eight records earlier
        assert out[j].tobytes() == out[j - 8].tobytes()
        assert pps[j].tobytes() == pps[j - 8].tobytes()


def test_device_resident_clouds_on_the_scratch_path(matrix):
    import torch
    from tbv_slam_public_amd import api
    ref, src, want = matrix["scratch_bsearch_rows"]
    host = api.CorAlRadarQuality(ref, Z, src, Z, want_per_point=True)
    dev = api.CorAlRadarQuality(torch.from_numpy(ref).cuda(), Z, torch.from_numpy(src).cuda(), Z, want_per_point=True)
    assert host.path == dev.path == want
    assert host.GetQualityMeasure() == dev.GetQualityMeasure() and host.count_valid == dev.count_valid
    np.testing.assert_array_equal(host.per_point, dev.per_point)


# ---- e. refusals (all made by the host or by an early return of the kernel) ---------------------------------------------------------
def _refused(call, status):
    from tbv_slam_public_amd import _lib as L
    with pytest.raises(L.CfearError) as e:
        call()
    assert e.value.status == status


def test_refusals_by_size_radius_and_grid():
    from tbv_slam_public_amd import api, _lib as L
    a, b = G.cluster_pair(50, 300, 300, (0, 12, 0, 12))
    # 16385 merged points: refused at entry
    _refused(lambda: api.coral_quality_batch([(G.clutter(51, 8193, 0, 70, 0, 70), Z, G.clutter(52, 8192, 0, 70, 0, 70), Z, Z)]), L.ERR_CAPACITY)
    for radius in (0.0, -1.0, float("nan")):
        _refused(lambda: api.coral_quality_batch([(a, Z, b, Z, Z)], radius), L.ERR_INVALID_ARGUMENT)
    # two clusters 4200 m apart: more than 4096 grid rows along y, served along x
    ry, sy = G.with_far_cluster(53, a, b, 0.0, 4200.0)
    assert G.predict(ry, sy, Z, Z) is None
    _refused(lambda: api.coral_quality_batch([(ry, Z, sy, Z, Z)]), L.ERR_CAPACITY)
    rx, sx = G.with_far_cluster(53, a, b, 4200.0, 0.0)
    q = _check(rx, sx, Z, Z, (0, 0, 0))
    assert q.path == G.predict(rx, sx, Z, Z) and q.count_valid >= 100
    assert q.per_point[np.concatenate([sx[:, 0] > 1000, rx[:, 0] > 1000]), 2].sum() >= 4
    # radius 0.05 over a 300 m scan: 6000 grid rows
    clouds, gt = _peaks(10, [0, 1])
    assert np.ptp(clouds[0][:, 1]) > 0.05 * 1.0001 * 4096
    _refused(lambda: api.coral_quality_batch([(clouds[0], gt[0], clouds[1], gt[1], Z)], 0.05), L.ERR_CAPACITY)


def test_empty_and_refused_jobs_inside_a_batch():
    """An empty cloud is the job's own status and the call succeeds; a refused job makes the call return its status, and
    every other record is still the oracle's (include/cfear_hip.h)."""
    from tbv_slam_public_amd import _lib as L
    a, b = G.cluster_pair(50, 300, 300, (0, 12, 0, 12))
    ry, sy = G.with_far_cluster(53, a, b, 0.0, 4200.0)
    none = np.zeros((0, 4), np.float32)
    good = (a, Z, b, Z, (0.1, 0.0, 0.0))
    jobs = [good, (a, Z, none, Z, Z), (none, Z, b, Z, Z), (b, Z, a, Z, Z)]
    rc, out, _ = _raw_batch(jobs)
    assert rc == L.OK
    np.testing.assert_array_equal(out["status"], [0, L.ERR_EMPTY_CLOUD, L.ERR_EMPTY_CLOUD, 0])
    for j in (1, 2):
        assert out[j]["overlap"] == 0.0 and out[j]["valid"] == 0 and out[j]["count_valid"] == 0 and out[j]["pad"] == 0
    for j in (0, 3):
        _assert_record(out[j], jobs[j][0], jobs[j][2], Z, Z, jobs[j][4])
    jobs = [good, (ry, Z, sy, Z, Z), (b, Z, a, Z, Z), (ry, Z, sy, Z, Z)]
    rc, out, pp = _raw_batch(jobs, want_per_point=True)
    assert rc == L.ERR_CAPACITY
    np.testing.assert_array_equal(out["status"], [0, L.ERR_CAPACITY, 0, L.ERR_CAPACITY])
    for j in (1, 3):
        assert out[j]["joint"] == 0.0 and out[j]["overlap"] == 0.0 and out[j]["valid"] == 0 and out[j]["pad"] == 0
    for j in (0, 2):
        exp = _assert_record(out[j], jobs[j][0], jobs[j][2], Z, Z, jobs[j][4])
        assert out[j]["count_valid"] >= 100
    np.testing.assert_array_equal(pp[:600, 2], _assert_record(out[0], a, b, Z, Z, (0.1, 0.0, 0.0))[:, 2])
