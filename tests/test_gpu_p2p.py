"""GPU: cfear_p2p_quality_batch, the p2pQuality / keypointRepetability / scanEvaluator mirrors against the NumPy definition
(tests/p2p_cpu.py).

per_point, matched and n_src are compared bit for bit.  sum: the kernel adds per thread in source order and then over a fixed
tree, the definition adds serially; both are sums of n <= n_src non-negative doubles, each within (n - 1) u of the true sum,
u = 2^-53, so they differ by at most 2 n_src 2^-53 relatively.  mean = sum / (matched + 3) is checked as that very division
of the kernel's own sum (IEEE, correctly rounded on both sides), and against the definition's mean with one more rounding on
either side: (2 n_src + 2) 2^-53.

Every checked record also carries, in `pad`, the path of the grid index that served it (CFEAR_CORAL_PATH_*), asserted against
tests/coral_geometry.py::predict_path for the job's reference cloud; test_path_word lists the paths the tests here reach."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import coral_geometry as G
from tests import p2p_cpu as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -53
IDENT = np.array([1, 0, 0, 0, 1, 0], np.float64)


def _api():
    from tbv_slam_public_amd import api
    return api


def _L():
    from tbv_slam_public_amd import _lib
    return _lib


def _pair(rng, n_ref, n_src, span, jitter=1.0, z=0.3):
    """a reference cloud and a source cloud of which about two thirds lie within `jitter` of a reference point"""
    ref = (rng.uniform(-1, 1, (n_ref, 4)) * [span, span, z, 1]).astype(F)
    src = (rng.uniform(-1, 1, (n_src, 4)) * [span, span, z, 1]).astype(F)
    near = rng.random(n_src) < 0.67
    pick = rng.integers(0, n_ref, n_src)
    src[near, :3] = (ref[pick[near], :3] + rng.normal(0, jitter, (int(near.sum()), 3)) * [1, 1, 0.1]).astype(F)
    return np.ascontiguousarray(ref), np.ascontiguousarray(src)


def _check_record(rec, pp, ref, src, T, radius, tag=""):
    want = R.p2p(ref, src, T, radius)
    n = want["n_src"]
    print("%s n_ref %d n_src %d matched %d/%d sum %.17g vs %.17g mean %.17g vs %.17g" % (
        tag, len(ref), n, rec["matched"], want["matched"], rec["sum"], want["sum"], rec["mean"], want["mean"]))
    assert rec["status"] == 0, (tag, rec["status"])
    path = G.predict_path(**G.grid_of_cloud(ref, radius))
    print("%s path %s, predicted %s" % (tag, G.describe(int(rec["pad"])), "a refusal" if path is None else G.describe(path)))
    assert int(rec["pad"]) == path, tag
    assert np.array_equal(np.asarray(pp).view(np.uint32), want["per_point"].view(np.uint32)), tag
    assert (int(rec["matched"]), int(rec["n_src"])) == (want["matched"], n), tag
    assert abs(float(rec["sum"]) - want["sum"]) <= 2 * n * U * want["sum"], tag
    assert float(rec["mean"]) == float(rec["sum"]) / (int(rec["matched"]) + 3), tag
    assert abs(float(rec["mean"]) - want["mean"]) <= (2 * n + 2) * U * want["mean"], tag
    return want


def _run_and_check(jobs, radius, tag=""):
    """jobs: (ref, src, T); one batched call, every record against the definition"""
    out, pp = _api().p2p_quality_batch(jobs, radius, want_per_point=True)
    return [_check_record(out[i], pp[i], ref, src, T, radius, "%s[%d]" % (tag, i)) for i, (ref, src, T) in enumerate(jobs)]


SIZES = (1, 2, 63, 64, 65, 1000)


@pytest.mark.parametrize("n_ref", SIZES)
def test_sizes(n_ref):
    rng = np.random.default_rng(100 + n_ref)
    T = R.tchange((0.5, -0.2, 0.1), (0.7, 0.1, 0.12), (0.05, 0.02, 0.003))
    jobs = []
    for n_src in SIZES:
        ref, src = _pair(rng, n_ref, n_src, 20.0)
        jobs.append((ref, src, T))
    got = _run_and_check(jobs, 3.0, "sizes")                                         # (every record's pad: _check_record)
    assert n_ref < 63 or sum(w["matched"] for w in got) > 0


def test_cluster_inside_one_cell():
    rng = np.random.default_rng(7)
    ref = (rng.uniform(0.1, 2.9, (5000, 4)) * [1, 1, 0.1, 1]).astype(F)         # one 3 m cell, one crowded grid row
    assert G.predict_path(**G.grid_of_cloud(ref, 3.0)) == G.path_bits(0, 0, G.SORT_RADIX)
    src = (rng.uniform(-1.0, 4.0, (777, 4)) * [1, 1, 0.1, 1]).astype(F)
    got = _run_and_check([(ref, src, IDENT)], 3.0, "cluster")
    assert got[0]["matched"] == 777


@pytest.mark.parametrize("radius", [3.0, 0.5])
def test_cloud_spread_over_390_m(radius):
    rng = np.random.default_rng(8)
    ref, src = _pair(rng, 1000, 1000, 390.0, jitter=radius / 2)
    ref[0, :2], ref[1, :2] = (-390.0, -390.0), (390.0, 390.0)
    src[0, :3], src[1, :3] = (-389.9, -390.1, 0.0), (390.2, 389.9, 0.0)             # matches at the corners of the grid and outside it
    # 260 x 260 cells fit the bitmap, 1560 x 1560 do not
    assert G.predict_path(**G.grid_of_cloud(ref, radius)) == G.path_bits(0, radius == 0.5, G.SORT_ROWS)
    got = _run_and_check([(ref, src, IDENT)], radius, "spread")
    assert got[0]["matched"] > 300


def test_largest_clouds():
    """16 384 points each: the bitonic sort, the sorted cloud in the global scratch, sixteen source points per lane"""
    rng = np.random.default_rng(15)
    ref, src = _pair(rng, 16384, 16384, 150.0)
    assert G.predict_path(**G.grid_of_cloud(ref, 3.0)) == G.path_bits(1, 0, G.SORT_BITONIC)
    got = _run_and_check([(ref, src, R.tchange((1.0, 2.0, 0.3), (1.2, 2.1, 0.31)))], 3.0, "largest")
    assert got[0]["matched"] > 8000


def _path_cases():
    """name -> (ref, src, radius, wanted path bits): the smallest clouds that reach each bit of the path word, chosen on the
    CPU with predict_path.  The sorted points leave the LDS when 16 n + 8 V > 131 088 bytes; the bitmap needs 6 bytes per 32
    grid cells behind them; the row sort declines above 512 points in a grid row or 8192 points, the radix sort above 8192."""
    B = G.path_bits
    rng = np.random.default_rng(30)
    out = {}

    def pair(n_ref, n_src, span, jitter=0.5):
        return _pair(rng, n_ref, n_src, span, jitter=jitter)

    out["lds_bitmap_rows"] = (*pair(1500, 300, 20.0), 1.0, B(0, 0, G.SORT_ROWS))
    out["scratch_bitmap_rows"] = (*pair(8000, 300, 40.0), 1.0, B(1, 0, G.SORT_ROWS))         # ~4600 of 80 x 80 cells occupied
    ref, src = pair(1000, 300, 390.0, 0.2)                                                    # 1560 x 1560 cells at radius 0.5
    out["lds_bsearch_rows"] = (ref, src, 0.5, B(0, 1, G.SORT_ROWS))
    ref, src = pair(8000, 300, 40.0)
    ref[0, :2], ref[1, :2] = (-1500.0, -1500.0), (1500.0, 1500.0)                            # 3000 x 3000 cells
    out["scratch_bsearch_rows"] = (ref, src, 1.0, B(1, 1, G.SORT_ROWS))
    ref, src = pair(1500, 300, 20.0)
    ref[:600, 1] = rng.uniform(0.1, 0.9, 600).astype(F)                                      # 600 points in one grid row
    out["lds_bitmap_radix"] = (ref, src, 1.0, B(0, 0, G.SORT_RADIX))
    out["scratch_bitmap_bitonic"] = (*pair(8200, 300, 40.0), 1.0, B(1, 0, G.SORT_BITONIC))
    return out


PATH_CASES = _path_cases()


@pytest.mark.parametrize("name", sorted(PATH_CASES))
def test_path_word(name):
    """cfear_p2p_result.pad names the path that served the job.  Between them, these cases and test_cluster_inside_one_cell,
    test_cloud_spread_over_390_m and test_largest_clouds show every bit: LDS and scratch, bitmap and binary search, and the
    row, radix and bitonic sorts."""
    ref, src, radius, want = PATH_CASES[name]
    assert G.predict_path(**G.grid_of_cloud(ref, radius)) == want, G.describe(want)          # the input is what its name says
    out, pp = _api().p2p_quality_batch([(ref, src, IDENT)], radius, want_per_point=True)
    got = _check_record(out[0], pp[0], ref, src, IDENT, radius, name)                         # pad against the prediction, which is `want`
    assert got["matched"] > 100


def test_path_word_cases_cover_every_bit():
    words = [c[3] for c in PATH_CASES.values()]
    assert {w & 1 for w in words} == {0, 1} and {(w >> 1) & 1 for w in words} == {0, 1}
    assert {(w >> 2) & 3 for w in words} == {G.SORT_ROWS, G.SORT_RADIX, G.SORT_BITONIC}


def test_more_large_clouds_than_one_launch_holds():
    """520 distinct reference clouds for which the HOST reserves the scratch (it sizes it from 24 bytes a point, the most a
    point can take with its cell table: 5600 points -> 134 464 > 131 088): the scratch holds two workgroups per compute
    unit (512 on an MI355X), so the batch takes a second launch.  That two-launch logic is what this test pins.  The
    KERNEL decides from the occupied cells it finds -- 3197 here, 115 200 bytes with the points -- and keeps these clouds
    in LDS: the path word says lds/bitmap/rows, asserted below (the scratch path itself: test_path_word,
    test_largest_clouds).  The clouds are copies, so one definition run serves every job; an infinite source point is
    scanned nowhere and has no neighbour."""
    rng = np.random.default_rng(17)
    ref, src = _pair(rng, 5600, 40, 100.0)
    src[3, 0], src[4, 1] = np.inf, -np.inf
    T = R.tchange((0, 0, 0), (0, 0, 0.001))          # a rotation: an infinite coordinate stays infinite (under the identity 0 * inf is NaN)
    refs = np.ascontiguousarray(np.broadcast_to(ref, (520,) + ref.shape))
    jobs = [(refs[k], src, T) for k in range(520)]
    assert G.predict_path(**G.grid_of_cloud(ref, 3.0)) == G.path_bits(0, 0, G.SORT_ROWS) and len(ref) * 24 + 64 > G.ROWBEG_OFF
    out, pp = _api().p2p_quality_batch(jobs, 3.0, want_per_point=True)
    want = _check_record(out[0], pp[0], ref, src, T, 3.0, "launches[0]")
    assert int(out[0]["pad"]) == G.path_bits(0, 0, G.SORT_ROWS)
    assert np.all(np.isinf(R.transform(src, T)[3:5, :2]))
    assert want["matched"] > 20 and want["per_point"][3] == want["per_point"][4] == -1
    assert all(out[k].tobytes() == out[0].tobytes() for k in range(520))
    assert all(np.array_equal(pp[k].view(np.uint32), pp[0].view(np.uint32)) for k in (1, 255, 511, 512, 519))


def test_radius_boundary_is_strict():
    ref = np.zeros((1, 4), F)
    below = np.nextafter(F(3), F(0))
    src = np.array([[3, 0, 0, 0], [below, 0, 0, 0], [0, 0, 3, 0], [0, 0, below, 0], [-3, 0, 0, 0], [0, -below, 0, 0]], F)
    got = _run_and_check([(ref, src, IDENT)], 3.0, "strict")
    assert got[0]["matched"] == 3
    assert list(got[0]["per_point"] >= 0) == [False, True, False, True, False, True]


@pytest.mark.parametrize("radius", [3.0, 0.5])
def test_pairs_straddling_cell_edges(radius):
    """reference points a hair on either side of the grid lines, source points about one radius away on the other side: the
    nearest neighbour lies in the neighbouring cell, at distances on both sides of the radius"""
    rng = np.random.default_rng(9)
    cell = radius * 1.0001
    n = 600
    k = rng.integers(-120, 120, n)
    side = rng.choice([-1.0, 1.0], n)
    ref = np.zeros((n, 4), F)
    ref[:, 0] = (k * cell + side * rng.uniform(0, 1e-3, n) * radius).astype(F)
    ref[:, 1] = (rng.integers(-120, 120, n) * cell + rng.choice([-1.0, 1.0], n) * rng.uniform(0, 1e-3, n) * radius).astype(F)
    src = ref.copy()
    ang = rng.uniform(0, 2 * np.pi, n)
    dist = radius * np.where(rng.random(n) < 0.5, 1 - rng.uniform(0, 3e-7, n), 1 + rng.uniform(0, 3e-7, n))
    src[:, 0] = (ref[:, 0] + dist * np.cos(ang)).astype(F)
    src[:, 1] = (ref[:, 1] + dist * np.sin(ang)).astype(F)
    src[::7, :2] = ref[::7, :2] + F(radius) * np.array([1, 0], F)                   # exactly one radius along x
    got = _run_and_check([(ref, src, IDENT)], radius, "edges")
    assert 100 < got[0]["matched"] < n - 100


def test_duplicates_and_out_of_range():
    rng = np.random.default_rng(10)
    ref, _ = _pair(rng, 200, 1, 30.0)
    dup = ref.copy()
    far = ref.copy()
    far[:, 0] += 500.0
    got = _run_and_check([(ref, dup, IDENT), (ref, far, IDENT)], 3.0, "dup")
    assert got[0]["matched"] == 200 and got[0]["sum"] == 0.0 and np.all(got[0]["per_point"] == 0)
    out, _ = _api().p2p_quality_batch([(ref, far, IDENT)], 3.0)
    assert out[0]["matched"] == 0 and out[0]["mean"] == 0.0 and out[0]["status"] == 0


def test_transform_composed_by_the_api():
    api = _api()
    rng = np.random.default_rng(11)
    ref, src = _pair(rng, 500, 400, 40.0, z=2.0)
    assert np.abs(src[:, 2]).max() > 1.0
    poses = [((12.5, -3.25, 0.7), (13.1, -2.9, 0.74), (0.0, 0.0, 0.0)), ((-40.0, 17.0, -2.9), (-39.5, 17.2, -2.85), (0.5, 0.0, 0.0099)),
             ((0.0, 0.0, 0.0), (0.3, 0.1, 3.1), (-0.35, 0.35, 0.0099))]
    out, pp = api.p2p_quality_batch([(ref, rp, src, sp, off) for rp, sp, off in poses], 3.0, want_per_point=True)
    for i, (rp, sp, off) in enumerate(poses):
        T = R.tchange(rp, sp, off)
        assert np.array_equal(api.p2p_tchange(rp, sp, off).view(np.uint64), T.view(np.uint64))
        # the source cloud is placed so that the composed transform keeps it near the reference
        src_i = src.copy()
        Tm = np.array([[T[0], T[1], T[2]], [T[3], T[4], T[5]], [0, 0, 1]])
        back = np.linalg.inv(Tm) @ np.vstack([src[:, 0], src[:, 1], np.ones(len(src))])
        src_i[:, 0], src_i[:, 1] = back[0].astype(F), back[1].astype(F)
        o2, p2 = api.p2p_quality_batch([(ref, rp, src_i, sp, off)], 3.0, want_per_point=True)
        want = _check_record(o2[0], p2[0], ref, src_i, T, 3.0, "transform[%d]" % i)
        assert want["matched"] > 100
        _check_record(out[i], pp[i], ref, src, T, 3.0, "transform-far[%d]" % i)
    # z enters d: the same pair with the source lifted by 2 m matches fewer points, at larger distances
    lifted = src.copy()
    lifted[:, 2] += 2.0
    a, b = _run_and_check([(ref, src, IDENT), (ref, lifted, IDENT)], 3.0, "z")
    assert b["matched"] < a["matched"]


@pytest.mark.parametrize("n_jobs", [1, 13, 257])
def test_batches_share_clouds_and_do_not_depend_on_position(n_jobs):
    api = _api()
    rng = np.random.default_rng(12)
    clouds = [_pair(rng, 300 + 50 * k, 257 + 31 * k, 25.0) for k in range(4)]
    vek = R.create_perturbations(12, 2 * math.pi, 0.5, 0.0099)
    jobs = []
    for j in range(n_jobs):
        ref, src = clouds[(j // 13) % 4]
        jobs.append((ref, src, R.tchange((0, 0, 0), (0, 0, 0), vek[j % 13])))
    if n_jobs > 13:                                                                 # a cloud as reference here, as source there
        jobs[20] = (clouds[1][0], clouds[0][0], jobs[20][2])
    out, pp = api.p2p_quality_batch(jobs, 3.0, want_per_point=True)
    for j in sorted({0, 5, 12, 13, 20, n_jobs // 2, n_jobs - 1} & set(range(n_jobs))):
        _check_record(out[j], pp[j], *jobs[j], 3.0, "batch%d[%d]" % (n_jobs, j))
    probe = jobs[n_jobs // 2]
    alone, pa = api.p2p_quality_batch([probe], 3.0, want_per_point=True)
    first, pf = api.p2p_quality_batch([probe] + jobs, 3.0, want_per_point=True)
    last, pl = api.p2p_quality_batch(jobs + [probe], 3.0, want_per_point=True)
    for rec, row in ((out[n_jobs // 2], pp[n_jobs // 2]), (first[0], pf[0]), (last[-1], pl[-1])):
        assert rec.tobytes() == alone[0].tobytes()
        assert np.array_equal(row.view(np.uint32), pa[0].view(np.uint32))
    assert first[1:].tobytes() == out.tobytes() == last[:-1].tobytes()


def test_device_pointers_equal_host_pointers():
    import torch
    api, L = _api(), _L()
    rng = np.random.default_rng(13)
    clouds = [_pair(rng, 400, 300, 25.0), _pair(rng, 7000, 900, 120.0)]            # the second leaves the LDS for the scratch
    vek = R.create_perturbations(4, 2 * math.pi, 0.5, 0.0099)
    host = [(clouds[k][0], clouds[k][1], R.tchange((0, 0, 0), (0, 0, 0), v)) for k in range(2) for v in vek]
    dev_clouds = [(torch.from_numpy(r).cuda(), torch.from_numpy(s).cuda()) for r, s in clouds]
    dev = [(dev_clouds[k][0], dev_clouds[k][1], R.tchange((0, 0, 0), (0, 0, 0), v)) for k in range(2) for v in vek]
    out_h, pp_h = api.p2p_quality_batch(host, 3.0, want_per_point=True)
    out_d, pp_d = api.p2p_quality_batch(dev, 3.0, want_per_point=True, device_out=True)
    torch.cuda.synchronize()
    rec = np.frombuffer(out_d.cpu().numpy().tobytes(), L.P2P_RESULT_DTYPE)
    assert rec.tobytes() == out_h.tobytes()
    assert np.array_equal(pp_d.cpu().numpy().view(np.uint32), np.concatenate(pp_h).view(np.uint32))
    out_m, pp_m = api.p2p_quality_batch(dev, 3.0, want_per_point=True)             # device clouds, host records
    assert out_m.tobytes() == out_h.tobytes() and all(np.array_equal(a, b) for a, b in zip(pp_m, pp_h))
    for i in (0, 5, 9):
        _check_record(out_h[i], pp_h[i], *host[i], 3.0, "device[%d]" % i)


def test_refusals():
    api, L = _api(), _L()
    rng = np.random.default_rng(14)
    ref, src = _pair(rng, 300, 200, 20.0)
    good = (ref, src, IDENT)
    want = R.p2p(ref, src, IDENT, 3.0)

    def ok(rec):
        return rec["status"] == 0 and rec["matched"] == want["matched"] and abs(rec["sum"] - want["sum"]) <= 400 * U * want["sum"]

    def refused(jobs, radius, status):
        with pytest.raises(L.CfearError) as e:
            api.p2p_quality_batch(jobs, radius)
        assert e.value.status == status
        out, _ = api.p2p_quality_batch([good], 3.0)                                 # a correct call right after a refused one
        assert ok(out[0])

    big = np.zeros((L.P2P_MAX_REF_POINTS + 1, 4), F)
    refused([good, (big, src, IDENT)], 3.0, L.ERR_CAPACITY)                         # at entry, before any launch
    for r in (0.0, -1.0, float("nan")):
        refused([good], r, L.ERR_INVALID_ARGUMENT)
    # per-job statuses: the call fails with the first, every record is written, the neighbours are valid
    ctx = api.default_context()
    for bad_ref in (False, True):
        nan_cloud = (ref if bad_ref else src).copy()
        nan_cloud[17, 1] = np.nan
        jobs = [good, (nan_cloud, src, IDENT) if bad_ref else (ref, nan_cloud, IDENT), good]
        arr = (L.P2pJob * 3)()
        keep = []
        for i, (rc, sc, T) in enumerate(jobs):
            keep += [rc, sc]
            arr[i].ref_xyzi, arr[i].src_xyzi, arr[i].n_ref, arr[i].n_src = rc.ctypes.data, sc.ctypes.data, len(rc), len(sc)
            for k in range(6):
                arr[i].T[k] = T[k]
        out = np.zeros(3, L.P2P_RESULT_DTYPE)
        assert ctx._lib.cfear_p2p_quality_batch(ctx.h, arr, 3, 3.0, out.ctypes.data, None) == L.ERR_CAPACITY
        assert list(out["status"]) == [0, L.ERR_CAPACITY, 0] and ok(out[0]) and ok(out[2])
        assert out[1]["matched"] == 0 and out[1]["mean"] == 0.0
        refused(jobs, 3.0, L.ERR_CAPACITY)
    # an empty cloud is its job's status and does not fail the call
    empty = np.zeros((0, 4), F)
    out, pp = api.p2p_quality_batch([good, (ref, empty, IDENT), (empty, src, IDENT), good], 3.0, want_per_point=True)
    assert list(out["status"]) == [0, L.ERR_EMPTY_CLOUD, L.ERR_EMPTY_CLOUD, 0] and ok(out[0]) and ok(out[3])
    assert len(pp[1]) == 0 and np.all(pp[2] == -1) and (out[1]["n_src"], out[2]["n_src"]) == (0, 200)
    rep = api.keypointRepetability({"T": (0, 0, 0), "cloud": ref}, {"T": (0, 0, 0), "cloud": empty})
    assert math.isnan(rep.GetQualityMeasure()[0]) and rep.GetQualityMeasure()[1:] == [0.0, 0.0]


def test_cen2018_landmarks_stay_on_the_device():
    import torch
    from tbv_slam_public_amd import synth
    api = _api()
    imgs, gt, _ = synth.scene_v1(2, 2)
    r = api.filter_cen2018(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), zq=5.0, sigma_gauss=17, min_range_bins=2,
                           range_res=0.0438, cap_points=16384)
    n = [int(v) for v in r["n_points"]]
    assert 1000 < min(n) and max(n) <= 16384
    scans = [{"T": tuple(float(v) for v in gt[b]), "cloud": r["xyzi"][b, :n[b]].contiguous(), "type": "Cen2018Radar"} for b in range(2)]
    par = api.AlignmentQualityParameters(method="P2P")
    off = (0.2, -0.1, 0.004)
    q = api.AlignmentQualityFactory.CreateQualityType(scans[0], scans[1], par, off)
    assert isinstance(q, api.p2pQuality) and par.radius == 3.0
    host = [s["cloud"].cpu().numpy() for s in scans]
    want = R.p2p(host[0], host[1], R.tchange(scans[0]["T"], scans[1]["T"], off), 3.0)
    res = q.GetResiduals()
    assert res[:3] == [0.0, 0.0, 0.0] and res == want["residuals"] and want["matched"] > 500
    assert abs(q.GetQualityMeasure()[0] - want["mean"]) <= (2 * n[1] + 2) * U * want["mean"] and q.GetQualityMeasure()[1:] == [0.0, 0.0]
    rep = api.keypointRepetability(scans[0], scans[1], par, off)
    assert rep.GetQualityMeasure() == want["repeatability"] and rep.GetResiduals() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        api.AlignmentQualityFactory.CreateQualityType(scans[0], scans[1], api.AlignmentQualityParameters(method="Coral"), off)
    with pytest.raises(ValueError):
        api.AlignmentQualityFactory.CreateQualityType(scans[0], scans[1], api.AlignmentQualityParameters(method="keypoint_repetability"), off)


def test_scan_evaluator(tmp_path):
    api = _api()
    scans = R.synthetic_sequence(8)
    for spacing, steps in ((1, 2), (2, 4)):
        epar = api.scanEvaluatorParameters(scan_spacing=spacing, offset_rotation_steps=steps)
        ev = api.scanEvaluator(scans, epar, api.AlignmentQualityParameters(method="P2P"))
        want = R.evaluate(scans, "P2P", 3.0, spacing, offset_rotation_steps=steps)
        assert len(ev.datapoints_) == len(want) == (8 - spacing) * (steps + 1)
        assert ev.vek_perturbation_ == R.create_perturbations(steps)
        for g, w in zip(ev.datapoints_, want):
            for key in ("index", "ref_id", "src_id", "distance", "aligned", "perturbation", "residuals"):
                assert g[key] == w[key], key
            assert abs(g["score"][0] - w["score"][0]) <= (2 * 300 + 2) * U * w["score"][0] and g["score"][1:] == [0.0, 0.0]
        path = ev.SaveEvaluation(str(tmp_path / ("eval%d.txt" % spacing)))
        text = open(path).read()
        assert text.split("\n")[0] == ",".join(R.HEADER) and len(text.split("\n")) == len(want) + 2
        got_rows, want_rows = text.split("\n")[1:-1], R.eval_text(want).split("\n")[1:-1]
        assert [r.split(",")[:4] + r.split(",")[5:] for r in got_rows] == [r.split(",")[:4] + r.split(",")[5:] for r in want_rows]
        if spacing == 1:                                                            # the aligned row scores best in every pair
            for i in range(0, len(want), steps + 1):
                assert ev.datapoints_[i]["aligned"]
                assert ev.datapoints_[i]["score"][0] < min(d["score"][0] for d in ev.datapoints_[i + 1:i + steps + 1])
    rep = api.scanEvaluator([dict(s, type="BFARScan") for s in scans], None, api.AlignmentQualityParameters(method="keypoint_repetability"))
    want = R.evaluate(scans, "keypoint_repetability", 3.0, 1)
    assert [d["score"] for d in rep.datapoints_] == [d["score"] for d in want]
    # method "Coral": the rows are coral_quality_batch's, job by job -- the evaluator adds nothing of its own
    qpar = api.AlignmentQualityParameters(method="Coral", radius=1.0)
    ev = api.scanEvaluator(scans, None, qpar)
    i = 0
    for k in range(1, 8):
        for verr in ev.vek_perturbation_:
            one, _ = api.coral_quality_batch([(scans[k - 1]["cloud"], scans[k - 1]["T"], scans[k]["cloud"], scans[k]["T"], verr)], 1.0)
            assert ev.datapoints_[i]["score"] == [float(one[0]["joint"]), float(one[0]["sep"]), float(one[0]["overlap"])]
            assert ev.datapoints_[i]["residuals"] == [0.0, 0.0, 0.0]
            i += 1
    assert i == len(ev.datapoints_) == 21
    with pytest.raises(ValueError):
        api.scanEvaluator([dict(s, type="Cen2018Radar") for s in scans], None, qpar)


def test_cpp_mirror(tmp_path):
    api = _api()
    exe = str(tmp_path / "p2p_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "p2p_signature.cpp"), "-o", exe, "-L", so_dir, "-lcfear_hip",
                           "-Wl,-rpath," + so_dir])
    assert subprocess.run([exe], capture_output=True, text=True).returncode == 0     # the signature block alone
    scans = R.synthetic_sequence(4)
    p = tmp_path / "scans.bin"
    with open(p, "wb") as fh:
        fh.write(np.int32(len(scans)).tobytes())
        for s in scans:
            fh.write(np.int32(len(s["cloud"])).tobytes() + np.asarray(s["T"], np.float64).tobytes() + s["cloud"].tobytes())
    out_txt = tmp_path / "eval.txt"
    r = subprocess.run([exe, str(p), str(out_txt), "3.0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    v = r.stdout.split()
    off = (0.3, -0.2, 0.01)
    q = api.p2pQuality(scans[0], scans[1], api.AlignmentQualityParameters(method="P2P"), off)
    rep = api.keypointRepetability(scans[0], scans[1], api.AlignmentQualityParameters(method="P2P"), off)
    assert [float(x) for x in v[0:3]] == q.GetQualityMeasure()
    assert [float(x) for x in v[3:6]] == rep.GetQualityMeasure()
    assert int(v[6]) == len(q.GetResiduals()) and int(v[8]) == 9 and int(v[9]) == 3
    want = R.p2p(scans[0]["cloud"], scans[1]["cloud"], R.tchange(scans[0]["T"], scans[1]["T"], off), 3.0)
    assert [float(x) for x in v[3:6]] == want["repeatability"]
    ev = api.scanEvaluator(scans, None, api.AlignmentQualityParameters(method="P2P"))
    assert open(out_txt).read() == ev.EvaluationText()


def test_scan_evaluator_on_cfear_features():
    """CFEARFeatures scans: the evaluator's rows and the factory's CFEARQuality are cfear_quality_batch's, job by job"""
    api = _api()
    rng = np.random.default_rng(16)
    a, b = rng.uniform(-30, 30, (24, 2)), rng.uniform(-30, 30, (24, 2))             # 24 walls, 120 returns each
    t = rng.uniform(0, 1, (24, 120, 1))
    world = (a[:, None] * (1 - t) + b[:, None] * t).reshape(-1, 2)
    scans = []
    for k in range(4):
        T = (0.8 * k, 0.1 * k, 0.02 * k)
        c, s = math.cos(T[2]), math.sin(T[2])
        dx, dy = world[:, 0] - T[0] + rng.normal(0, 0.03, len(world)), world[:, 1] - T[1] + rng.normal(0, 0.03, len(world))
        cloud = np.zeros((len(world), 4), F)
        cloud[:, 0], cloud[:, 1], cloud[:, 3] = c * dx + s * dy, -s * dx + c * dy, 100.0
        scans.append({"T": T, "cloud": cloud, "CFEAR": api.MapPointNormal(cloud, 3.0), "pose_id": k, "type": "CFEARFeatures"})
    assert min(s["CFEAR"].GetSize() for s in scans) > 20
    for method in ("P2L", "P2P"):
        qpar = api.AlignmentQualityParameters(method=method)
        ev = api.scanEvaluator(scans, None, qpar)
        assert len(ev.datapoints_) == 9
        i = 0
        for k in range(1, 4):
            for verr in ev.vek_perturbation_:
                one = api.cfear_quality_batch([(scans[k - 1]["CFEAR"], scans[k - 1]["T"], scans[k]["CFEAR"], scans[k]["T"], verr)], method)
                d = ev.datapoints_[i]
                assert d["score"] == [float(v) for v in one[0]] and d["residuals"] == [0.0, 0.0, 0.0]
                assert (d["index"], d["ref_id"], d["src_id"]) == (k, k - 1, k)
                i += 1
        assert all(d["score"][1] > 0 and d["score"][2] > 20 for d in ev.datapoints_)       # GetCost served every job
        q = api.AlignmentQualityFactory.CreateQualityType(scans[0], scans[1], qpar, tuple(ev.vek_perturbation_[1]))
        assert isinstance(q, api.CFEARQuality) and q.GetQualityMeasure() == ev.datapoints_[1]["score"] and q.valid_
        assert q.GetResiduals() == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        api.scanEvaluator(scans, None, api.AlignmentQualityParameters(method="Coral"))
    coral = api.AlignmentQualityFactory.CreateQualityType(dict(scans[0], type="kstrongRadar"), dict(scans[1], type="kstrongRadar"),
                                                          api.AlignmentQualityParameters(method="Coral", radius=1.0))
    assert isinstance(coral, api.CorAlRadarQuality) and coral.GetResiduals() == [0.0, 0.0, 0.0] and len(coral.GetQualityMeasure()) == 3
