"""GPU: Scan Context kernels against the CPU oracle (and the NumPy restatement of the raw path) away from TBV's 40 x 120
default, over the geometry grid of tests/sc_geometry.py: cloud and local-map descriptors and keys bit-exact on every cell
(only points whose sector depends on how atan rounds are removed, and none from the edge cloud), the intensity domain of
the descriptor, the column-shift distance bit for bit over search ratios up to 2.5 (several similarity chunks, duplicated
shifts), refusals of the shapes the distance kernel cannot hold, and raw sweeps at other ring x sector counts."""
import math

import numpy as np
import pytest

from tests import sc_geometry as G

pytestmark = pytest.mark.gpu

SHIFTS = (0.0, -2.0, 2.0, -4.0, 4.0)
NO_POINT = -7.5


def _gid(g):
    return "%dx%d_r%g" % g


def _par(R, S, rmax, **kw):
    from tbv_slam_public_amd import api
    return api.sc_params(num_ring=R, num_sector=S, max_radius=rmax, **kw)


def _unambiguous(c, R, S, rmax, shifts=SHIFTS):
    bad = np.zeros(len(c), bool)
    for dy in shifts:
        bad |= G.ambiguous(c, R, S, rmax, dy)
    assert bad.sum() <= max(3, len(c) // 200), int(bad.sum())      # rare: a point within an ulp of a sector edge
    return c[~bad]


# ---- descriptors and keys ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", G.GEOMETRIES, ids=_gid)
def test_descriptors_and_keys_exact_on_every_cell(geom):
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    R, S, rmax = geom
    clouds = [_unambiguous(G.random_cloud(100 + i, R, S, rmax), R, S, rmax) for i in range(2)]
    for fn in ("sum", "max"):
        for div in (1000.0, 1.0):
            par = _par(R, S, rmax, desc_function=fn, desc_divider=div, no_point=NO_POINT)
            desc, rk, sk = api.sc_descriptors(clouds, par, SHIFTS)
            assert desc.shape == (2, 5, R, S)
            for i, c in enumerate(clouds):
                for k, dy in enumerate(SHIFTS):
                    e = O.sc_descriptor(c, R, S, rmax, fn, div, NO_POINT, dy)
                    np.testing.assert_array_equal(desc[i, k], e, err_msg="%s %g cloud %d shift %g" % (fn, div, i, dy))
                    erk, esk = O.sc_keys(e)
                    np.testing.assert_array_equal(rk[i, k], erk)
                    np.testing.assert_array_equal(sk[i, k], esk)
            if div == 1.0 and R * S > 8:
                assert (desc == NO_POINT).any()                    # empty bins take no_point when the divider is 1


@pytest.mark.parametrize("geom", G.GEOMETRIES, ids=_gid)
def test_edge_cloud_exact(geom):
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    R, S, rmax = geom
    c = G.edge_cloud(R, S, rmax)
    assert not G.ambiguous(c, R, S, rmax).any()
    ring, _ = O.sc_bins(c, R, S, rmax)
    x = c[:, 0]
    rim = ring[(x == np.float32(rmax)) & (c[:, 1] == 0)]
    assert len(rim) >= 2 and (rim == R - 1).all()                                              # the rim is kept
    assert (ring[x == np.nextafter(np.float32(rmax), np.float32(np.inf))] == -1).all()        # the next float is not
    for fn in ("sum", "max"):
        for div in (1.0, 1000.0):
            par = _par(R, S, rmax, desc_function=fn, desc_divider=div, no_point=NO_POINT)
            desc, rk, sk = api.sc_descriptors([c], par)
            e = O.sc_descriptor(c, R, S, rmax, fn, div, NO_POINT)
            np.testing.assert_array_equal(desc[0, 0], e, err_msg="%s %g" % (fn, div))
            erk, esk = O.sc_keys(e)
            np.testing.assert_array_equal(rk[0, 0], erk)
            np.testing.assert_array_equal(sk[0, 0], esk)


def _graph_without_ambiguous_points(R, S, rmax, n_agg, n=9, seed=40):
    """A small pose graph whose local maps hold no point an atan rounding could move: member points that are ambiguous
    in some centre's merged cloud (at some lateral shift) are removed until none is left."""
    from tests.test_gpu_sc_sequence import _merge
    from tbv_slam_public_amd import synth
    clouds, poses = synth.sc_graph(n, seed=seed, points=400, step=3.0)
    clouds = [c.copy() for c in clouds]
    for c in clouds:
        c[:, :2] *= np.float32(rmax / 80.0)                        # fill the geometry's disc
    poses = poses.copy()
    poses[:, :2] *= rmax / 80.0
    ids = np.arange(n)
    for _ in range(6):
        drop = [np.zeros(len(c), bool) for c in clouds]
        for i in range(n):
            m = _merge(clouds, poses, ids, i, n_agg)
            bad = np.zeros(len(m), bool)
            for dy in SHIFTS:
                bad |= G.ambiguous(m, R, S, rmax, dy)
            mem = [j for j in range(n) if abs(j - i) <= n_agg]
            off = np.cumsum([0] + [len(clouds[j]) for j in mem])
            for j, a, b in zip(mem, off[:-1], off[1:]):
                drop[j] |= bad[a:b]
        if not any(d.any() for d in drop):
            return clouds, poses, ids
        clouds = [c[~d] for c, d in zip(clouds, drop)]
    raise AssertionError("ambiguous points keep appearing")


@pytest.mark.parametrize("geom", [(37, 113, 80.0), (20, 60, 50.0), (64, 80, 120.0), (1, 2048, 80.0)], ids=_gid)
@pytest.mark.parametrize("n_agg", [0, 2, 5])
def test_local_map_descriptors_match_oracle(geom, n_agg):
    from oracle import pyoracle as O
    from tests.test_gpu_sc_sequence import _merge
    from tbv_slam_public_amd import api
    R, S, rmax = geom
    clouds, poses, ids = _graph_without_ambiguous_points(R, S, rmax, n_agg)
    for fn, div in (("sum", 1000.0), ("max", 1.0)):
        par = _par(R, S, rmax, desc_function=fn, desc_divider=div, no_point=NO_POINT)
        desc, rk, sk = api.sc_local_map_descriptors(clouds, poses, n_agg, None, par, SHIFTS)
        for i in range(len(clouds)):
            m = _merge(clouds, poses, ids, i, n_agg)
            for k, dy in enumerate(SHIFTS):
                e = O.sc_descriptor(m, R, S, rmax, fn, div, NO_POINT, dy)
                np.testing.assert_array_equal(desc[i, k], e, err_msg="%s node %d shift %g" % (fn, i, dy))
                erk, esk = O.sc_keys(e)
                np.testing.assert_array_equal(rk[i, k], erk)
                np.testing.assert_array_equal(sk[i, k], esk)


# ---- the intensity domain (include/cfear_hip.h, cfear_sc_descriptors) ----------------------------------------------

def _one_bin(values, x=10.0, y=0.5):
    c = np.zeros((len(values), 4), np.float32)
    c[:, 0], c[:, 1], c[:, 3] = x, y, values
    return c


def test_large_integer_intensities_stack_exactly():
    """Inside the domain (non-negative integer values, bin sums below 2^53) the order of arrival cannot matter: 4096
    points of up to 2^24 in one bin, and a bin of 2^24 - 1 next to ones."""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(7)
    big = rng.integers(2 ** 23, 2 ** 24 + 1, 4096).astype(np.float32)
    c = np.concatenate([_one_bin(big), _one_bin([2 ** 24 - 1] + [1] * 999, 30.0, -4.0), _one_bin([0.0], 50.0, 20.0)])
    for fn in ("sum", "max"):
        for div in (1.0, 1000.0):
            par = _par(40, 120, 80.0, desc_function=fn, desc_divider=div)
            desc = api.sc_descriptors([c], par, SHIFTS)[0]
            for k, dy in enumerate(SHIFTS):
                np.testing.assert_array_equal(desc[0, k], O.sc_descriptor(c, 40, 120, 80.0, fn, div, 0.0, dy))
    s = api.sc_descriptors([c], _par(40, 120, 80.0, desc_divider=1.0))[0][0, 0]
    assert s.max() == float(big.astype(np.float64).sum()) and s.max() > 2 ** 35


def test_outside_the_domain_bins_hold_the_plain_sum_or_maximum():
    """Pinned behaviour outside the domain: "sum" bins hold the sum of every intensity, "max" bins the maximum; the
    reference's rule (a bin still at NO_POINT = -1000 is replaced, not added to) is not followed.  A result equal to
    NO_POINT after the division still becomes no_point, as in the reference."""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    bins = {(5.0, 0.5): [-1000.0, 5.0], (15.0, 0.5): [600.0, -1600.0, 7.0], (25.0, 0.5): [-3.0],
            (35.0, 0.5): [-400.0, -600.0], (45.0, 0.5): [-1000.0, -2000.0], (55.0, 0.5): [12.0, 30.0]}
    c = np.concatenate([_one_bin(v, x, y) for (x, y), v in bins.items()])
    par = _par(40, 120, 80.0, desc_divider=1.0, no_point=NO_POINT)
    got = api.sc_descriptors([c], par)[0][0, 0]
    mx = api.sc_descriptors([c], _par(40, 120, 80.0, desc_function="max", desc_divider=1.0, no_point=NO_POINT))[0][0, 0]
    ref = O.sc_descriptor(c, 40, 120, 80.0, "sum", 1.0, NO_POINT)
    ring, sec = O.sc_bins(c, 40, 120, 80.0)
    for (x, y), v in bins.items():
        k = int(np.flatnonzero((c[:, 0] == np.float32(x)))[0])
        cell = (ring[k], sec[k])
        s = math.fsum(v)
        assert got[cell] == (NO_POINT if s == -1000.0 else s), (x, v, got[cell])
        assert mx[cell] == (NO_POINT if max(v) == -1000.0 else max(v)), (x, v, mx[cell])
    cell = lambda x: (ring[c[:, 0] == np.float32(x)][0], sec[c[:, 0] == np.float32(x)][0])   # noqa: E731
    assert ref[cell(5.0)] == 5.0 and got[cell(5.0)] == -995.0          # the reference replaces the -1000 it reached
    assert ref[cell(55.0)] == got[cell(55.0)] == 42.0                  # inside the domain both agree
    empty = np.ones((40, 120), bool)
    empty[ring, sec] = False
    assert (got[empty] == NO_POINT).all()


def test_fractional_intensities_sum_to_within_rounding():
    """Outside the domain: a sum of fractional intensities depends on the order of arrival only in its last bits."""
    from tbv_slam_public_amd import api
    v = (np.random.default_rng(3).uniform(0, 1, 3000)).astype(np.float32)
    got = api.sc_descriptors([_one_bin(v)], _par(40, 120, 80.0, desc_divider=1.0))[0][0, 0]
    exact = math.fsum(v.astype(np.float64))
    assert abs(got.max() - exact) <= 3000 * np.finfo(np.float64).eps * exact


# ---- distance ------------------------------------------------------------------------------------------------------

def _distance_set(R, S, rmax, seed):
    """Descriptors (oracle-made, so the distance is checked on its own): two places, rotated copies, all-zero columns,
    two all-empty descriptors, TBV's empty descriptor, and periodic column patterns (argmin ties in both searches)."""
    from oracle import pyoracle as O
    a = O.sc_descriptor(G.random_cloud(seed, R, S, rmax), R, S, rmax)
    b = O.sc_descriptor(G.random_cloud(seed + 1, R, S, rmax, n=800), R, S, rmax, "max", 1.0)
    holes = a.copy()
    holes[:, ::3] = 0.0
    holes[:, S // 2:S // 2 + max(S // 5, 1)] = 0.0
    p = max(S // 6, 1)
    rng = np.random.default_rng(seed)
    period = np.tile(rng.integers(0, 4, (R, p)).astype(np.float64), (1, S // p + 1))[:, :S]
    const = np.full((R, S), 0.25)
    const[R // 2] = 1.0
    zero = np.zeros((R, S))
    return [a, np.roll(a, -(S // 7 + 1), axis=1), np.roll(a, S // 2, axis=1), b, holes, zero, zero.copy(),
            np.full((R, S), -1.0), period, np.roll(period, 1, axis=1), const]


def _check_distances(D, R, S, ratio, pairs):
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    par = _par(R, S, 80.0, search_ratio=ratio)
    dist, shift = api.sc_distance_batch(D, D, pairs, par)
    for (q, c), d, s in zip(pairs, dist, shift):
        ed, es = O.sc_distance(D[q], D[c], ratio)
        assert s == es and (d == ed or (np.isnan(d) and np.isnan(ed))), (R, S, ratio, q, c, d, ed, s, es)
    # argmin_shift lies in [0, S) while round(0.5 ratio S) <= S; past that the reference's index arithmetic also yields
    # shifts in (-S, 0) (include/cfear_hip.h, cfear_sc_distance_batch)
    lo = 0 if G.search_space_size(S, ratio) <= 2 * S + 1 else 1 - S
    assert ((lo <= shift) & (shift < S)).all()
    return dist, shift


@pytest.mark.parametrize("geom", G.GEOMETRIES, ids=_gid)
def test_distance_bit_identical_to_oracle(geom):
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    R, S, rmax = geom
    D = np.stack(_distance_set(R, S, rmax, 60))
    n = D.shape[0]
    pairs = [(q, c) for q in range(n) for c in range(n)] if S <= 128 else \
        [(0, c) for c in range(n)] + [(q, q) for q in range(1, n)] + [(5, 6), (8, 9), (9, 8), (4, 0), (10, 0)]
    ratios = list(G.RATIOS)
    if (R, S) == (40, 120):
        # search spaces just below and just above one similarity chunk
        m = max(m for m in range(1, 2 * S + 2, 2) if G.distance_layout(R, S, G.ratio_for_m(S, m))[1] >= m)
        assert G.distance_layout(R, S, G.ratio_for_m(S, m + 2))[1] < m + 2
        ratios += [G.ratio_for_m(S, m), G.ratio_for_m(S, m + 2), -0.3]
    for ratio in ratios:
        if not G.distance_layout(R, S, ratio)[2]:
            with pytest.raises(L.CfearError) as e:
                api.sc_distance_batch(D, D, pairs[:1], _par(R, S, rmax, search_ratio=ratio))
            assert e.value.status == L.ERR_CAPACITY
            continue
        dist, shift = _check_distances(D, R, S, ratio, pairs)
        if (R, S) == (40, 120) and ratio == 2.5:
            assert (shift < 0).any()                                   # the negative shifts are exercised
        rot = pairs.index((0, 1))
        assert dist[rot] < 1e-12                                       # a rotated copy of itself
        if R > 1 and S > 1:                                            # (one ring: every shift ties at 0)
            assert shift[rot] == S // 7 + 1
        assert dist[pairs.index((5, 6))] == 1.0                       # two all-empty descriptors: no column counted


def test_distance_refuses_shapes_beyond_its_lds_and_non_finite_ratios():
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    D = np.zeros((1, 1, 8))
    for kw, status in [(dict(num_ring=2, num_sector=2560), L.ERR_CAPACITY), (dict(num_ring=1, num_sector=5120), L.ERR_CAPACITY),
                       (dict(num_ring=1, num_sector=G.S_MAX + 1), L.ERR_CAPACITY),
                       (dict(num_ring=41, num_sector=125), L.ERR_CAPACITY), (dict(num_ring=0), L.ERR_CAPACITY),
                       (dict(search_ratio=float("nan")), L.ERR_INVALID_ARGUMENT),
                       (dict(search_ratio=float("inf")), L.ERR_INVALID_ARGUMENT),
                       (dict(search_ratio=-float("inf")), L.ERR_INVALID_ARGUMENT),
                       (dict(search_ratio=1e300), L.ERR_CAPACITY)]:
        par = api.sc_params(**kw)
        R, S = par.num_ring, par.num_sector
        for call in (lambda: api.sc_distance_batch(np.zeros((1, max(R, 1), S)), np.zeros((1, max(R, 1), S)), [(0, 0)], par),
                     lambda: api.sc_descriptors([np.zeros((0, 4), np.float32)], par),
                     lambda: api.RSCManagerNative(par=par)):
            with pytest.raises(L.CfearError) as e:
                call()
            assert e.value.status == status, (kw, e.value.status)
    # the largest accepted shape works
    par = api.sc_params(num_ring=1, num_sector=G.S_MAX)
    D = np.abs(np.random.default_rng(1).normal(size=(2, 1, G.S_MAX)))
    _check_distances(D, 1, G.S_MAX, 0.1, [(0, 1), (1, 0)])
    assert api.sc_descriptors([G.random_cloud(1, 1, G.S_MAX, 80.0)], par)[0].shape == (1, 1, 1, G.S_MAX)


# ---- raw sweeps ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,S", [(20, 60), (64, 80), (40, 128), (1, 120)])
def test_raw_sweeps_at_other_geometries(R, S):
    from tests import sc_raw_cpu as X
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(R * 1000 + S)
    paths = set()
    for shape in ((400, 3360), (400, 3768)):
        imgs = rng.integers(0, 256, (2,) + shape, dtype=np.uint8)
        imgs[1] = np.minimum(imgs[1], 70)
        for transpose in (0, 1):
            H, W = (shape[1], shape[0]) if transpose else shape
            paths.add(X.resize_path(H, W, R, S))
            par = api.sc_params(num_ring=R, num_sector=S)
            d, rk, sk = api.sc_raw_descriptors(imgs, par, api.sc_raw_params(transpose=transpose))
            for b in range(2):
                e, erk, esk = X.raw_descriptor(imgs[b], R, S, 0.0, bool(transpose))
                np.testing.assert_array_equal(d[b], e, err_msg="%s transpose %d sweep %d" % (shape, transpose, b))
                np.testing.assert_array_equal(rk[b], erk)
                np.testing.assert_array_equal(sk[b], esk)
    assert "general" in paths
    from tbv_slam_public_amd import _lib as L
    with pytest.raises(L.CfearError) as e:                            # 64 x 100 = 6400 cells: past the capacity
        api.sc_raw_descriptors(imgs, api.sc_params(num_ring=64, num_sector=100))
    assert e.value.status == L.ERR_CAPACITY
