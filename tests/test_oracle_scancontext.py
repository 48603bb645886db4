"""CPU: the oracle's radar Scan Context (RadarScancontext.cpp:59-131, Scancontext.cpp:60-268) against a NumPy
restatement written from the paper-level definition: polar binning with ceil indices, np.roll column
shifts, cosine distance over non-empty columns."""
import numpy as np
import pytest

from tests import sc_geometry as G


def _cloud(seed, n=3000):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 4), np.float32)
    r = rng.uniform(1, 100, n)
    a = rng.uniform(0, 2 * np.pi, n)
    c[:, 0], c[:, 1] = r * np.cos(a), r * np.sin(a)
    c[:, 3] = rng.integers(60, 256, n)
    c[0, :2] = (0, 5); c[1, :2] = (-7, 0); c[2, :2] = (0, -3); c[3, :2] = (80, 0); c[4, :2] = (0, 0)   # axes, rim, origin
    return c


def _numpy_theta(c, dy=0.0):
    x = c[:, 0].astype(np.float32)
    y = (c[:, 1].astype(np.float64) + dy).astype(np.float32) if dy else c[:, 1].astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0).astype(np.float32)


def _numpy_desc(c, R=40, S=120, rmax=80.0, fn="sum", div=1000.0, no_point=0.0, dy=0.0):
    x = c[:, 0].astype(np.float32)
    y = (c[:, 1].astype(np.float64) + dy).astype(np.float32) if dy else c[:, 1].astype(np.float32)
    rng_ = np.sqrt(x * x + y * y).astype(np.float32)
    th = _numpy_theta(c, dy)
    keep = ~(rng_.astype(np.float64) > rmax)
    ring = np.clip(np.ceil(rng_.astype(np.float64) / rmax * R).astype(int), 1, R) - 1
    sec = np.clip(np.ceil(th.astype(np.float64) / 360.0 * S).astype(int), 1, S) - 1
    desc = np.full((R, S), -1000.0)
    for k in np.nonzero(keep)[0]:
        v = float(c[k, 3])
        if desc[ring[k], sec[k]] == -1000.0:
            desc[ring[k], sec[k]] = v
        elif fn == "sum":
            desc[ring[k], sec[k]] += v
        else:
            desc[ring[k], sec[k]] = max(desc[ring[k], sec[k]], v)
    desc = desc / div
    desc[desc == -1000.0] = no_point
    return desc, ring, sec, keep


def _numpy_dist(a, b, ratio=0.1):
    S = a.shape[1]
    v1, v2 = a.mean(0), b.mean(0)
    norms = [np.linalg.norm(v1 - np.roll(v2, sh)) for sh in range(S)]
    sh0 = int(np.argmin(norms))
    x = 0.5 * ratio * S
    rad = int(np.floor(abs(x) + 0.5) * np.sign(x))             # std::round: half away from zero
    # the reference keeps duplicated shifts (search_ratio > 1 wraps around the circle), and its C++ % leaves
    # sh0 - i + S negative once i > sh0 + S (search_ratio > 2): such a shift is applied modulo S and reported as it is
    cmod = lambda a: int(np.fmod(a, S))                        # noqa: E731
    space = sorted([sh0] + [cmod(sh0 + i + S) for i in range(1, rad + 1)] + [cmod(sh0 - i + S) for i in range(1, rad + 1)])
    best, arg = 1e7, 0
    for sh in space:
        bs = np.roll(b, sh, axis=1)
        n1, n2 = np.linalg.norm(a, axis=0), np.linalg.norm(bs, axis=0)
        ok = (n1 != 0) & (n2 != 0)
        sim = ((a * bs).sum(0)[ok] / (n1[ok] * n2[ok])).sum() / max(int(ok.sum()), 1)
        if 1 - sim < best:
            best, arg = 1 - sim, sh
    return best, arg


@pytest.mark.parametrize("fn,div,dy", [("sum", 1000.0, 0.0), ("max", 1.0, 0.0), ("sum", 1000.0, -4.0), ("sum", 1.0, 2.0)])
def test_descriptor_matches_numpy(fn, div, dy):
    from oracle import pyoracle as O
    c = _cloud(1)
    d = O.sc_descriptor(c, desc_function=fn, desc_divider=div, no_point=0.0, shift_y=dy)
    e, ring, sec, keep = _numpy_desc(c, fn=fn, div=div, dy=dy)
    # float atan (reference) vs double atan2 may disagree on a point that sits within an ulp of a sector edge
    bad = np.abs(d - e) > 1e-12
    assert bad.sum() <= 4
    if div == 1000.0:
        assert (d[e == -1.0] == -1.0).all()        # empty bins keep NO_POINT / divider ("division before the check")
    else:
        assert (d[e == 0.0] == 0.0).all()
    rk, sk = O.sc_keys(d)
    np.testing.assert_allclose(rk, d.mean(1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(sk, d.mean(0), rtol=1e-12, atol=1e-15)


def test_axis_points_and_rim():
    from oracle import pyoracle as O
    c = _cloud(2)[:5].copy()
    c[:, 3] = [10, 20, 30, 40, 50]
    d = O.sc_descriptor(c, desc_function="sum", desc_divider=1.0, no_point=0.0)
    assert d[2, 29] == 20 + 0 or d[2, 29] == 10        # (0, 5): range 5 -> ring 3, angle 90 deg -> sector 30
    assert d[3, 59] == 20                              # (-7, 0): 180 deg -> sector 60
    assert d[1, 89] == 30                              # (0, -3): 270 deg -> sector 90
    assert d[39, 0] == 40                              # (80, 0): on the rim, angle 0 -> sector 1 (max(.,1))
    assert d.sum() == 10 + 20 + 30 + 40 + 50           # the origin lands in ring 1, sector 1


@pytest.mark.parametrize("shift", [0, 7, 61, 119])
def test_distance_recovers_rotation(shift):
    from oracle import pyoracle as O
    a = O.sc_descriptor(_cloud(3), desc_divider=1000.0)
    b = np.roll(a, -shift, axis=1)                      # the same place seen with a heading change
    d, sh = O.sc_distance(a, b)
    e, esh = _numpy_dist(a, b)
    assert sh == esh == shift
    np.testing.assert_allclose(d, e, rtol=1e-9, atol=1e-12)
    assert d < 1e-9
    other = O.sc_descriptor(_cloud(4), desc_divider=1000.0)
    d2, sh2 = O.sc_distance(a, other)
    e2, esh2 = _numpy_dist(a, other)
    assert sh2 == esh2
    np.testing.assert_allclose(d2, e2, rtol=1e-9)
    assert d2 > 0.2


# ---- the geometry grid (tests/sc_geometry.py): the oracle is the GPU tests' ground truth there --------------------------

def _gid(g):
    return "%dx%d_r%g" % g


@pytest.mark.parametrize("geom", G.GEOMETRIES, ids=_gid)
@pytest.mark.parametrize("fn,div,dy", [("sum", 1000.0, 0.0), ("max", 1.0, 2.0), ("sum", 1.0, -4.0)])
def test_descriptor_matches_numpy_on_the_grid(geom, fn, div, dy):
    """Exact on every cell once the points the two angle definitions put on different sides of a sector edge are removed:
    the paper-level double atan2 and the reference's float atan differ by a few float ulps, so such points must lie within
    1e-4 sectors of an edge."""
    from oracle import pyoracle as O
    R, S, rmax = geom
    c = G.random_cloud(7, R, S, rmax)
    _, ring, sec, keep = _numpy_desc(c, R, S, rmax, fn, div, -7.5, dy)
    oring, osec = O.sc_bins(c, R, S, rmax, dy)
    kept = oring >= 0
    np.testing.assert_array_equal(kept, keep)
    np.testing.assert_array_equal(oring[kept], ring[kept])
    split = kept & (osec != sec)
    pos = _numpy_theta(c, dy).astype(np.float64) / 360.0 * S
    assert (np.abs(pos[split] - np.round(pos[split])) < 1e-4).all()
    assert split.sum() <= 3
    c = c[~split]
    d = O.sc_descriptor(c, R, S, rmax, fn, div, -7.5, dy)
    e = _numpy_desc(c, R, S, rmax, fn, div, -7.5, dy)[0]
    np.testing.assert_array_equal(d, e)
    rk, sk = O.sc_keys(d)
    np.testing.assert_allclose(rk, d.mean(1), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(sk, d.mean(0), rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("geom", G.GEOMETRIES, ids=_gid)
def test_edge_cloud_bins(geom):
    """The edge cloud of the GPU tests: the oracle bins it like the correctly rounded restatement, keeps the rim, drops
    the next float past it and non-finite ranges, and puts NaN ranges / the origin into the first bin."""
    from oracle import pyoracle as O
    R, S, rmax = geom
    c = G.edge_cloud(R, S, rmax)
    ring, sec = O.sc_bins(c, R, S, rmax)
    kr, ks = G.kernel_bins(c, R, S, rmax)
    np.testing.assert_array_equal(ring, kr)
    np.testing.assert_array_equal(sec, ks)
    x, y = c[:, 0], c[:, 1]
    assert (ring[(x == np.float32(rmax)) & (y == 0)] == R - 1).all()
    assert (ring[np.abs(x) == np.nextafter(np.float32(rmax), np.float32(np.inf))] == -1).all()
    nan = np.isnan(x) | np.isnan(y)                                # a NaN range is not > max_radius: kept
    assert (ring[(np.isinf(x) | np.isinf(y)) & ~nan] == -1).all()
    assert (ring[nan] == 0).all() and (sec[nan] == 0).all()
    assert ring[0] == 0 and sec[0] == 0
    for k in range(1, R + 1):                                      # a point exactly on ring edge k: ring k (ceil)
        e = np.float32(k * rmax / R)
        if float(e) / rmax * R == k:
            assert ring[(x == e) & (y == 0)][0] == k - 1


@pytest.mark.parametrize("geom", G.GEOMETRIES, ids=_gid)
def test_distance_matches_numpy_on_the_grid(geom):
    """Random places and rotated copies at every ratio of the GPU grid, duplicated shifts included (ratio > 1)."""
    from oracle import pyoracle as O
    R, S, rmax = geom
    a = O.sc_descriptor(G.random_cloud(11, R, S, rmax), R, S, rmax)
    b = O.sc_descriptor(G.random_cloud(12, R, S, rmax), R, S, rmax, "max", 1.0)
    rot = (S // 7 + 1) % S
    for ratio in G.RATIOS + ((-0.3,) if S == 120 else ()):
        if not G.distance_layout(R, S, ratio)[2] and S > 2048:
            continue                                               # refused by the library; the oracle is not needed there
        for q, c in ((a, np.roll(a, -rot, axis=1)), (a, b), (b, a)):
            d, sh = O.sc_distance(q, c, ratio)
            e, esh = _numpy_dist(q, c, ratio)
            assert sh == esh, (ratio, sh, esh)
            np.testing.assert_allclose(d, e, rtol=1e-9, atol=1e-12)
        if R > 1:                                                  # one ring: every column's cosine is 1, all shifts tie
            assert O.sc_distance(a, np.roll(a, -rot, axis=1), ratio)[1] == rot


def test_distance_layout_limits():
    """The shapes the library's distance kernel accepts (tests/sc_geometry.py mirrors scancontext.hip's layout)."""
    assert max(S for S in range(1, 5121) if G.distance_layout(1, S, 0.1)[2]) == G.S_MAX
    assert all(G.distance_layout(R, S, 2.5)[2] for R, S, _ in G.GEOMETRIES if S <= 2048)
    assert not G.distance_layout(2, 2560, 0.0)[2] and not G.distance_layout(1, 5120, 0.0)[2]
    assert G.search_space_size(120, 2.5) == 301 > 2 * 120 + 2     # more shifts than S: duplicates
    assert G.search_space_size(120, -1.0) == 1 and G.search_space_size(3, 1.0) == 5    # round(1.5) = 2, away from zero
