"""CPU: the route tests' inputs stay on the branches they are there for.  tests/surface_routes.predict restates the surface
kernels' thresholds; here every case of the GPU route matrix is checked against the features it names, the order-sensitive
fixture proves (on the oracle) that it sees the in-voxel order on every route's padding, and the run-length fixture that it
covers every length at every offset -- so none of the GPU cases can go blind without a GPU noticing."""
import numpy as np
import pytest

from tests import surface_routes as R
from tests import test_gpu_surface_routes as G


@pytest.mark.parametrize("name", sorted(G.MATRIX))
def test_matrix_case_is_predicted_on_its_branch(name):
    build, factor, rot, feats = G.MATRIX[name]
    cloud = build()
    path = R.predict(cloud, 3.0, factor, rot)
    assert path is not None
    for f in feats:
        assert R.FEATURES[f](path), (f, R.describe(path))
    np.testing.assert_array_equal(cloud, build())                      # seeded: the same cloud every time


def test_matrix_predictions_cover_every_route_bit():
    seen = {f for build, factor, rot, _ in G.MATRIX.values() for f, hit in R.FEATURES.items() if hit(R.predict(build(), 3.0, factor, rot))}
    assert seen >= set(R.FEATURES) - {"rows"}, sorted(set(R.FEATURES) - seen)


def test_tier_edges_sit_on_both_sides_of_every_threshold():
    tiers = {c: R.predict(G._tier(c)) & (R.TIER16 | R.TIER4 | R.TIER1) for c in (5, 6, 16, 17, 64, 65)}
    assert tiers == {5: 0, 6: R.TIER1, 16: R.TIER1, 17: R.TIER4, 64: R.TIER4, 65: R.TIER16}


@pytest.mark.parametrize("route", sorted(G.ORDER_PADS))
def test_order_fixture_sees_the_order_on_every_route(route):
    pad, feats = G.ORDER_PADS[route]
    cloud = R.order_blocks(40, pad())                                  # asserts >= 5 cells change when the cloud is reversed
    path = R.predict(cloud)
    for f in feats:
        assert R.FEATURES[f](path), (f, R.describe(path))


def test_run_length_fixture_covers_every_offset():
    cloud = R.run_lengths(41)                                          # asserts the coverage itself
    assert R.predict(cloud) & R.KIND_MASK == R.FAST


@pytest.mark.parametrize("name", sorted(G.EDGES) + sorted(G.COMPENSATED))
def test_edge_and_compensation_cases_are_accepted(name):
    if name in G.EDGES:
        assert R.predict(G.EDGES[name]()) is not None
    else:
        from oracle import pyoracle as O
        build, factor, feats = G.COMPENSATED[name]
        path = R.predict(O.compensate(build(), G.MOT, False), 3.0, factor, G.MOT[2])
        for f in feats:
            assert R.FEATURES[f](path), (f, R.describe(path))
