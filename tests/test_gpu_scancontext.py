"""GPU: radar Scan Context descriptors, keys and column-shift distances through the C-ABI vs the CPU oracle,
and the RSCManager mirror (database + odometry-coupled candidate search) vs a restatement driven by the oracle.

Descriptor bins are sums of integer-valued intensities: bit-exact once the points within an ulp of a sector
edge, which float atan on the CPU and the correctly rounded one on the GPU put on different sides, are removed.
Distances use the oracle's summation order: bit-identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.sc_manager_ref import reference_manager_run   # noqa: E402
from tests.test_oracle_coral import _peaks   # noqa: E402


def _local_maps(seed, n_nodes, k=12):
    """Peak clouds of consecutive frames, each in its own frame (N_aggregate = 0 local maps)."""
    clouds, gt = _peaks(seed, list(range(n_nodes)), k=k)
    return clouds, gt


@pytest.mark.parametrize("fn,div", [("sum", 1000.0), ("max", 1.0), ("sum", 1.0)])
def test_descriptors_and_keys_match_oracle(fn, div):
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    from tests.sc_geometry import ambiguous
    clouds, _ = _local_maps(20, 3)
    par = api.sc_params(desc_function=fn, desc_divider=div)
    shifts = (0.0, -2.0, 2.0, -4.0, 4.0)
    # only the points whose sector depends on how atan rounds (CPU float atan vs the correctly rounded one) are removed
    clouds = [c[~np.any([ambiguous(c, 40, 120, 80.0, dy) for dy in shifts], axis=0)] for c in clouds]
    desc, rk, sk = api.sc_descriptors(clouds, par, shifts)
    assert desc.shape == (3, 5, 40, 120)
    for i, c in enumerate(clouds):
        for k, dy in enumerate(shifts):
            e = O.sc_descriptor(c, 40, 120, 80.0, fn, div, 0.0, dy)
            np.testing.assert_array_equal(desc[i, k], e, err_msg="cloud %d shift %g" % (i, dy))
            erk, esk = O.sc_keys(e)
            np.testing.assert_array_equal(rk[i, k], erk)
            np.testing.assert_array_equal(sk[i, k], esk)
    assert (desc[:, 0] != desc[:, 1]).any()                      # the augmentation moved points across bins


def test_device_clouds_and_empty_cloud():
    import torch
    from tbv_slam_public_amd import api
    clouds, _ = _local_maps(21, 2)
    host = api.sc_descriptors(clouds)[0]
    dev = api.sc_descriptors([torch.from_numpy(c).cuda() for c in clouds])[0]
    # descriptor database kept in HBM: same bits, and sc_distance_batch takes the device tensors as they are
    resident, rk_r, _ = api.sc_descriptors(clouds, device_out=True)
    assert resident.is_cuda and resident.dtype == torch.float64
    np.testing.assert_array_equal(resident.cpu().numpy(), host)
    np.testing.assert_array_equal(rk_r, api.sc_descriptors(clouds)[1])
    pairs = [(0, 1), (1, 0), (1, 1)]
    d_dev, s_dev = api.sc_distance_batch(resident[:, 0], resident[:, 0], pairs)
    d_host, s_host = api.sc_distance_batch(host[:, 0], host[:, 0], pairs)
    np.testing.assert_array_equal(d_dev, d_host)
    np.testing.assert_array_equal(s_dev, s_host)
    np.testing.assert_array_equal(host, dev)
    empty = api.sc_descriptors([np.zeros((0, 4), np.float32)])[0]
    assert (empty == -1.0).all()                                 # NO_POINT / 1000: "division before the check"


def test_distance_batch_bit_identical_to_oracle():
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    clouds, _ = _local_maps(22, 6)
    desc = api.sc_descriptors(clouds)[0][:, 0]
    rolled = np.stack([np.roll(desc[0], -17, axis=1), np.roll(desc[3], -101, axis=1)])
    cand = np.concatenate([desc, rolled])
    pairs = [(q, c) for q in range(6) for c in range(cand.shape[0])]
    dist, shift = api.sc_distance_batch(desc, cand, pairs)
    for (q, c), d, s in zip(pairs, dist, shift):
        ed, es = O.sc_distance(desc[q], cand[c])
        assert s == es and d == ed, (q, c, d, ed, s, es)
    assert shift[pairs.index((0, 6))] == 17 and dist[pairs.index((0, 6))] < 1e-12
    assert shift[pairs.index((3, 7))] == 101


@pytest.mark.parametrize("odom_coupled,augment", [(True, True), (False, False)])
def test_rsc_manager_finds_the_revisit(odom_coupled, augment):
    """A loop: 14 nodes driving away, then the first 4 places again (same clouds, rotated headings, odometry
    drifted by a few metres): the manager must propose the true revisits, exactly like the restatement."""
    from tbv_slam_public_amd import api
    clouds, gt = _local_maps(23, 14, k=12)
    seq_clouds = list(clouds)
    poses = [np.array([8.0 * i, 0.0, 0.0]) for i in range(14)]
    for j in range(4):                                   # revisit places 0..3 with a heading change of 90 degrees
        c = clouds[j].copy()
        x, y = c[:, 0].copy(), c[:, 1].copy()
        c[:, 0], c[:, 1] = y, -x                         # rotate the sensor by +90 deg
        seq_clouds.append(c)
        poses.append(np.array([8.0 * j + 2.0, 1.5, np.pi / 2]))
    mgr = api.RSCManager(odometry_coupled_closure=odom_coupled, augment_sc=augment)
    got = []
    for c, T in zip(seq_clouds, poses):
        mgr.makeAndSaveScancontextAndKeysRadarCloud(c, T)
        got.append(mgr.detectLoopClosureID())
    exp = reference_manager_run(seq_clouds, poses, odometry=odom_coupled, augment=augment)
    for g, e in zip(got, exp):
        assert [c["nn_idx"] for c in g] == [c[2] for c in e]
        np.testing.assert_allclose([c["min_dist"] for c in g], [c[0] for c in e], rtol=1e-12, atol=1e-15)
        assert [c["argmin_shift"] for c in g] == [c[3] for c in e]
    if not odom_coupled:
        # VanillaKDNNSearch asks a kd-tree that is rebuilt on every 50th call only (RadarScancontext.cpp:227): over these 18
        # calls it is the tree of the first searchable moment -- node 0 alone -- so every proposal is node 0 (the rest of the
        # zero-initialised index vector).  That IS the reference's behaviour on a short run; equality with the restatement
        # (which runs the reference's own nanoflann tree when oracle/_ref is built) is the assertion above.
        assert all(c["nn_idx"] == 0 for g in got for c in g)
        return
    for j in range(4):                                   # the revisits are found, with the 90 degree column shift
        best = got[14 + j][0]
        assert best["nn_idx"] == j and best["min_dist_sc"] < 0.15
        assert abs(best["argmin_shift"] - 30) <= 1 or abs(best["argmin_shift"] - 90) <= 1


def test_native_manager_equals_python_mirror_over_a_lap():
    """cfear_sc_manager (database in HBM, policy in the library's C++) against api.RSCManager (policy in Python, same
    kernels) over the 68 local maps of the synthetic lap: identical candidate lists, distances and guesses for every
    node, with and without the odometry coupling / the augmentations."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import loop_closure_demo as demo
    from oracle import pyoracle as O
    from tbv_slam_public_amd import api
    sc = demo.circle_scene()
    n = 68
    gt = np.stack([sc.pose_at(f, n) for f in range(n)])
    poses = np.array([demo.xyt_compose(demo.xyt_inverse(gt[0]), g) for g in gt])
    peaks = []
    for f in range(n):
        img = sc.render(f, n)
        sr, si, cnt = O.kstrongest(img, 40, 60)
        peaks.append(O.kstrongest_cloud(sr, si, cnt, 0.0438, 2.5, mask=O.peaks(img, 40, sr, cnt)))
    maps = []
    for i in range(n - 1):
        merged = [demo.transform_cloud(peaks[j], poses[j]) for j in (i - 1, i, i + 1) if 0 <= j < n]
        maps.append(demo.transform_cloud(np.concatenate(merged), demo.xyt_inverse(poses[i])))
    for kw in (dict(), dict(odometry_coupled_closure=False), dict(augment_sc=False, n_candidates=5)):
        py, nat = api.RSCManager(**kw), api.RSCManagerNative(**kw)
        found = 0
        for i, m in enumerate(maps):
            py.makeAndSaveScancontextAndKeysRadarCloud(m, poses[i])
            nat.makeAndSaveScancontextAndKeysRadarCloud(m, poses[i])
            a, b = py.detectLoopClosureID(), nat.detectLoopClosureID()
            assert [c["nn_idx"] for c in a] == [c["nn_idx"] for c in b], (kw, i)
            for ca, cb in zip(a, b):
                assert ca["argmin_shift"] == cb["argmin_shift"] and ca["yaw_diff_rad"] == cb["yaw_diff_rad"]
                assert ca["Taug"] == cb["Taug"]
                for f in ("min_dist", "min_dist_sc", "min_dist_odom"):
                    np.testing.assert_allclose(ca[f], cb[f], rtol=0, atol=1e-12)
            found += len(b)
        assert nat.size() == len(maps) and found > 100
        nat.close()
