"""GPU: raw-sweep Scan Context (cfear_sc_raw_descriptors, sc_raw_descriptor_kernel) bit-exact against the NumPy
restatement tests/sc_raw_cpu.py -- descriptors, ring keys and sector keys -- over shapes, both orientations, strides,
thresholds, batches and host / device memory; and the raw path of both RSCManagers."""
import numpy as np
import pytest

from tests import sc_raw_cpu as X

pytestmark = pytest.mark.gpu


def _check(imgs, R=40, S=120, thr=0.0, transpose=None, got=None):
    """imgs: uint8 [B, H, W] stored sweeps; got = (desc, rk, sk) from the library."""
    d, rk, sk = got
    d = d.cpu().numpy() if hasattr(d, "cpu") else d
    for b in range(imgs.shape[0]):
        e, erk, esk = X.raw_descriptor(imgs[b], R, S, thr, transpose)
        np.testing.assert_array_equal(d[b], e, err_msg="sweep %d" % b)
        np.testing.assert_array_equal(rk[b], erk)
        np.testing.assert_array_equal(sk[b], esk)


def _scene_sweeps(n, seed=3, cols=3360):
    from tbv_slam_public_amd import synth
    sc = synth.Scene(seed, cols=cols)
    return np.stack([sc.render(f, n) for f in range(n)])


@pytest.mark.parametrize("shape", [(400, 3360), (400, 3768), (3360, 400)])
@pytest.mark.parametrize("transpose", [0, 1])
def test_shapes_and_orientations(shape, transpose):
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(sum(shape) + transpose)
    imgs = rng.integers(0, 256, (3,) + shape, dtype=np.uint8)
    imgs[1] = np.minimum(imgs[1], 90)                                 # a darker sweep
    raw = api.sc_raw_params(transpose=transpose)
    _check(imgs, transpose=bool(transpose), got=api.sc_raw_descriptors(imgs, raw=raw))


def test_rendered_oxford_sweeps_default_orientation():
    from tbv_slam_public_amd import api
    imgs = _scene_sweeps(4)
    _check(imgs, got=api.sc_raw_descriptors(imgs))                     # H < W: read transposed, the reader's rule
    one = api.sc_raw_descriptors(imgs[2])
    assert one[0].shape == (40, 120) and one[1].shape == (40,) and one[2].shape == (120,)
    np.testing.assert_array_equal(one[0], X.raw_descriptor(imgs[2])[0])


@pytest.mark.parametrize("thr", [-1.0, 0.0, 64.5, 255.0])
def test_thresholds(thr):
    from tbv_slam_public_amd import api
    imgs = _scene_sweeps(2, seed=5)
    _check(imgs, thr=thr, got=api.sc_raw_descriptors(imgs, raw=api.sc_raw_params(radar_threshold=thr)))
    assert imgs[0].max() > 64                                          # the caller's sweep is not thresholded in place


@pytest.mark.parametrize("pad", [1, 5, 13, 16])
@pytest.mark.parametrize("transpose", [0, 1])
def test_odd_strides_and_batch_stride(pad, transpose):
    import torch
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(pad)
    big = rng.integers(0, 256, (3, 400 + 1, 3768 + pad), dtype=np.uint8)   # an extra row: batch_stride > rows * stride
    view = big[:, :400, :3768]
    raw = api.sc_raw_params(transpose=transpose)
    want = api.sc_raw_descriptors(np.ascontiguousarray(view), raw=raw)
    _check(np.ascontiguousarray(view), transpose=bool(transpose), got=want)
    host = api.sc_raw_descriptors(view, raw=raw)
    dev = api.sc_raw_descriptors(torch.from_numpy(big).cuda()[:, :400, :3768], raw=raw)
    for a, b, c in zip(want, host, dev):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("shape,R,S", [((3, 4), 1, 3), ((3, 4), 3, 3), ((7, 15), 3, 4), ((7, 15), 2, 5),
                                       ((15, 7), 5, 3), ((4, 3), 2, 3), ((9, 6), 3, 2)])
def test_tiny_images(shape, R, S):
    """Images of fewer than 16 bins: the tail piece of every row is read byte by byte or whole only where it ends inside
    the image; device images are allocated to the exact byte count."""
    import torch
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(R * 100 + S)
    for transpose in (0, 1):
        H, W = (shape[1], shape[0]) if transpose else shape
        if H < R or W < S:
            continue
        try:
            X.resize_path(H, W, R, S)
        except X.Refused:
            continue
        imgs = rng.integers(0, 256, (2,) + shape, dtype=np.uint8)
        par = api.sc_params(num_ring=R, num_sector=S)
        raw = api.sc_raw_params(transpose=transpose)
        got = api.sc_raw_descriptors(imgs, par, raw)
        _check(imgs, R, S, transpose=bool(transpose), got=got)
        flat = torch.from_numpy(imgs.reshape(-1)).cuda()                  # exactly 2 * H * W bytes
        dev = api.sc_raw_descriptors(flat.view(imgs.shape), par, raw, device_out=True)
        np.testing.assert_array_equal(dev[0].cpu().numpy(), got[0])


def test_fast_path_and_general_path_on_the_gpu():
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(11)
    fast = rng.integers(0, 256, (2, 360, 3360), dtype=np.uint8)        # 360 -> 120 = 3, 3360 -> 40 = 84: integer scales
    assert X.resize_path(3360, 360, 40, 120) == "fast"
    _check(fast, got=api.sc_raw_descriptors(fast))
    ties = np.zeros((1, 3, 8), np.uint8)                               # 3 x 4 boxes: 30 * (1.f / 12) = 2.5f -> 2
    ties[0, 0, :3] = 10
    ties[0, 1, 4:7] = 14                                               # 42 * (1.f / 12) = 3.5f -> 4
    par = api.sc_params(num_ring=1, num_sector=2)
    got = api.sc_raw_descriptors(ties, par, api.sc_raw_params(transpose=0))
    _check(ties, 1, 2, transpose=False, got=got)
    np.testing.assert_array_equal(got[0][0], [[2.0, 4.0]])


def test_batch_of_512_host_and_device():
    import torch
    from tbv_slam_public_amd import api
    base = _scene_sweeps(4, seed=9)
    rng = np.random.default_rng(2)
    imgs = np.concatenate([base, rng.integers(0, 256, (508, 400, 3360), dtype=np.uint8)])
    host = api.sc_raw_descriptors(imgs)
    for b in list(range(6)) + [255, 511]:
        e, erk, esk = X.raw_descriptor(imgs[b])
        np.testing.assert_array_equal(host[0][b], e)
        np.testing.assert_array_equal(host[1][b], erk)
        np.testing.assert_array_equal(host[2][b], esk)
    d = torch.from_numpy(imgs).cuda()
    dev = api.sc_raw_descriptors(d, device_out=True)
    assert dev[0].is_cuda
    np.testing.assert_array_equal(dev[0].cpu().numpy(), host[0])
    np.testing.assert_array_equal(dev[1], host[1])
    np.testing.assert_array_equal(api.sc_raw_descriptors(d)[0], host[0])            # device in, host out
    np.testing.assert_array_equal(api.sc_raw_descriptors(imgs, device_out=True)[0].cpu().numpy(), host[0])


def test_errors_leave_the_context_usable():
    from tbv_slam_public_amd import _lib as L
    from tbv_slam_public_amd import api
    imgs = _scene_sweeps(1)
    ok = api.sc_raw_descriptors(imgs)
    for raw, par, img in [(api.sc_raw_params(normalize=1), None, imgs),
                          (api.sc_raw_params(interpolation="bilinear"), None, imgs),
                          (api.sc_raw_params(radar_threshold=float("nan")), None, imgs),
                          (api.sc_raw_params(transpose=0), api.sc_params(num_ring=4, num_sector=4), np.zeros((1, 8, 8), np.uint8)),
                          (api.sc_raw_params(transpose=0), None, np.zeros((1, 3, 4), np.uint8))]:
        with pytest.raises(L.CfearError) as e:
            api.sc_raw_descriptors(img, par, raw)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
    again = api.sc_raw_descriptors(imgs)
    for a, b in zip(ok, again):
        np.testing.assert_array_equal(a, b)


def test_rotation_is_a_column_shift():
    from tbv_slam_public_amd import api
    img = _scene_sweeps(1, seed=4)[0]
    rolled = np.roll(img, 10, axis=0)                                  # 10 azimuths = 3 sectors
    a = api.sc_raw_descriptors(img)[0]
    b = api.sc_raw_descriptors(rolled)[0]
    np.testing.assert_array_equal(np.roll(a, 3, axis=1), b)
    dist, shift = api.sc_distance_batch(b[None], a[None], [(0, 0)])
    assert dist[0] < 1e-6 and shift[0] == 3                            # query rolled forward: the candidate shifts by 3
    d, s = api.sc_distance_batch(a[None], b[None], [(0, 0)])
    assert d[0] < 1e-6 and s[0] == 117                                 # and -3 the other way round


def _lap_sweeps():
    """A synthetic lap: 14 keyframes 5 m apart, then the sweep of keyframe 2 seen again (revisit, new speckle) at its pose."""
    from tbv_slam_public_amd import synth
    sc = synth.Scene(17)
    n = 14
    imgs = [sc.render(f * 2, 2 * n) for f in range(n)]
    poses = [sc.pose_at(f * 2, 2 * n) for f in range(n)]
    rng = np.random.default_rng(0)
    revisit = np.clip(imgs[2].astype(int) + rng.integers(-3, 4, imgs[2].shape), 0, 255).astype(np.uint8)
    return imgs + [revisit], poses + [poses[2]]


@pytest.mark.parametrize("odom_coupled", [True, False])
def test_native_and_python_managers_agree_and_find_the_loop(odom_coupled):
    from tbv_slam_public_amd import api
    imgs, poses = _lap_sweeps()
    py = api.RSCManager(odometry_coupled_closure=odom_coupled)
    nat = api.RSCManagerNative(odometry_coupled_closure=odom_coupled)
    found = False
    for i, (img, T) in enumerate(zip(imgs, poses)):
        py.makeAndSaveScancontextAndKeysRadarRaw(img, T)
        nat.makeAndSaveScancontextAndKeysRadarRaw(img, T)
        a, b = py.detectLoopClosureID(), nat.detectLoopClosureID()
        assert len(a) == len(b), i
        for x, y in zip(a, b):
            assert x["nn_idx"] == y["nn_idx"] and x["argmin_shift"] == y["argmin_shift"], (i, x, y)
            assert x["min_dist"] == y["min_dist"] and x["min_dist_sc"] == y["min_dist_sc"], (i, x, y)
            assert tuple(x["Taug"]) == tuple(y["Taug"]) == (0.0, 0.0, 0.0)
        if i == len(imgs) - 1:
            found = any(c["nn_idx"] == 2 for c in a)
    # the odometry-coupled search finds it; the vanilla kd-tree is first rebuilt at its 50th call (empty until then)
    assert found or not odom_coupled, "the revisit of keyframe 2 was not proposed"
    assert nat.size() == len(imgs)
    nat.close()


def test_raw_and_cloud_nodes_share_one_database():
    from tbv_slam_public_amd import api
    from tests.test_oracle_coral import _peaks
    clouds, _ = _peaks(20, [0, 1], k=12)
    imgs = _scene_sweeps(2, seed=6)
    for m in (api.RSCManager(), api.RSCManagerNative()):
        m.makeAndSaveScancontextAndKeysRadarCloud(clouds[0], (0.0, 0.0, 0.0))
        assert len(getattr(m, "current_and_augments_", [0] * 5)) == 5
        m.makeAndSaveScancontextAndKeysRadarRaw(imgs[0], (1.0, 0.0, 0.0))
        m.makeAndSaveScancontextAndKeysRadarCloud(clouds[1], (2.0, 0.0, 0.0))
        m.makeAndSaveScancontextAndKeysRadarRaw(imgs[1], (3.0, 0.0, 0.0))
        m.detectLoopClosureID()
        if isinstance(m, api.RSCManagerNative):
            assert m.size() == 4
            m.close()
        else:
            assert len(m.polarcontexts_) == 4
