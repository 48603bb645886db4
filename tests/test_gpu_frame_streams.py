"""GPU: the small copies of a frame batch run on the fuser's copy stream, ordered against the kernel stream by events
(odometry.hip): the surface job table and the image-offset table go up while kernels run, the result block comes down while
the next sweep runs.  A stale offset table, a job table that arrives late or a result block read early each change what a
frame reports, so every way of feeding the same frames must report the same, field for field.

Three streams, a ring of four distinct sweeps per stream, eight frames: both filter buffers are used four times, the
four-keyframe window fills and passes its first eviction.  The vehicle drives 0.5 m per sweep and the keyframe distance is
0.25 m, so every frame becomes a keyframe -- also the one that steps back from the ring's last sweep to its first.

Every case runs on both kinds of kernel stream a context can have: one of the runtime's stream handles (the default context
enqueues on torch's null stream) and a stream object of the context's own.  Only behind a stream object does the result
block come down on the copy stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, RING, FRAMES = 3, 4, 8
IMG = 400 * 3360
SLOT = IMG + 4096                                   # gaps between the images of the ring
PAR = dict(min_keyframe_dist=0.25)
POS_TOL, ROT_TOL = 1e-4, 1e-5                       # BASELINE.json: pose against the CPU path, per frame

_cache = {}
KINDS = ("handle", "stream")


def _ctx(kind):
    import torch
    from tbv_slam_public_amd import api
    _frames()
    if kind == "handle":
        return api.default_context()
    if "ctx" not in _cache:
        torch.cuda.synchronize()                    # a stream of its own is not ordered behind torch's: the frames must exist
        _cache["ctx"] = api.Context(0)
    return _cache["ctx"]


def _frames():
    """sweeps [B][RING][400][3360], the device ring that holds them in shuffled slots, offsets [B][RING]"""
    if not _cache:
        import torch
        from tbv_slam_public_amd import synth
        seqs = np.stack([synth.scene_v1(60 + b, RING, speed=2.0)[0] for b in range(B)])
        order = np.random.default_rng(1).permutation(B * RING)
        ring = torch.zeros(B * RING * SLOT, dtype=torch.uint8, device="cuda")
        off = np.zeros((B, RING), np.int64)
        for b in range(B):
            for f in range(RING):
                off[b, f] = int(order[b * RING + f]) * SLOT
                ring[off[b, f]:off[b, f] + IMG] = torch.from_numpy(seqs[b, f].reshape(-1)).cuda()
        dev = [torch.from_numpy(np.ascontiguousarray(seqs[:, f])).cuda() for f in range(RING)]
        torch.cuda.synchronize()
        _cache.update(seqs=seqs, ring=ring, off=off, dev=dev)
    return _cache


def _plain():
    """the reference of this file, computed once: the strided entry, one frame per call, no prefetch"""
    if "plain" not in _cache:
        from tbv_slam_public_amd import api
        fr = _frames()
        od = api.OdometryKeyframeFuser(B, 400, 3360, api.odometry_params(**PAR))
        _cache["plain"] = [od.process(fr["dev"][t % RING]).copy() for t in range(FRAMES)]
        od.close()
        last = _cache["plain"][-1]
        assert (last["reg_status"] == 0).all()
        # the window of four keyframes filled and evicted: the first frame and at least four more became keyframes
        added = sum(i["keyframe_added"].astype(int) for i in _cache["plain"])
        assert (added >= 5).all(), added
    return _cache["plain"]


def _same(got, t):
    exp = _plain()[t]
    for name in exp.dtype.names:
        np.testing.assert_array_equal(got[name], exp[name], err_msg="%s frame %d" % (name, t))


def test_the_ring_differs_from_frame_to_frame_and_stream_to_stream():
    fr = _frames()
    assert len(set(fr["off"].reshape(-1).tolist())) == B * RING
    for t in range(FRAMES):                          # no frame could pass with its neighbour's offsets
        assert (fr["off"][:, t % RING] != fr["off"][:, (t + 1) % RING]).all()
    info = _plain()
    for t in range(1, FRAMES):
        assert (info[t]["pose"] != info[t - 1]["pose"]).any(axis=1).all()
        assert len({tuple(p) for p in info[t]["pose"]}) == B


@pytest.mark.parametrize("kind", KINDS)
def test_prefetched_offsets_equal_the_plain_path(kind):
    from tbv_slam_public_amd import api
    fr = _frames()
    od = api.OdometryKeyframeFuser(B, 400, 3360, api.odometry_params(**PAR), ctx=_ctx(kind))
    for t in range(FRAMES):
        nxt = fr["off"][:, (t + 1) % RING] if t + 1 < FRAMES else None
        _same(od.process_offsets(fr["ring"], fr["off"][:, t % RING], nxt), t)
    od.close()


@pytest.mark.parametrize("kind", KINDS)
def test_offsets_without_a_prefetch_on_every_second_frame(kind):
    from tbv_slam_public_amd import api
    fr = _frames()
    od = api.OdometryKeyframeFuser(B, 400, 3360, api.odometry_params(**PAR), ctx=_ctx(kind))
    for t in range(FRAMES):
        nxt = fr["off"][:, (t + 1) % RING] if (t + 1 < FRAMES and t % 2 == 0) else None
        _same(od.process_offsets(fr["ring"], fr["off"][:, t % RING], nxt), t)
    od.close()


def _oracle():
    """the CPU path over the same eight frames, once: per frame and stream (pose, info, points, peaks)"""
    if "oracle" not in _cache:
        from oracle import pyoracle as O
        from tbv_slam_public_amd import api
        fr = _frames()
        par = api.odometry_params(keep_nodes=1, **PAR)
        reg = O.reg_params(cost=par.reg.cost, loss=par.reg.loss, loss_limit=0.1, weight_opt=par.reg.weight_opt, regularization=0.0)
        fz = [O.Fuser(reg, res=par.res, submap_scan_size=par.submap_scan_size, weight_intensity=bool(par.weight_intensity),
                      min_keyframe_dist=PAR["min_keyframe_dist"]) for _ in range(B)]
        drv = api.radarDriver(api.radarDriverParameters(k_strongest=par.kstrong.k_strongest, z_min=int(par.kstrong.z_min),
                                                        range_res=par.kstrong.range_res))
        peaks = [[np.array(drv.CallbackOffline(fr["seqs"][b, f])[1]).shape[0] for f in range(RING)] for b in range(B)]
        out = []
        for t in range(FRAMES):
            row = []
            for b in range(B):
                sr, si, sc = O.kstrongest(fr["seqs"][b, t % RING], par.kstrong.k_strongest, par.kstrong.z_min)
                cloud = O.kstrongest_cloud(sr, si, sc, par.kstrong.range_res, 2.5)
                pose, info = fz[b].process(cloud)
                row.append((pose, info.copy(), cloud.shape[0], peaks[b][t % RING]))
            out.append(row)
        _cache["oracle"] = out
    return _cache["oracle"]


@pytest.mark.parametrize("kind", KINDS)
def test_keep_nodes_on_the_strided_entry_matches_the_oracle(kind):
    """keep_nodes = 1: the filter writes clouds and a peaks cloud, the point counts reach the result block through a device
    copy and the peak counts through a read-back of their own -- both ordered behind the frame's last kernel."""
    from tbv_slam_public_amd import api
    fr, exp = _frames(), _oracle()
    od = api.OdometryKeyframeFuser(B, 400, 3360, api.odometry_params(keep_nodes=1, **PAR), ctx=_ctx(kind))
    for t in range(FRAMES):
        nxt = fr["dev"][(t + 1) % RING] if (t + 1 < FRAMES and t % 3 != 2) else None
        info = od.process(fr["dev"][t % RING], nxt)
        for b in range(B):
            pose_o, info_o, npts_o, npk_o = exp[t][b]
            d = np.abs(info["pose"][b] - pose_o)
            print("frame %d stream %d: |dpose| %.3g %.3g %.3g" % (t, b, d[0], d[1], d[2]))
            assert info["n_points"][b] == npts_o, (t, b)
            assert info["n_cells"][b] == info_o[0], (t, b)
            assert info["keyframe_added"][b] == info_o[1], (t, b)
            if t > 0:
                assert (info["reg_status"][b] == 0) == bool(info_o[2]), (t, b)
                assert info["outer_iters"][b] == info_o[3], (t, b)
            assert d[:2].max() <= POS_TOL and d[2] <= ROT_TOL, (t, b, d)
            node = od.node(b)
            assert node["cloud"].shape == (npts_o, 4) and node["peaks"].shape[0] == npk_o, (t, b)
    od.close()
