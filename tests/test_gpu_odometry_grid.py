"""GPU: cfear_odometry_grid -- a parameter grid of odometry streams as one batch -- against one plain OdometryKeyframeFuser per
configuration: every cfear_frame_info of every stream and frame, byte for byte.  Nine configurations that between them vary
k, z_min, res, the cost, the loss, the weight option, the window, the intensity weights, compensation and the filter (one
CA-CFAR); two sequences of 400 x 3360 sweeps (the second at 1 m per frame, so that it adds a keyframe every other frame), six
frames.  Both sides run in one context whose matcher is forced to one form (4 wavefronts, 40 KB): in a fixed form a
registration's record does not depend on the size of the batch it runs in (test_every_form_of_the_matcher_agrees), so the
grouped launches of the grid and the two-job launches of the plain objects must agree exactly.  The grid runs behind torch's
stream handle (every matcher group on the context's stream) and in a context with a stream of its own (the groups dealt to
side streams); the plain objects always behind the handle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, COLS, N_FRAMES = 400, 3360, 6


@functools.lru_cache(maxsize=None)
def _ctx(private=False):
    """private: a context with a stream of its own -- there the grid deals its matcher groups to side streams; behind torch's
    stream handle (the default) every group runs on the context's stream."""
    import torch
    from tbv_slam_public_amd import api, _lib as L
    ctx = api.Context(0, None if private else (torch.cuda.current_stream(0).cuda_stream or 1))
    ctx.set_option(L.OPT_MATCHER_WAVES, 4)
    ctx.set_option(L.OPT_MATCHER_LDS_KB, 40)
    return ctx


def _configs():
    from tbv_slam_public_amd import api, _lib as L
    P = api.odometry_preset
    return [P("CFEAR-3"),                                                   # k 40, z_min 60, res 3, P2P, Huber 0.1, option 4, window 4
            P("CFEAR-3", kstrong_k_strongest=12),
            P("CFEAR-3", kstrong_z_min=70.0),
            P("CFEAR-3", res=3.5),
            P("CFEAR-3", reg_cost=L.COST["P2L"]),
            P("CFEAR-3", reg_loss=L.LOSS["Cauchy"], reg_loss_limit=0.2),
            P("CFEAR-3", reg_weight_opt=0),
            P("CFEAR-3", submap_scan_size=2, weight_intensity=0, compensate=0),
            P("CFEAR-3", filter_type=1)]                                    # CA-CFAR


@functools.lru_cache(maxsize=None)
def _sequences(zero_frame):
    """[2 sequences][frames][400][3360]; zero_frame: sequence 1 delivers an all-zero sweep in frame 3."""
    from tbv_slam_public_amd import synth
    seqs = np.stack([synth.scene_v1(0, N_FRAMES)[0], synth.scene_v1(1, N_FRAMES, speed=4.0)[0]])
    if zero_frame:
        seqs[1, 3] = 0
    seqs.setflags(write=False)
    return seqs


@functools.lru_cache(maxsize=None)
def _plain(config, zero_frame):
    """The plain pipeline: one OdometryKeyframeFuser(2, ...) with configuration `config` over both sequences -> info [frames][2]
    (computed once per configuration, shared, read only)."""
    from tbv_slam_public_amd import api
    seqs = _sequences(zero_frame)
    od = api.OdometryKeyframeFuser(2, ROWS, COLS, _configs()[config], ctx=_ctx())
    out = np.stack([od.process(np.ascontiguousarray(seqs[:, f])) for f in range(N_FRAMES)])
    od.close()
    out.setflags(write=False)
    return out


def _run_grid(stream_sequence, stream_config, zero_frame=False, device=False, private=False):
    import torch
    from tbv_slam_public_amd import api
    seqs = _sequences(zero_frame)
    grid = api.OdometryGrid(ROWS, COLS, _configs(), 2, stream_sequence, stream_config, ctx=_ctx(private))
    out = []
    for f in range(N_FRAMES):
        frame = np.ascontiguousarray(seqs[:, f])
        if device:
            frame = torch.from_numpy(frame).cuda()
            torch.cuda.synchronize()                                         # a private stream is not ordered with torch's
        out.append(grid.process(frame))
    seq, cfg = grid.stream_sequence, grid.stream_config
    grid.close()
    return np.stack(out), seq, cfg


def _assert_equal_to_plain(got, seq, cfg, zero_frame):
    for s in range(got.shape[1]):
        want = _plain(int(cfg[s]), zero_frame)[:, int(seq[s])]
        for f in range(N_FRAMES):
            assert got[f, s].tobytes() == want[f].tobytes(), (f, s, int(seq[s]), int(cfg[s]), got[f, s], want[f])


def test_the_plain_runs_tell_configurations_and_keyframes_apart():
    """Against a vacuous pass, on the plain side: configurations end at different poses, and within the six frames a stream
    adds a keyframe behind its first and a stream passes a frame without adding one."""
    n = len(_configs())
    last = np.stack([_plain(c, False)[-1]["pose"] for c in range(n)])       # [config][sequence][3]
    distinct = {last[c].tobytes() for c in range(n)}
    assert len(distinct) >= 2, last
    added = np.stack([_plain(c, False)["keyframe_added"][1:] for c in range(n)])
    status = np.stack([_plain(c, False)["reg_status"][1:] for c in range(n)])
    assert (added == 1).any() and ((added == 0) & (status == 0)).any()


@pytest.mark.parametrize("private", [False, True], ids=["torch-stream", "own-stream"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_full_product_equals_one_plain_object_per_configuration(device, private):
    from tbv_slam_public_amd import api
    plan = api.odometry_grid_plan(ROWS, COLS, _configs(), 2)["totals"]
    # per sequence: one k-strongest sweep (three classes: k 40 / z 60, k 12 / z 60, k 40 / z 70) and one CA-CFAR sweep
    assert (plan["n_streams"], plan["n_sweeps"], plan["n_classes"], plan["n_derived_classes"]) == (18, 4, 8, 6)
    assert plan["n_surface_groups"] == 4 and plan["n_matcher_groups"] == 5
    got, seq, cfg = _run_grid(None, None, device=device, private=private)
    assert seq.tolist() == [0] * 9 + [1] * 9 and cfg.tolist() == list(range(9)) * 2
    _assert_equal_to_plain(got, seq, cfg, False)


def test_ragged_streams_a_single_class_and_an_empty_sweep():
    """A ragged stream list in which sequence 0 holds one k-strongest class (the direct fused sweep, no derivation) and
    sequence 1 three; sequence 1's sweep of frame 3 is all zero: its streams report the surface stage's status and keep their
    state, the others are unaffected -- all of it exactly as the plain objects fed the same images."""
    from tbv_slam_public_amd import api, _lib as L
    seq = [0, 1, 0, 1, 1, 0, 1]
    cfg = [0, 3, 8, 1, 0, 6, 2]
    plan = api.odometry_grid_plan(ROWS, COLS, _configs(), 2, seq, cfg)
    assert plan["totals"]["n_derived_classes"] == 3 and plan["totals"]["n_classes"] == 5 and plan["totals"]["n_sweeps"] == 3
    got, s, c = _run_grid(seq, cfg, zero_frame=True, private=True)
    _assert_equal_to_plain(got, s, c, True)
    on1 = np.array(seq) == 1
    assert (got["reg_status"][3, on1] == L.ERR_EMPTY_CLOUD).all() and (got["n_points"][3, on1] == 0).all()
    assert (got["pose"][3, on1] == got["pose"][2, on1]).all()                 # the state is kept ...
    assert (got["reg_status"][4, on1] == 0).all()                             # ... and the stream goes on from it
    assert (got["reg_status"][3, ~on1] == 0).all()
    undisturbed = _plain(0, False)[:, 0]
    assert got[:, 0].tobytes() == undisturbed.tobytes()                       # stream 0 (sequence 0) never saw the empty sweep


def test_creation_refusals_carry_the_plans_reason():
    from tbv_slam_public_amd import api, _lib as L
    P = api.odometry_preset
    for configs, kw, match in (([P("CFEAR-3"), P("CFEAR-3", keep_nodes=1)], {}, "configuration 1: keep_nodes"),
                               ([P("CFEAR-3", estimate_cov_by_sampling=1)], {}, "configuration 0: estimate_cov_by_sampling"),
                               ([P("CFEAR-3", kstrong_k_strongest=65)], {}, "configuration 0: k_strongest"),
                               ([P("CFEAR-3")], dict(stream_sequence=[0, 2], stream_config=[0, 0]), "stream 1: sequence 2"),
                               ([P("CFEAR-3")], dict(stream_sequence=[], stream_config=[]), "n_streams must be >= 1")):
        with pytest.raises(L.CfearError, match=match) as e:
            api.OdometryGrid(ROWS, COLS, configs, 2, ctx=_ctx(), **kw)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
