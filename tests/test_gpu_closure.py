"""GPU: cfear_closure_candidates_batch (csrc/closure.hip) -- GTVicinityClosure and MiniClosure candidates of a batch of pose
graphs, one lane per origin node.  Every comparison is the device against the plain-Python restatement of the reference's
loops (tests/closure_cpu.py); only batch invariance compares the device with itself.

to and exhausted must be equal and eucl, trav, rel bitwise equal: + * / sqrt are correctly rounded on both sides and the
kernels are built without contraction.  odom_bounds is compared with the host function the kernel restates
(cfear_verify_by_odometry); only the device's cos / sin / exp may differ from the host's.  The largest deviation measured
over the cases of this file on an MI355X is 8.882e-16 (the 513-node lap; EXPERIMENTS.md, "Vicinity closure")."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import closure_cpu as M
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, T = L.CLOSURE_ORIGINS, L.CLOSURE_TILE
# |device odom_bounds - host odom_bounds|: ten times the largest deviation measured (8.882e-16), well inside 1e-12
ODOM_BOUND = 8.882e-15
MODES = ("gtvicinity", "mini")
CASES = M.small_cases() + [(n, 100.0, None) for n in (T - 1, T, T + 1, 2 * T + 1, 700)]


@functools.lru_cache(maxsize=None)
def _lap(n, circumference, seed=M.LAP_SEED):
    return M.lap(n, seed, circumference)


@functools.lru_cache(maxsize=None)
def _model(n, circumference, mode, small, seed=M.LAP_SEED):
    pos, steps, rel = _lap(n, circumference, seed)
    thr = dict(small) if small else M.DEFAULTS[mode]
    rec = M.candidates(pos, steps, mode, **thr)
    return rec, M.with_odom_bounds(rec, rel), thr


def _same(dev, rec, ob, where):
    assert dev["to"].tolist() == rec["to"].tolist(), where
    assert dev["exhausted"].tolist() == rec["exhausted"].tolist(), where
    for f in ("eucl", "trav", "rel"):
        assert dev[f].view(np.uint64).tolist() == rec[f].view(np.uint64).tolist(), (where, f)
    dev_ob = dev["odom_bounds"]
    d = float(np.abs(dev_ob - ob).max()) if len(ob) else 0.0
    print("%s: %d candidates, max |odom_bounds - host| = %.3e" % (where, int((rec["to"] >= 0).sum()), d))
    assert d <= ODOM_BOUND, (where, d)
    assert (dev_ob[rec["to"] < 0] == 0.0).all(), where


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,circumference,thr", CASES, ids=["%d-%s" % (c[0], "small" if c[2] else "default") for c in CASES])
def test_parity_with_the_model(n, circumference, thr, mode):
    pos, steps, rel = _lap(n, circumference)
    rec, ob, used = _model(n, circumference, mode, tuple(sorted(thr.items())) if thr else None)
    n_c = int((rec["to"] >= 0).sum())
    assert 0 < n_c < n                                     # no vacuous case
    dev = api.closure_candidates([(pos, steps, rel)], mode=mode, **used)[0]
    _same(dev, rec, ob, "n=%d %s" % (n, mode))
    if mode == "gtvicinity":
        assert not dev["exhausted"].any()


@pytest.mark.parametrize("mode", MODES)
def test_graphs_of_no_and_one_node_emit_nothing(mode):
    pos, steps, rel = _lap(1, 20.0)
    out = api.closure_candidates([(pos[:0], steps[:0], rel[:0]), (pos, steps, rel), (pos[:0], steps[:0], rel[:0])], mode=mode)
    assert [len(o) for o in out] == [0, 1, 0]
    assert out[1].tobytes() == np.array([(-1, 0, 0.0, 0.0, 0.0, 0.0)], L.CLOSURE_CANDIDATE_DTYPE).tobytes()
    assert [len(o) for o in api.closure_candidates([(pos[:0], steps[:0])], mode=mode)] == [0]


def _edge(pos, steps, mode, want_to=None, want_exhausted=None, **thr):
    pos, steps = np.asarray(pos, np.float64), np.asarray(steps, np.float64)
    rel = np.zeros((len(pos), 3))
    rel[:, 0] = steps
    rec = M.candidates(pos, steps, mode, **thr)
    dev = api.closure_candidates([(pos, steps, rel)], mode=mode, **thr)[0]
    _same(dev, rec, M.with_odom_bounds(rec, rel), "edge %s" % mode)
    if want_to is not None:
        assert dev["to"].tolist() == want_to
    if want_exhausted is not None:
        assert dev["exhausted"].tolist() == want_exhausted
    return dev


@pytest.mark.parametrize("mode", MODES)
def test_zero_travel_never_wins(mode):
    """min_d_travel = 0 with duplicated poses and zero steps: 0 / 0 is NaN and x / 0 is inf, and neither is < DBL_MAX."""
    pos = [[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [0.5, 0, 0]]
    dev = _edge(pos, [0.0, 0.0, 0.0, 1.0, 0.0], mode, want_to=[4, 4, 4, 4, -1], min_d_travel=0.0, max_d_travel=10.0, max_d_close=5.0)
    assert dev["rel"].tolist() == [0.5, 0.5, 0.5, 0.5, 0.0]
    # nothing but zero steps: every ratio is NaN or inf, nobody wins
    _edge(pos, [0.0] * 5, mode, want_to=[-1] * 5, want_exhausted=[0] * 5, min_d_travel=0.0, max_d_travel=10.0, max_d_close=5.0)


@pytest.mark.parametrize("mode", MODES)
def test_first_of_two_bit_equal_ratios_wins(mode):
    pos = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [4, 0, 0]]                    # from node 0: 1 / 2, 2 / 4, 4 / 8
    dev = _edge(pos, [2.0, 2.0, 4.0, 0.0], mode, min_d_travel=1.0, max_d_travel=100.0, max_d_close=10.0)
    assert dev["to"][0] == 1 and dev["rel"][0] == 0.5 and dev["eucl"][0] == 1.0 and dev["trav"][0] == 2.0


@pytest.mark.parametrize("mode", MODES)
def test_pairs_exactly_on_the_thresholds(mode):
    """Dyadic coordinates: every comparison is exact.  From node 0: node 1 sits on min_d_travel and max_d_close (3 / 4), node 2
    on max_d_travel and max_d_close (3 / 8, the winner), nodes 3 and 4 are nearer but past max_d_travel (MiniClosure gives the
    origin up there).  Then the pair (0, 1) alone, with each threshold moved by 2^-40 to the other side of it."""
    pos = [[0, 0, 0], [3, 0, 0], [0, 3, 0], [0.5, 0, 0], [0.5, 0.25, 0]]
    steps = [4.0, 4.0, 0.25, 0.25, 0.0]
    thr = dict(min_d_travel=4.0, max_d_travel=8.0, max_d_close=3.0)
    dev = _edge(pos, steps, mode, want_to=[2, 4, -1, -1, -1], want_exhausted=[1, 0, 0, 0, 0] if mode == "mini" else [0] * 5, **thr)
    assert (dev["eucl"][0], dev["trav"][0], dev["rel"][0]) == (3.0, 8.0, 0.375)
    only = _edge(pos[:2], steps[:2], mode, want_to=[1, -1], **thr)                    # on min_d_travel and on max_d_close: taken
    assert (only["eucl"][0], only["trav"][0], only["rel"][0]) == (3.0, 4.0, 0.75)
    for nudge, want in ((dict(max_d_close=3.0 - 2.0 ** -40), -1), (dict(min_d_travel=4.0 + 2.0 ** -40), -1), (dict(max_d_travel=4.0), 1),
                        (dict(max_d_travel=4.0 - 2.0 ** -40), -1)):
        _edge(pos[:2], steps[:2], mode, want_to=[want, -1], **dict(thr, **nudge))


def test_mini_gives_an_origin_up_before_any_close_pair():
    pos = [[10.0 * k, 0, 0] for k in range(6)]
    _edge(pos, [10.0] * 6, "mini", want_to=[-1] * 6, want_exhausted=[1, 1, 1, 0, 0, 0], min_d_travel=5.0, max_d_travel=25.0, max_d_close=3.0)
    _edge(pos, [10.0] * 6, "gtvicinity", want_to=[-1] * 6, want_exhausted=[0] * 6, min_d_travel=5.0, max_d_travel=25.0, max_d_close=3.0)
    # below min_d_travel an origin is never given up, even past max_d_travel (the reference asks `trav < min` first)
    _edge(pos, [10.0] * 6, "mini", want_to=[-1] * 6, want_exhausted=[1, 0, 0, 0, 0, 0], min_d_travel=45.0, max_d_travel=25.0, max_d_close=3.0)


@pytest.mark.parametrize("mode", MODES)
def test_odometry_bound_switched_off_or_without_motions(mode):
    n = G + 1
    pos, steps, rel = _lap(n, 20.0)
    rec = _model(n, 20.0, mode, tuple(sorted(M.SMALL.items())))[0]
    off = api.closure_candidates([(pos, steps, rel)], mode=mode, verify_via_odometry=0, **M.SMALL)[0]
    assert (off["odom_bounds"] == np.where(rec["to"] >= 0, 1.0, 0.0)).all() and off["to"].tolist() == rec["to"].tolist()
    none = api.closure_candidates([(pos, steps)], mode=mode, **M.SMALL)[0]
    assert (none["odom_bounds"] == 0.0).all() and none["to"].tolist() == rec["to"].tolist()
    # another sigma: still the host function's figure
    dev = api.closure_candidates([(pos, steps, rel)], mode=mode, odom_sigma_error=0.05, **M.SMALL)[0]
    assert np.abs(dev["odom_bounds"] - M.with_odom_bounds(rec, rel, 0.05)).max() <= ODOM_BOUND


@pytest.mark.parametrize("mode", MODES)
def test_batch_invariance(mode):
    sizes = [65, 0, T + 1, 1, 2, 63, 3, 0, 2 * T + 1, 64, T - 1, 1, G + 1, T, 0, 97, G - 1]
    assert len(sizes) == 17
    graphs = [_lap(n, 20.0, seed=100 + k) for k, n in enumerate(sizes)]
    together = api.closure_candidates(graphs, mode=mode, **M.SMALL)
    assert [len(o) for o in together] == sizes and sum((o["to"] >= 0).sum() for o in together) > 100
    alone = [api.closure_candidates([g], mode=mode, **M.SMALL)[0] for g in graphs]
    backwards = api.closure_candidates(graphs[::-1], mode=mode, **M.SMALL)[::-1]
    for k, (a, b, c) in enumerate(zip(together, alone, backwards)):
        assert a.tobytes() == b.tobytes() == c.tobytes(), k
    # and the batch is right, not only stable: one of its larger graphs against the model
    k = sizes.index(2 * T + 1)
    rec = M.candidates(graphs[k][0], graphs[k][1], mode, **M.SMALL)
    _same(together[k], rec, M.with_odom_bounds(rec, graphs[k][2]), "batched %s" % mode)


def test_refusals_leave_out_untouched_and_name_the_graph():
    ctx = api.default_context()
    parts = [M.lap(5, 1), M.lap(1, 2), M.lap(6, 3)]
    pos, steps, rel = (np.concatenate([p[k] for p in parts]) for k in range(3))
    off = np.array([0, 5, 5, 6, 12], np.int64)
    par = api.closure_params("mini", **M.SMALL)

    def call(p_, s_, o_, par_):
        out = np.full(len(p_), 7, L.CLOSURE_CANDIDATE_DTYPE)
        bad = C.c_int32(5)
        rc = ctx._lib.cfear_closure_candidates_batch(ctx.h, p_.ctypes.data, s_.ctypes.data, rel.ctypes.data, o_.ctypes.data, len(p_),
                                                     len(o_) - 1, C.byref(par_), out.ctypes.data, C.byref(bad))
        return rc, bad.value, out, ctx._lib.cfear_last_error(ctx.h).decode()

    def edited(arr, idx, v):
        a = arr.copy()
        a[idx] = v
        return a
    untouched = np.full(len(pos), 7, L.CLOSURE_CANDIDATE_DTYPE).tobytes()
    unknown = api.closure_params("mini")
    unknown.mode = -1
    cases = [(pos, steps, edited(off, 0, 1), par, 0), (pos, steps, edited(off, 4, 11), par, 3), (pos, steps, edited(off, 2, 4), par, 1),
             (pos, edited(steps, 8, -0.5), off, par, 3), (pos, edited(steps, 2, np.inf), off, par, 0), (pos, edited(steps, 1, np.nan), off, par, 0),
             (edited(pos, (5, 1), np.nan), steps, off, par, 2), (edited(pos, (11, 2), np.inf), steps, off, par, 3),
             (pos, steps, off, api.closure_params("mini", max_d_close=np.nan), -1), (pos, steps, off, api.closure_params("mini", min_d_travel=np.nan), -1),
             (pos, steps, off, api.closure_params("gtvicinity", max_d_travel=np.nan), -1), (pos, steps, off, unknown, -1)]
    for k, (p_, s_, o_, par_, want) in enumerate(cases):
        rc, bad, out, msg = call(p_, s_, o_, par_)
        assert (rc, bad) == (L.ERR_INVALID_ARGUMENT, want), (k, msg)
        assert out.tobytes() == untouched, k
        assert want < 0 or ("graph %d" % want) in msg, (k, msg)
    # the same arrays unedited are taken, and the unused last step of a graph may hold anything
    rc, bad, out, _ = call(pos, edited(steps, 4, np.nan), off, par)
    assert (rc, bad) == (L.OK, -1) and out.tobytes() != untouched
    rec = M.candidates(parts[2][0], parts[2][1], "mini", **M.SMALL)
    assert out["to"][6:].tolist() == rec["to"].tolist()
    # the Python wrapper reports the graph
    with pytest.raises(L.CfearError) as e:
        api.closure_candidates([parts[0], (parts[2][0], edited(parts[2][1], 2, -1.0), parts[2][2])], mode="mini")
    assert e.value.status == L.ERR_INVALID_ARGUMENT and e.value.graph == 1


def test_candidates_go_through_verification_end_to_end():
    """examples/vicinity_closure_demo.py on the lap of examples/loop_closure_demo.py: poses and odometry constraints from the
    odometry pipeline, candidates in both modes, closure_verify_jobs -> verify_loop_candidates: one record per candidate."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import vicinity_closure_demo as vdemo
    out = vdemo.run()
    n = len(out["poses"])
    assert n >= 2 and len(out["constraints"]) == n - 1
    pos, steps, rel = api._closure_graph_arrays((out["poses"], out["constraints"]), "lap")
    for mode in MODES:
        m = out["modes"][mode]
        rec = M.candidates(pos, steps, mode, **M.DEFAULTS[mode])
        _same(m["candidates"], rec, M.with_odom_bounds(rec, rel), "lap %s" % mode)
        n_c = int((rec["to"] >= 0).sum())
        assert n_c > 0 and len(m["jobs"]) == n_c == len(m["results"])
        assert [(j["from"], j["to"]) for j in m["jobs"]] == [(int(r["to"]), i) for i, r in enumerate(rec) if r["to"] >= 0]
        assert np.isfinite(m["results"]["probability"]).all()
        assert (m["results"]["odom_bounds"] == [j["odom_bounds"] for j in m["jobs"]]).all()
