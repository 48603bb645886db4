"""GPU: cfear_pgo_solve_batch (csrc/pgo_batch.hip) -- many pose graphs in one call, one wavefront each.

The yardsticks are the unchanged host solver cfear_pgo_solve and the dense NumPy LM of tests/pgo_dense.py; the device
solver is never compared with itself, except where the claim IS self-consistency (batch invariance, bit for bit).

Device against host, graph by graph (test_batch_matches_host_solver): the counts must be equal; poses and costs differ by
summation order only (the device splits the host's serial sums over 64 lanes) and by the last bit of sin / cos / log.
Measured on the first green run over the four parameter sets of the seeded 256-graph batch (EXPERIMENTS.md, "Batched pose-graph optimisation"):
    position 6.416e-08 m, quaternion 1.210e-09, cost (relative) 4.526e-12   (all three at loop_scaling 1 with the constraints' own
    information; 2.3e-13 m / 5.3e-15 / 2.5e-13 with the identity replacement, 1.0e-10 m / 1.7e-12 / 5.8e-14 at loop_scaling 500000)
The bounds below are ten times those figures, and never looser than the 2e-6 m / 2e-7 / 1e-6 the host solver itself is
held to against the dense LM.  Seeds replaced because a graph sat on a tolerance threshold: none."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tbv_slam_public_amd import synth
from pgo_dense import DensePGO, dense_lm
from test_pgo import PAR, _loop_graph
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20240611
# ten times the measured maxima (module docstring), capped by the host solver's own bounds against the dense LM
BOUND_P, BOUND_Q, BOUND_COST = min(10 * 6.416e-08, 2e-6), min(10 * 1.210e-09, 2e-7), min(10 * 4.526e-12, 1e-6)
COUNTS = ("iterations", "usable", "num_residual_blocks")


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _deviation(dev, host):
    (dp, ds), (hp, hs) = dev, host
    return (np.abs(dp[:, :3] - hp[:, :3]).max(), np.abs(dp[:, 3:] - hp[:, 3:]).max(),
            max(abs(ds[k] - hs[k]) / max(abs(hs[k]), 1e-300) for k in ("initial_cost", "final_cost")))


def _same_bits(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


@pytest.mark.parametrize("loop_scaling", [500000.0, 50.0])
def test_batch_matches_dense_lm_with_exact_steps(ctx, loop_scaling):
    """The graphs of test_pgo_matches_dense_lm_with_exact_steps, both loop_scaling values' graphs in one batch per value."""
    graphs = [_loop_graph(24, np.random.default_rng(3))[:3], _loop_graph(24, np.random.default_rng(3))[:3]]
    par = dict(PAR, loop_scaling=loop_scaling)
    res = api.pose_graph_optimize_batch(graphs, ctx=ctx, loop_scaling=loop_scaling)
    for (poses, ids, cons), (out, summ) in zip(graphs, res):
        ref, costs, _ = dense_lm(DensePGO(cons, ids, par), poses)
        print("dense LM: iterations", summ["iterations"], len(costs) - 1, "cost", summ["initial_cost"], costs[0], summ["final_cost"], min(costs),
              "max |dp|", np.abs(out[:, :3] - ref[:, :3]).max(), "max |dq|", np.abs(out[:, 3:] - ref[:, 3:]).max())
        assert summ["usable"] and summ["num_residual_blocks"] == 23 + 4
        assert summ["iterations"] == len(costs) - 1
        np.testing.assert_allclose(summ["initial_cost"], costs[0], rtol=1e-12)
        np.testing.assert_allclose(summ["final_cost"], min(costs), rtol=1e-6)
        np.testing.assert_allclose(out[:, :3], ref[:, :3], atol=2e-6)
        np.testing.assert_allclose(out[:, 3:], ref[:, 3:], atol=2e-7)
        np.testing.assert_array_equal(out[0], poses[0])
        np.testing.assert_allclose(np.linalg.norm(out[:, 3:], axis=1), 1.0, atol=1e-12)
        assert summ["final_cost"] < summ["initial_cost"]


@pytest.mark.parametrize("loop_scaling,replace", [(500000.0, 1), (500000.0, 0), (1.0, 1), (1.0, 0)])
def test_batch_matches_host_solver(ctx, loop_scaling, replace):
    graphs = synth.pgo_ragged_batch(SEED)
    assert len(graphs) >= 256 and min(len(g[1]) for g in graphs) == 2 and max(len(g[1]) for g in graphs) == 4096
    par = dict(loop_scaling=loop_scaling, replace_cov_by_identity=replace)
    dev = api.pose_graph_optimize_batch(graphs, ctx=ctx, **par)
    worst = np.zeros(3)
    mismatched = []
    for g, (poses, ids, cons) in enumerate(graphs):
        host = api.pose_graph_optimize(poses, ids, cons, **par)
        if any(dev[g][1][k] != host[1][k] for k in COUNTS):
            mismatched.append((g, len(ids), {k: (dev[g][1][k], host[1][k]) for k in COUNTS}))
        worst = np.maximum(worst, _deviation(dev[g], host))
        np.testing.assert_array_equal(dev[g][0][0], poses[0])
    print("device against host, loop_scaling %g replace %d: max |dp| %.3e m, max |dq| %.3e, max relative cost %.3e; count mismatches %s"
          % (loop_scaling, replace, worst[0], worst[1], worst[2], mismatched))
    assert not mismatched
    assert worst[0] <= BOUND_P and worst[1] <= BOUND_Q and worst[2] <= BOUND_COST


def test_batch_invariance_bit_for_bit(ctx):
    """Alone, anywhere in a shuffled batch, and under any chunking a graph's poses and summary are the same bits."""
    graphs = synth.pgo_ragged_batch(SEED + 1, n_graphs=23, n_max=700, loops_max=20)
    base = api.pose_graph_optimize_batch(graphs, ctx=ctx, loop_scaling=1.0)
    for g in (0, 5, 22):
        assert _same_bits(api.pose_graph_optimize_batch([graphs[g]], ctx=ctx, loop_scaling=1.0)[0], base[g])
    order = np.random.default_rng(9).permutation(len(graphs))
    shuffled = api.pose_graph_optimize_batch([graphs[i] for i in order], ctx=ctx, loop_scaling=1.0)
    for k, i in enumerate(order):
        assert _same_bits(shuffled[k], base[i]), (k, i)
    assert ctx.get_option(L.OPT_PGO_GRAPH_CHUNK) == 0                        # never set on this context: chunks by the budget alone
    capped = api.Context(0)
    try:
        for chunk in (1, 7, 2 ** 31 - 1):
            capped.set_option(L.OPT_PGO_GRAPH_CHUNK, chunk)
            again = api.pose_graph_optimize_batch(graphs, ctx=capped, loop_scaling=1.0)
            assert all(_same_bits(a, b) for a, b in zip(again, base)), chunk
        with pytest.raises(L.CfearError):
            capped.set_option(L.OPT_PGO_GRAPH_CHUNK, 0)                       # a cap of 0 graphs is refused
        assert capped.get_option(L.OPT_PGO_GRAPH_CHUNK) == 2 ** 31 - 1
    finally:
        capped.close()


def test_batch_closes_the_loop_when_loops_are_trusted(ctx):
    """test_pgo_closes_the_loop_when_loops_are_trusted, solved on the device (both parameter sets, two calls: one per set)."""
    rng = np.random.default_rng(5)
    poses, ids, cons, true = _loop_graph(60, rng, drift=(0.001, 0.001, 0.0002), n_loops=6)
    before = np.abs(poses[-1, :2] - true[-1, :2]).max()
    (out, summ), = api.pose_graph_optimize_batch([(poses, ids, cons)], ctx=ctx, loop_scaling=1.0)
    after = np.abs(out[-1, :2] - true[-1, :2]).max()
    assert summ["usable"] and before > 0.5 and after < 0.02 * before
    (out2, _), = api.pose_graph_optimize_batch([(poses, ids, cons)], ctx=ctx)
    assert np.abs(out2[-1, :2] - poses[-1, :2]).max() < 0.05
    assert summ["linear_iterations"] <= 40 * max(summ["iterations"], 1)


def test_prefix_batch_equals_host_prefix_by_prefix(ctx):
    poses, ids, cons = synth.pgo_lap_graph(300, np.random.default_rng(11), n_loops=9, drift=(0.004, 0.002, 0.0008))[:3]
    prefixes = api.pose_graph_prefixes(poses, ids, cons)
    assert len(prefixes) == 9
    dev = api.pose_graph_optimize_batch(prefixes, ctx=ctx, loop_scaling=1.0)
    for (p, i, c), d in zip(prefixes, dev):
        host = api.pose_graph_optimize(p, i, c, loop_scaling=1.0)
        assert all(d[1][k] == host[1][k] for k in COUNTS), (d[1], host[1])
        dp, dq, dc = _deviation(d, host)
        assert dp <= BOUND_P and dq <= BOUND_Q and dc <= BOUND_COST


def _raw_call(ctx, arrs, par=None, node_off="auto", con_off="auto", n_nodes=None, n_cons=None):
    """cfear_pgo_solve_batch on caller-owned arrays -> (rc, failed graph, poses as the call left them)."""
    p = L.PgoParams()
    ctx._lib.cfear_pgo_params_default(C.byref(p))
    for k, v in (par or {}).items():
        setattr(p, k, type(getattr(p, k))(v))
    no = np.concatenate([[0], np.cumsum([a[0].shape[0] for a in arrs])]).astype(np.int64) if isinstance(node_off, str) else node_off
    co = np.concatenate([[0], np.cumsum([a[2].shape[0] for a in arrs])]).astype(np.int64) if isinstance(con_off, str) else con_off
    poses = np.ascontiguousarray(np.concatenate([a[0] for a in arrs], 0))
    ids = np.ascontiguousarray(np.concatenate([a[1] for a in arrs]))
    cons = np.ascontiguousarray(np.concatenate([a[2] for a in arrs]))
    summ = np.zeros(len(arrs), L.PGO_SUMMARY_DTYPE)
    bad = C.c_int32(-7)
    rc = ctx._lib.cfear_pgo_solve_batch(ctx.h, poses.ctypes.data, ids.ctypes.data, None if no is None else no.ctypes.data,
                                        poses.shape[0] if n_nodes is None else n_nodes, cons.ctypes.data,
                                        None if co is None else co.ctypes.data, cons.shape[0] if n_cons is None else n_cons,
                                        len(arrs), C.byref(p), summ.ctypes.data, C.byref(bad))
    return rc, bad.value, poses


def test_refusals_name_the_graph_and_leave_poses_untouched(ctx):
    """Each argument error of test_pgo_argument_errors (and non-SPD information) in the middle of an otherwise valid batch."""
    rng = np.random.default_rng(7)
    poses, ids, cons, _ = _loop_graph(8, rng, n_loops=1)
    good = api._pgo_graph_arrays(poses, ids, cons, "good")
    not_spd = [dict(c, information=-np.eye(6)) for c in cons]
    broken = {"ids descend": (poses, ids[::-1].copy(), cons, {}),
              "unknown node": (poses, ids, [dict(cons[0], id_begin=12345)], {}),
              "nothing to optimise": (poses, ids, [cons[-1]], {}),
              "information not SPD": (poses, ids, not_spd, dict(replace_cov_by_identity=0))}
    for name, (p, i, c, par) in broken.items():
        with pytest.raises(L.CfearError):
            api.pose_graph_optimize(p, i, c, **par)                         # the host solver refuses it: so must the batch
        arrs = [good, good, api._pgo_graph_arrays(p, i, c, name), good]
        before = np.concatenate([a[0] for a in arrs], 0)
        rc, bad, after = _raw_call(ctx, arrs, par)
        assert rc == L.ERR_INVALID_ARGUMENT and bad == 2, (name, rc, bad)
        assert after.tobytes() == before.tobytes(), name
        with pytest.raises(L.CfearError) as e:
            api.pose_graph_optimize_batch([(poses, ids, cons), (p, i, c)], ctx=ctx, **par)
        assert e.value.graph == 1 and "graph 1" in str(e.value)
    # offsets: null, or not spanning the arrays (a table of the wrong size)
    arrs = [good, good]
    before = np.concatenate([a[0] for a in arrs], 0)
    for kw in (dict(node_off=None), dict(con_off=None), dict(node_off=np.array([0, 8, 15], np.int64)), dict(con_off=np.array([0, 3, 5], np.int64)),
               dict(node_off=np.array([0, 12, 16], np.int64), con_off=np.array([0, 9, 18], np.int64), n_nodes=15),
               dict(node_off=np.array([1, 8, 16], np.int64)), dict(node_off=np.array([0, 17, 16], np.int64))):
        rc, bad, after = _raw_call(ctx, arrs, **kw)
        assert rc == L.ERR_INVALID_ARGUMENT and after.tobytes() == before.tobytes(), kw
    rc, bad, after = _raw_call(ctx, arrs)
    assert rc == L.OK and bad == -1 and after.tobytes() != before.tobytes()


def _tables_call(ctx, node, n_nodes, con, n_cons):
    """Two offset tables alone: a malformed one is refused before an array is read -> (rc, failed graph, message)."""
    node, con = np.array(node, np.int64), np.array(con, np.int64)
    poses, ids, cons = np.zeros((16, 7)), np.arange(16, dtype=np.uint64), np.zeros(16, L.GRAPH_CONSTRAINT_DTYPE)
    summ = np.zeros(len(node), L.PGO_SUMMARY_DTYPE)
    p, bad = L.PgoParams(), C.c_int32(-7)
    ctx._lib.cfear_pgo_params_default(C.byref(p))
    rc = ctx._lib.cfear_pgo_solve_batch(ctx.h, poses.ctypes.data, ids.ctypes.data, node.ctypes.data, n_nodes, cons.ctypes.data, con.ctypes.data,
                                        n_cons, len(node) - 1, C.byref(p), summ.ctypes.data, C.byref(bad))
    return rc, bad.value, ctx._lib.cfear_last_error(ctx.h).decode()


def test_malformed_offset_tables_blame_the_same_graph_as_before(ctx):
    """The tables of tests/test_batch_tables_cpu.py, as node offsets beside a sound constraint table and the other way
    round.  This entry point asks for its context first, so it is not among that test's calls without a device.  It tests the
    start and the end of both tables before any range, and then blames the first range that descends or is too large; the
    literals are what the library answered before the checks were folded into one helper."""
    from test_batch_tables_cpu import BIG, TABLES
    inv, cap = L.ERR_INVALID_ARGUMENT, L.ERR_CAPACITY
    ends = "offsets must run from 0 to n_nodes / n_constraints over n_graphs + 1 entries"
    graph = "graph %d: offsets descend, or more than 29826161 nodes / constraints"
    want = {"start not 0": (inv, -1, ends), "end short of total": (inv, -1, ends), "end past total": (inv, -1, ends),
            "descends": (inv, 1, graph % 1), "leaves then descends": (inv, 2, graph % 2),
            "first range leaves, second descends": (inv, 1, graph % 1), "descends and wrong end": (inv, -1, ends),
            "start not 0 and descends": (inv, -1, ends), "no ranges, start not 0": (inv, -1, ends),
            "no ranges, start not 0 but equal to total": (inv, -1, ends), "second range over capacity": (cap, 1, graph % 1)}
    sound = {1: [0], 4: [0, 2, 4, 6]}
    assert sorted(want) == sorted(t for t in TABLES if t not in ("fine", "empty ranges", "no ranges"))
    for name, (off, total) in TABLES.items():
        if name in want:
            mine = sound[len(off)]
            assert _tables_call(ctx, off, total, mine, mine[-1]) == want[name], ("node_offsets", name)
            assert _tables_call(ctx, mine, mine[-1], off, total) == want[name], ("constraint_offsets", name)
    # a descent in one table and a wrong end in the other: the ends are tested first; two descents: the earlier graph
    assert _tables_call(ctx, [0, 5, 3, 8], 8, [0, 2, 4, 6], 7) == (inv, -1, ends)
    assert _tables_call(ctx, [0, 3, 2, 8], 8, [0, 5, 3, 6], 6) == (inv, 1, graph % 1)
    assert _tables_call(ctx, [0, 2, 2 + BIG, 3 + BIG], 3 + BIG, [0, 5, 3, 6], 6) == (inv, 1, graph % 1)
    assert _tables_call(ctx, [0, 2 + BIG, 3 + BIG, 4 + BIG], 4 + BIG, [0, 3, 2, 6], 6) == (cap, 0, graph % 0)


def test_sizes_from_two_nodes_to_8192_nodes_and_1024_loops(ctx):
    big = synth.pgo_lap_graph(8192, np.random.default_rng(21), n_loops=1024)[:3]
    small = synth.pgo_lap_graph(2, np.random.default_rng(22), n_loops=1)[:3]
    dev = api.pose_graph_optimize_batch([small, big, small], ctx=ctx, loop_scaling=1.0)
    assert dev[1][1]["num_residual_blocks"] == 8191 + 1024 and dev[0][1]["num_residual_blocks"] == 2
    assert _same_bits(dev[0], dev[2])
    for g, d in zip((small, big), dev):
        host = api.pose_graph_optimize(*g, loop_scaling=1.0)
        assert all(d[1][k] == host[1][k] for k in COUNTS), (d[1], host[1])
        dp, dq, dc = _deviation(d, host)
        assert dp <= BOUND_P and dq <= BOUND_Q and dc <= BOUND_COST


def test_cpp_wrapper_runs(tmp_path):
    exe = str(tmp_path / "pgo_batch_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "pgo_batch_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    out = subprocess.check_output([exe], timeout=300).decode().split()
    assert out[:2] == ["2", "-1"]
    for g, n in enumerate((4, 6)):
        usable, blocks, iters, cost, x_last = out[2 + 5 * g:7 + 5 * g]
        assert (int(usable), int(blocks)) == (1, n - 1) and int(iters) >= 1
        assert float(cost) < 1e-9 and abs(float(x_last) - (n - 1)) < 1e-4      # unit steps along x: the chain straightens
