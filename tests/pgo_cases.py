"""The pose-graph case matrix: seeded NumPy generators of planar and SPATIAL graphs, the topology variants the solvers'
loops can get wrong, and the parameter sets they are solved under.  Shared by tests/test_pgo_matrix_cpu.py (host solver
against the dense reference of tests/pgo_dense.py) and tests/test_gpu_pgo_matrix.py (device solver against both).

  spatial_lap   a helix: yaw, pitch, roll and z all move, so the (x, y, yaw) and (z, roll, pitch) subsystems do NOT decouple
                and all six tangent columns of every node carry gradient.  Nodes are the SE(3)-integrated biased odometry;
                t_be is the relative pose in the begin node's frame; every constraint has its own SPD information.
  planar_lap    synth.pgo_lap_graph with its truth lifted to [n, 7].
  SIZES         node counts at the wavefront's lane boundaries (the device loops are nd = 1 + lane; nd < n, c = lane; c < m
                and k < 6 n) with loop counts that put the block count m on 63, 64, 65, 128 and 129.
  variants      hubs onto node 0 / node n-1 / a middle node, type-1 loops between neighbours in both storage orders, an
                odometry edge stored twice, a graph of type-1 constraints only, a last node nothing touches, outlier loops,
                a scrambled start.
  MATRIX        {parameter set name: (par dict, [case names])}; cases() builds every graph once.
A constraint with id_begin == id_end is not a case: Ceres refuses duplicate parameter blocks."""
import numpy as np

from pgo_dense import plus, qconj, qmul, qrot
from tbv_slam_public_amd import synth

ID_STEP = 10


def _quat_zyx(yaw, pitch, roll):
    """[..., 4] (x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll)."""
    z = np.zeros_like(yaw)
    qz = np.stack([z, z, np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    qy = np.stack([z, np.sin(pitch / 2), z, np.cos(pitch / 2)], -1)
    qx = np.stack([np.sin(roll / 2), z, z, np.cos(roll / 2)], -1)
    return qmul(qmul(qz, qy), qx)


def rel7(a, b):
    """The pose of b in a's frame, [..., 7]."""
    qai = qconj(a[..., 3:])
    return np.concatenate([qrot(qai, b[..., :3] - a[..., :3]), qmul(qai, b[..., 3:])], -1)


def comp7(a, r):
    return np.concatenate([a[..., :3] + qrot(a[..., 3:], r[..., :3]), qmul(a[..., 3:], r[..., 3:])], -1)


def _small7(d):
    """A small relative pose from a 6-vector (translation, rotation vector / 2)."""
    return plus(np.array([0, 0, 0, 0, 0, 0, 1.0]), np.asarray(d, float))


def spd(rng):
    a = rng.normal(0, 0.3, (6, 6))
    return a @ a.T + np.diag([100.0, 100.0, 60.0, 40.0, 30.0, 1000.0])


def _con(i, j, t_be, info, typ):
    return dict(id_begin=int(i) * ID_STEP, id_end=int(j) * ID_STEP, t_be=np.asarray(t_be, float), information=info, type=typ)


def loop_between(true, i, j, rng, outlier=False):
    """A type-1 constraint from node i to node j measuring the TRUE relative pose (plus noise; outlier: metres away)."""
    meas = comp7(rel7(true[i], true[j]), _small7(rng.normal(0, 0.002, 6)))
    if outlier:
        meas = comp7(meas, _small7([6.0, -4.0, 1.5, 0.1, -0.05, 0.15]))
    return _con(i, j, meas, spd(rng), 1)


def spatial_lap(n, rng, n_loops=4, direction="back", drift=(0.02, 0.01, 0.008, 0.001, -0.0015, 0.002), outlier=False, extras=True):
    """-> (poses [n, 7], ids [n], constraints, true [n, 7]); the arguments of synth.pgo_lap_graph, in three dimensions."""
    i = np.arange(n)
    th = 2 * np.pi * i / max(n, 2)
    p = np.stack([20 * np.sin(th), 20 * (1 - np.cos(th)), 3 * np.sin(2 * th) + 0.05 * i], 1)
    true = np.concatenate([p, _quat_zyx(th, 0.25 * np.sin(2 * th + 0.3), 0.2 * np.cos(3 * th))], 1)
    scale = min(1.0, 24.0 / n)                     # the lap's total drift stays that of a 24-node lap
    est = np.zeros((n, 7))
    est[0] = true[0]
    for k in range(1, n):
        step = comp7(rel7(true[k - 1], true[k]), _small7(np.asarray(drift) * scale + rng.normal(0, 0.003 * scale, 6)))
        est[k] = comp7(est[k - 1], step)
    est[:, 3:] /= np.linalg.norm(est[:, 3:], axis=1, keepdims=True)
    cons = []
    for k in range(1, n):
        b = direction == "back" or (direction == "mixed" and rng.random() < 0.5)
        a_, b_ = (k, k - 1) if b else (k - 1, k)
        cons.append(_con(a_, b_, rel7(est[a_], est[b_]), spd(rng), 0))
    for k in range(min(n_loops, n // 2)):
        cons.append(loop_between(true, n - 1 - k, k, rng, outlier))
    if extras and n > 1:
        cons.insert(len(cons) // 2, _con(1, 0, comp7(_small7([9, 9, 1, 0, 0, 0]), _small7([0, 0, 0, 0.1, 0.2, 0.5])), np.eye(6), 3))
        cons.append(_con(0, n - 1, _small7([-3, 2, 0.5, 0.2, 0.1, 0.25]), np.eye(6), 2))
    return est, i * ID_STEP, cons, true


def planar_lap(n, rng, n_loops=4, direction="back", outlier=False):
    poses, ids, cons, true = synth.pgo_lap_graph(n, rng, n_loops=n_loops, direction=direction, outlier=outlier, id_step=ID_STEP)
    z = np.zeros(n)
    return poses, ids, cons, np.concatenate([true[:, :2], z[:, None], _quat_zyx(true[:, 2], z, z)], 1)


# ---- topology variants: each takes a lap (poses, ids, cons, true) and returns one --------------------------------------------
def with_hub(lap, hub, rng, n_loops=72):
    """n_loops type-1 constraints between `hub` and the other nodes, every other one stored from the hub outwards; the
    others cycle, so some pairs are joined twice and the hub's neighbours are among them."""
    poses, ids, cons, true = lap
    others = [k for k in range(len(ids)) if k != hub]
    cons = list(cons)
    for k in range(n_loops):
        o = others[(7 * k) % len(others)]
        cons.append(loop_between(true, *((hub, o) if k % 2 else (o, hub)), rng))
    return poses, ids, cons, true


def with_neighbour_loops(lap, rng):
    """Type-1 constraints between neighbouring nodes (they enter the chain part of the preconditioner), in both storage
    orders, the pairs (1, 0) and (n-1, n-2) included."""
    poses, ids, cons, true = lap
    n = len(ids)
    cons = list(cons)
    for k in sorted(set([0, 1, n // 2, n - 2])):
        cons.append(loop_between(true, k + 1, k, rng))
        cons.append(loop_between(true, k, k + 1, rng))
    return poses, ids, cons, true


def with_duplicate_odometry(lap, rng):
    """The odometry edge into the middle node a second time (its own information), stored last."""
    poses, ids, cons, true = lap
    odo = [c for c in cons if c["type"] == 0]
    return poses, ids, list(cons) + [dict(odo[len(odo) // 2], information=spd(rng))], true


def loops_only(lap):
    """Every odometry constraint retyped to 1: no type-0 block at all (n_odom = 0), the chain is made of Cauchy blocks."""
    poses, ids, cons, true = lap
    return poses, ids, [dict(c, type=1) if c["type"] == 0 else c for c in cons], true


def with_untouched_node(lap):
    """One more node, last, that no constraint names."""
    poses, ids, cons, true = lap
    extra = comp7(poses[-1], _small7([1.0, 0.5, 0.25, 0.05, 0.1, -0.2]))
    return np.vstack([poses, extra]), np.append(ids, ids[-1] + ID_STEP), cons, np.vstack([true, extra])


def scrambled(lap, rng, sigma_p=1.0, sigma_r=0.3):
    """The same graph started from poses knocked about in all six directions (node 0 stays): far from the odometry's
    optimum, so the trust region has to shrink before steps are accepted."""
    poses, ids, cons, true = lap
    out = plus(poses, np.concatenate([rng.normal(0, sigma_p, (len(ids), 3)), rng.normal(0, sigma_r, (len(ids), 3))], 1))
    out[0] = poses[0]
    return out, ids, cons, true


# ---- the matrix ----------------------------------------------------------------------------------------------------------
# (n, loops): m = n - 1 + loops lands on 63, 64, 65, 128 and 129
SIZES = [(2, 1), (3, 1), (7, 2), (63, 1), (64, 1), (65, 1), (66, 4), (129, 0), (129, 1)]
DIRECTIONS = ("back", "forward", "mixed")
SEED = 20241019


def _build():
    out = {}

    def rng_of(name):
        return np.random.default_rng([SEED] + [ord(ch) for ch in name])

    for kind, lap in (("planar", planar_lap), ("spatial", spatial_lap)):
        for k, (n, loops) in enumerate(SIZES):
            name = "%s_n%d_l%d" % (kind, n, loops)
            out[name] = lap(n, rng_of(name), n_loops=loops, direction=DIRECTIONS[k % 3])
    for kind, lap in (("planar", planar_lap), ("spatial", spatial_lap)):
        def base(name, direction="back", **kw):
            return lap(66, rng_of(name), n_loops=4, direction=direction, **kw)
        for hub_name, hub in (("hub0", 0), ("hublast", 65), ("hubmid", 31)):
            name = "%s_%s" % (kind, hub_name)
            out[name] = with_hub(base(name, "mixed"), hub, rng_of(name + "+"))
        name = kind + "_neighbours"
        out[name] = with_neighbour_loops(base(name, "forward"), rng_of(name + "+"))
    name = "spatial_duplicate"
    out[name] = with_duplicate_odometry(spatial_lap(66, rng_of(name), n_loops=4, direction="mixed"), rng_of(name + "+"))
    name = "spatial_loops_only"
    out[name] = loops_only(spatial_lap(66, rng_of(name), n_loops=4, direction="mixed"))
    name = "spatial_untouched"
    out[name] = with_untouched_node(spatial_lap(65, rng_of(name), n_loops=4, direction="back"))
    name = "spatial_outliers"
    out[name] = spatial_lap(66, rng_of(name), n_loops=6, direction="forward", outlier=True)
    name = "planar_outliers"
    out[name] = planar_lap(66, rng_of(name), n_loops=6, direction="forward", outlier=True)
    name = "spatial_scrambled"
    out[name] = scrambled(spatial_lap(66, rng_of(name), n_loops=4, direction="mixed"), rng_of(name + "+"))
    name = "spatial_restart"                       # solved twice by the CPU test: the second start is the first solution
    out[name] = spatial_lap(24, rng_of(name), n_loops=4, direction="back")
    return out


_CASES = None


def cases():
    """{name: (poses, ids, constraints, true)}; built once, never modified by a test."""
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


FULL = dict(replace_cov_by_identity=0, loop_scaling=1.0)
_SIZE_NAMES = ["%s_n%d_l%d" % (kind, n, loops) for kind in ("planar", "spatial") for n, loops in SIZES]
_TOPOLOGY = ["planar_hub0", "planar_hublast", "planar_hubmid", "planar_neighbours", "planar_outliers", "spatial_hub0", "spatial_hublast",
             "spatial_hubmid", "spatial_neighbours", "spatial_duplicate", "spatial_loops_only", "spatial_untouched", "spatial_outliers",
             "spatial_scrambled", "spatial_restart"]
_CORE = ["spatial_n65_l1", "spatial_hub0", "spatial_loops_only", "planar_n64_l1"]
MATRIX = {
    "full_ls1": (FULL, _SIZE_NAMES + _TOPOLOGY),
    "default": (dict(), _CORE + ["spatial_scrambled"]),
    "full_ls5e5": (dict(replace_cov_by_identity=0, loop_scaling=500000.0), _CORE),
    "full_ls50_limit05": (dict(replace_cov_by_identity=0, loop_scaling=50.0, loop_loss_limit=0.5), _CORE + ["spatial_scrambled", "spatial_neighbours"]),
    "identity_ls1_odom": (dict(replace_cov_by_identity=1, loop_scaling=1.0, odom_vxx=0.02, odom_vyy=0.005, odom_vtt=0.002), _CORE + ["spatial_hubmid"]),
    "identity_ls50_limit05": (dict(replace_cov_by_identity=1, loop_scaling=50.0, loop_loss_limit=0.5), ["spatial_n65_l1", "spatial_hublast"]),
    "full_ls1_iter0": (dict(FULL, max_num_iterations=0), ["spatial_n65_l1", "spatial_hub0", "planar_n64_l1"]),
    "full_ls1_iter1": (dict(FULL, max_num_iterations=1), ["spatial_n65_l1", "spatial_hub0", "spatial_scrambled"]),
    "full_ls1_iter2": (dict(FULL, max_num_iterations=2), ["spatial_n65_l1", "spatial_hub0", "spatial_scrambled"]),
}


def solves():
    """[(parameter set, case)] of the whole matrix."""
    return [(s, c) for s, (_, names) in MATRIX.items() for c in names]


# ---- the yardsticks of one solve, computed once per process and shared by the CPU and the GPU tests --------------------------
_DENSE, _HOST = {}, {}


def dense(set_name, case):
    """(x, costs, history, blocks) of dense_lm on one solve of the matrix."""
    if (set_name, case) not in _DENSE:
        from pgo_dense import DensePGO, dense_lm
        par = dict(MATRIX[set_name][0])
        max_iter = par.pop("max_num_iterations", 200)
        poses, ids, cons, _ = cases()[case]
        prob = DensePGO(cons, ids, par)
        _DENSE[set_name, case] = dense_lm(prob, poses, max_iter=max_iter) + (prob.m,)
    return _DENSE[set_name, case]


def host(set_name, case):
    """(poses, summary) of cfear_pgo_solve on one solve of the matrix."""
    if (set_name, case) not in _HOST:
        from tbv_slam_public_amd import api
        poses, ids, cons, _ = cases()[case]
        _HOST[set_name, case] = api.pose_graph_optimize(poses, ids, cons, **MATRIX[set_name][0])
    return _HOST[set_name, case]


# what a solver must share with the dense reference: the bounds tests/test_pgo.py holds the host solver to; BOUND_C0 and
# COST_FLOOR are derived in tests/test_pgo_matrix_cpu.py
BOUND_P, BOUND_Q, BOUND_COST = 2e-6, 2e-7, 1e-6
BOUND_C0 = 10 * 1.3e-14
COST_FLOOR = 1e-25


def check_against_dense(out, summ, set_name, case):
    """What a solver's result for one solve of the matrix must share with the dense reference (also used by the GPU tests)."""
    poses = cases()[case][0]
    ref, costs, hist, blocks = dense(set_name, case)
    dp, dq = np.abs(out[:, :3] - ref[:, :3]).max(), np.abs(out[:, 3:] - ref[:, 3:]).max()
    d0 = abs(summ["initial_cost"] - costs[0])
    d1 = abs(summ["final_cost"] - min(costs))
    noise = min(costs) <= 1e3 * COST_FLOOR                                # a cost of rounding errors has no relative figure
    figures = dict(dp=dp, dq=dq, c0=0.0 if noise else d0 / costs[0], c1=0.0 if noise else d1 / min(costs))
    where = (set_name, case, figures)
    assert summ["iterations"] == len(costs) - 1, where                     # the same accept / reject history
    assert summ["usable"] is True and summ["num_residual_blocks"] == blocks, where
    assert dp <= BOUND_P and dq <= BOUND_Q, where
    assert d0 <= BOUND_C0 * costs[0] + COST_FLOOR, where
    assert d1 <= BOUND_COST * min(costs) + COST_FLOOR, where
    assert out[0].tobytes() == poses[0].tobytes(), where                   # the first node is constant
    assert np.abs(np.linalg.norm(out[:, 3:], axis=1) - 1.0).max() <= 1e-12, where
    if case == "spatial_untouched":
        assert out[-1].tobytes() == poses[-1].tobytes(), where
    if MATRIX[set_name][0].get("max_num_iterations") == 0:
        assert out.tobytes() == poses.tobytes() and summ["final_cost"] == summ["initial_cost"], where
    return figures
