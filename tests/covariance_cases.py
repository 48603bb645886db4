"""Shared cases of the covariance by cost sampling (odometrykeyframefuser.cpp:261-380, loopclosure.cpp:99-208): built and
judged on the CPU oracle (tests/test_covariance_cases_cpu.py asserts, per case, the property the case exists for), then
run on the GPU by tests/test_gpu_covariance_matrix.py.  The oracle and NumPy only: no GPU here.

Scans are the oracle's own cells (scene_v1 at k = 12: 40-125 cells per scan; uploaded with MapPointNormal(cells=...), so no
mean differs).  A case = dict(name, group, scene = (kind, seed, frames), window = indices into the scene's scans, cost, loss,
limit, wopt, outer, inner (SetParameters), poses (after the oracle's register where the case has one), first_itr (the
leftover itr_ GetCost's radius follows), summary = (final_cost, num_residuals) of the registration record, n, xy_range,
yaw_range, scaler).

Every verdict, accepted or rejected, must survive 100 random relative perturbations of +-1e-9 of the oracle's sample costs
(ten times the GPU bound on a sample cost) under the NumPy fit, so that the GPU's summation order cannot decide one; a case
that does not is re-chosen here, never skipped (robust() is asserted for every case by the CPU test, and EXPECTED_CASES
keeps the list from losing one).
"""
import numpy as np

from tests import covfit_ref as R

COSTS = ("P2P", "P2L", "P2D")
LOSSES = ("None", "Huber", "Cauchy", "SoftLOne", "Combined", "Tukey")
BRANCHED = ("Huber", "Tukey", "Combined")
FORM_PAIRS = (("P2P", "Huber"), ("P2P", "SoftLOne"), ("P2L", "Huber"), ("P2L", "Tukey"), ("P2D", "Huber"), ("P2D", "Combined"))
ODOM = dict(xy_range=0.4, yaw_range=0.0043625, scaler=4.0)       # odometrykeyframefuser.h:107-110
LOOP = dict(xy_range=0.4, yaw_range=0.0044, scaler=4.0)          # loopclosure.cpp:108-112
MATRIX_SCENE = ("v1", 5, (0, 2, 4))
PAIR_SCENE = ("v1", 6, (0, 1))
SMALL_SCENE = ("v1", 7, (0, 1, 2))                               # ~40 cells per scan: the n = 15 job
FAR = 800.0                                                      # xy_range of the failing-sample cases: offsets of +-400 m, more
                                                                 # than two sensor ranges (2 x 147 m) + the association radius
EXPECTED_CASES = 18 + 1 + 1 + 1 + 4 + 5
_CACHE = {}


def rel(a, b):
    c, s = np.cos(a[2]), np.sin(a[2])
    d = b[:2] - a[:2]
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], b[2] - a[2]])


def scene(key):
    """(cells of the scene's frames, their poses relative to the first) -- built once per key."""
    if key not in _CACHE:
        from oracle import pyoracle as O
        from tbv_slam_public_amd import synth
        kind, seed, frames = key
        world = synth.scene_dense if kind == "dense" else synth.scene_v1
        imgs, gt, _ = world(seed, max(frames) + 1)
        cells = []
        for f in frames:
            sr, si, sc = O.kstrongest(imgs[f], 40 if kind == "dense" else 12, 60)
            cells.append(O.surface_points(O.kstrongest_cloud(sr, si, sc, 0.0438, 2.5), 3.0, 1.0, (0, 0), True))
        _CACHE[key] = (cells, np.array([rel(gt[frames[0]], gt[f]) for f in frames]))
    return _CACHE[key]


def case_cells(case):
    cells, _ = scene(case["scene"])
    return [cells[i] for i in case["window"]]


def oracle_par(case):
    from oracle import pyoracle as O
    return O.reg_params(cost=case["cost"], loss=case["loss"], loss_limit=case["limit"], weight_opt=case["wopt"],
                        max_outer=case["outer"], max_inner=case["inner"], first_itr=case["first_itr"])


def _case(name, group, scene_key, window, cost, loss, limit, wopt, offset, register=True, outer=8, inner=20, first_itr=0,
          summary=None, n=3, sampling=ODOM, **over):
    from oracle import pyoracle as O
    _, truth = scene(scene_key)
    poses = np.array([rel(truth[window[0]], truth[i]) for i in window], dtype=np.float64)
    poses[-1] += np.asarray(offset, dtype=np.float64)
    c = dict(name=name, group=group, scene=scene_key, window=tuple(window), cost=cost, loss=loss, limit=limit, wopt=wopt,
             outer=outer, inner=inner, poses=poses, first_itr=first_itr, summary=summary, n=n, **sampling)
    c.update(over)
    if register:
        ok, pr, res = O.register(case_cells(c), poses, oracle_par(c))
        assert ok, name
        c["poses"], c["first_itr"] = pr, int(res.outer_iters)
        if summary is None:
            c["summary"] = (float(res.final_cost), int(res.num_residuals))
    assert c["summary"] is not None, name
    return c


def matrix_limit(cost):
    return 0.3 if cost == "P2L" else 1.0                              # as test_gpu_matcher_matrix.test_get_cost_batch chooses


def cases():
    if "cases" not in _CACHE:
        out = []
        for cost in COSTS:
            for loss in LOSSES:
                # At a converged P2L pose under 2 % of the blocks lie beyond Huber's or Tukey's branch and none beyond Combined's
                # (|r| > 1.31 m): those three are sampled after a registration that stops before its first solver step
                # (max_itr_solver = 0, usable as Ceres 2.1 has it), 3 x (0.4, -0.3, 0.01) from the truth.
                early = cost == "P2L" and loss in BRANCHED
                out.append(_case("matrix-%s-%s" % (cost, loss), "matrix", MATRIX_SCENE, (0, 1, 2), cost, loss, matrix_limit(cost), 4,
                                 (1.2, -0.9, 0.03) if early else (0.2, -0.1, 0.005), outer=1 if early else 8, inner=0 if early else 20))
        pair = dict(scene_key=PAIR_SCENE, window=(0, 1), cost="P2L", loss="Huber", limit=0.1, wopt=0, register=False, first_itr=4,
                    summary=(10.0, 200))
        far = dict(ODOM, xy_range=FAR)
        out.append(_case("failing-samples", "failing", offset=(0.0, 0.0, 0.0), sampling=far, **pair))
        out.append(_case("all-fail", "all-fail", offset=(1500.0, 1500.0, 0.0), sampling=far, **pair))
        out.append(_case("far-from-optimum", "rejected", offset=REJECTED_OFFSET, **pair))
        acc = dict(scene_key=MATRIX_SCENE, window=(0, 1, 2), cost="P2L", loss="Huber", limit=0.3, wopt=4, offset=(0.2, -0.1, 0.005))
        for fc, nres in ((10.0, 200), (0.0, 200), (10.0, 3), (10.0, 2)):
            out.append(_case("summary-%g-%d" % (fc, nres), "summary", summary=(fc, nres), **acc))
        cnt = dict(scene_key=MATRIX_SCENE, window=(0, 2), cost="P2L", loss="Huber", limit=0.1, wopt=0, offset=(0.2, -0.1, 0.005))
        for n in (1, 2, 4, 5):
            out.append(_case("count-%d" % n, "counts", n=n, **cnt))
        out.append(_case("count-15", "counts", SMALL_SCENE, (0, 1), "P2L", "Huber", 0.1, 0, (0.2, -0.1, 0.005), n=15, sampling=LOOP))
        _CACHE["cases"] = out
    return _CACHE["cases"]


# pose offset of the rejected case (the construction of test_cov_by_sampling_not_convex_is_rejected), chosen on the oracle so
# that the fit is indefinite with its most negative eigenvalue far from 0 (test_covariance_cases_cpu asserts both)
REJECTED_OFFSET = (1.2, 1.0, 0.05)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def group(g):
    return [c for c in cases() if c["group"] == g]


def accepted():
    """One accepted case per cost among the sampling matrix."""
    return [by_name("matrix-%s-%s" % (cost, loss)) for cost, loss in ACCEPTED]


ACCEPTED = (("P2P", "Huber"), ("P2L", "Cauchy"), ("P2D", "Huber"))


def oracle_samples(case):
    """GetCost at every sample, as approximateCovarianceBySampling walks them -> dict(offsets [m, 3], ok [m] bool,
    blocks [m] residual blocks, raw [m] GetCost's own cost, costs [m] with a failed sample carrying the previous value
    (0.0 before the first success)); cached."""
    key = ("samples", case["name"])
    if key not in _CACHE:
        from oracle import pyoracle as O
        cells, par = case_cells(case), oracle_par(case)
        off = R.offsets(case["n"], case["xy_range"] * 0.5, case["yaw_range"] * 0.5)
        ok, blocks, raw, costs, last = [], [], [], [], 0.0
        rpb = 1 if case["cost"] == "P2L" else 2
        for o in off:
            p = np.array(case["poses"], dtype=np.float64)
            p[-1] = [o[0] + p[-1][0], o[1] + p[-1][1], o[2] + p[-1][2]]          # odometrykeyframefuser.cpp:297-299
            good, c, res, _ = O.get_cost(cells, p, par)
            assert len(res) % rpb == 0
            if good:
                last = c
            ok.append(good); blocks.append(len(res) // rpb); raw.append(c); costs.append(last)
        _CACHE[key] = dict(offsets=off, ok=np.array(ok), blocks=np.array(blocks), raw=np.array(raw), costs=np.array(costs))
    return _CACHE[key]


def oracle_cov(case):
    """The oracle's approximateCovarianceBySampling -> (verdict, cov 6x6, samples [m, 4]); cached."""
    key = ("cov", case["name"])
    if key not in _CACHE:
        from oracle import pyoracle as O
        _CACHE[key] = O.cov_by_sampling(case_cells(case), case["poses"], oracle_par(case), case["summary"][0], case["summary"][1],
                                        case["xy_range"], case["yaw_range"], case["n"], case["scaler"])
    return _CACHE[key]


def numpy_verdict(case, costs):
    """(verdict, 3x3 block or None) of the NumPy fit with GetCovarianceScaler's own refusal (n_scan_normal.cpp:433-439)."""
    fc, nres = case["summary"]
    if nres - 3 == 0:
        return False, None
    return R.numpy_fit(oracle_samples(case)["offsets"], costs, fc / (nres - 3), case["scaler"])


def robust(case, trials=100, rel_step=1e-9):
    """The NumPy verdict on the oracle's costs survives `trials` perturbations of +-rel_step of every successful sample (a
    carried value moves with the sample it came from)."""
    s = oracle_samples(case)
    base = numpy_verdict(case, s["costs"])[0]
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    for _ in range(trials):
        raw = s["raw"] * (1.0 + rel_step * rng.choice([-1.0, 1.0], size=s["raw"].shape))
        costs, last = [], 0.0
        for good, c in zip(s["ok"], raw):
            if good:
                last = c
            costs.append(last)
        if numpy_verdict(case, np.array(costs))[0] != base:
            return False
    return True
