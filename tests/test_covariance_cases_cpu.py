"""CPU: every case of tests/covariance_cases.py shows, on the oracle, the property it exists for -- so that the GPU test
(tests/test_gpu_covariance_matrix.py) compares against a reference that really walks the branch in question."""
import numpy as np
import pytest

from tests import covariance_cases as CC
from tests import covfit_ref as R


def test_the_case_list_is_complete_and_every_verdict_is_robust():
    cases = CC.cases()
    assert len(cases) == CC.EXPECTED_CASES and len({c["name"] for c in cases}) == len(cases)
    assert [c["group"] for c in cases].count("matrix") == 18
    for c in cases:
        s = CC.oracle_samples(c)
        ok, cov, smp = CC.oracle_cov(c)
        assert np.array_equal(smp[:, :3], s["offsets"]), c["name"]
        assert np.array_equal(smp[:, 3], s["costs"]), c["name"]              # the oracle carries as restated here
        assert ok == CC.numpy_verdict(c, s["costs"])[0], c["name"]
        assert CC.robust(c), c["name"]


def _branch_share(case):
    """Share of the residual blocks of the centre sample beyond the loss's branch (s > a^2; ln(1 + s) > 1 for Combined)."""
    from oracle import pyoracle as O
    from tests.test_oracle_pinning import DenseProblem
    cells, par = CC.case_cells(case), CC.oracle_par(case)
    pairs, w = O.associate(cells, case["poses"], par, case["first_itr"])
    prob = DenseProblem(cells, case["poses"], pairs, w, case["cost"], case["loss"], case["limit"], dtype=np.longdouble)
    prob.normal_eq(case["poses"][-1])
    if case["loss"] == "Combined":
        return float((np.log1p(prob.sq) > 1.0).mean())
    return float((prob.sq > np.longdouble(case["limit"]) ** 2).mean())


@pytest.mark.parametrize("cost", CC.COSTS)
def test_sampling_matrix(cost):
    for loss in CC.LOSSES:
        c = CC.by_name("matrix-%s-%s" % (cost, loss))
        s = CC.oracle_samples(c)
        assert len(c["window"]) == 3 and c["n"] == 3 and s["ok"].all() and s["blocks"].min() >= 30, c["name"]
        if loss in CC.BRANCHED:
            share = _branch_share(c)
            assert 0.05 <= share <= 0.95, (c["name"], share)


def test_failing_samples():
    c = CC.by_name("failing-samples")
    s = CC.oracle_samples(c)
    assert len(c["window"]) == 2 and c["n"] == 3
    assert not s["ok"][0] and s["costs"][0] == 0.0                           # a leading failure carries 0.0
    first = int(np.argmax(s["ok"]))
    assert (~s["ok"][first:]).any()                                          # a failure after a success
    assert s["ok"].sum() >= 3
    assert (s["blocks"][~s["ok"]] == 0).all() and (s["blocks"][s["ok"]] >= 30).all()   # nobody at the num_residuals > 1 edge
    for i in np.flatnonzero(~s["ok"]):
        assert s["costs"][i] == (s["costs"][i - 1] if i else 0.0)
    assert len(set(s["costs"][s["ok"]].tolist())) == int(s["ok"].sum())      # distinct values: a wrong carry shows


def test_all_samples_fail():
    c = CC.by_name("all-fail")
    s = CC.oracle_samples(c)
    assert not s["ok"].any() and (s["blocks"] == 0).all() and (s["costs"] == 0.0).all() and len(s["costs"]) == 27
    assert CC.oracle_cov(c)[0] is False


def test_rejected_far_from_the_optimum():
    c = CC.by_name("far-from-optimum")
    s = CC.oracle_samples(c)
    assert s["ok"].all() and s["blocks"].min() >= 30
    assert CC.oracle_cov(c)[0] is False
    ev = R.mp_fit(s["offsets"], s["costs"], 1.0, 1.0)[2]
    assert min(ev) < 0 and abs(min(ev)) >= 1e-6 * max(abs(e) for e in ev), ev    # indefinite, not marginally


def test_accepted():
    assert {c["cost"] for c in CC.accepted()} == set(CC.COSTS)
    for c in CC.accepted():
        ok, cov, _ = CC.oracle_cov(c)
        assert ok and np.all(np.linalg.eigvalsh(R.block3(cov)) > 0), c["name"]


def test_summary_record():
    base = CC.oracle_cov(CC.by_name("summary-10-200"))
    assert base[0]
    ok, cov, _ = CC.oracle_cov(CC.by_name("summary-0-200"))
    assert ok and np.array_equal(R.block3(cov), np.zeros((3, 3)))             # a zero score: a zero block, still accepted
    assert CC.oracle_cov(CC.by_name("summary-10-3"))[0] is False              # GetCovarianceScaler fails
    ok, cov, _ = CC.oracle_cov(CC.by_name("summary-10-2"))
    assert ok                                                                # 10 / (2 - 3): the negative scale, as the reference
    np.testing.assert_allclose(R.block3(cov), R.block3(base[1]) * (200 - 3) / (2 - 3), rtol=1e-12)
    assert R.block3(cov)[0, 0] < 0


def test_sample_counts():
    got = {}
    for c in CC.group("counts"):
        s = CC.oracle_samples(c)
        assert len(s["costs"]) == c["n"] ** 3 and s["ok"].all()
        ok, cov, _ = CC.oracle_cov(c)
        exp_ok, exp3 = CC.numpy_verdict(c, s["costs"])
        assert ok == exp_ok, c["name"]
        got[c["n"]] = ok
    assert sorted(got) == [1, 2, 4, 5, 15]
    assert len(CC.by_name("count-15")["window"]) == 2
