"""CPU: the bracket of tests/cen2019_audit_cpu.py against cen2019_cpu.literal() under shuffled tie
orders -- sound (R_in <= R(order) <= R_out, a certain target under every order, a clear sweep never changes), not vacuous,
and exact on the constructed sweeps."""
import os
import subprocess

import numpy as np
import pytest

from tests import cen2019_audit_cpu as A
from tests import cen2019_cpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ORDERS = 12


def _tset(t):
    return {tuple(x) for x in np.asarray(t).tolist()}


def _orders(img, mp, mr, im, seed):
    """literal() under the forward order, the reversed one and N_ORDERS shuffled ones"""
    out = [R.literal(img, mp, mr, im=im), R.literal(img, mp, mr, tie_rng=A.ReversedTies(), im=im)]
    rng = np.random.default_rng(seed)
    return out + [R.literal(img, mp, mr, tie_rng=rng, im=im) for _ in range(N_ORDERS)]


@pytest.fixture(scope="module")
def random_sweeps():
    """random_case(0 .. 399): per case the audit, and whether any order's marks / targets differ from the forward order's"""
    rows = []
    for k in range(400):
        img, mp, mr = R.random_case(k)
        pre = A.prepare(img)
        a = A.audit(img, mp, mr, pre=pre)
        lits = _orders(img, mp, mr, pre["im"], 9000 + k)
        rows.append((k, a, lits))
    return rows


def test_bracket_is_sound_on_random_sweeps(random_sweeps):
    bad = []
    for k, a, lits in random_sweeps:
        rec = a["record"][0]
        sure = _tset(a["targets"][a["certain"] == 1])
        fwd = lits[0]
        assert np.array_equal(a["R"], fwd["R"].astype(bool)) and np.array_equal(a["targets"], fwd["targets"]), k
        img, mp, mr = R.random_case(k)
        assert (rec["n_candidates"], rec["n_fresh"]) == tuple(R.order_free(img, mp, mr)["counts"][:2]), k
        for o, lit in enumerate(lits):
            Ro = lit["R"].astype(bool)
            if (a["R_in"] & ~Ro).any() or (Ro & ~a["R_out"]).any():
                bad.append((k, o, "bracket"))
            if not sure <= _tset(lit["targets"]):
                bad.append((k, o, "certain"))
            if rec["n_marks_in"] == rec["n_marks_out"] and not (np.array_equal(Ro, a["R"]) and np.array_equal(lit["targets"], a["targets"])):
                bad.append((k, o, "clear"))
    assert not bad, bad[:10]


def test_bracket_is_not_vacuous_and_some_sweep_is_exposed(random_sweeps):
    clear = sum(int(a["record"][0]["n_marks_in"] == a["record"][0]["n_marks_out"]) for _, a, _ in random_sweeps)
    n_t = sum(int(a["record"][0]["n_targets"]) for _, a, _ in random_sweeps)
    n_c = sum(int(a["record"][0]["n_targets_certain"]) for _, a, _ in random_sweeps)
    assert clear >= 200, clear                                              # at least half
    assert n_t > 0 and 4 * n_c >= 3 * n_t, (n_c, n_t)                       # at least three quarters
    exposed_and_changed = 0
    for _, a, lits in random_sweeps:
        rec = a["record"][0]
        if rec["n_marks_in"] != rec["n_marks_out"] and any(not np.array_equal(lit["R"].astype(bool), a["R"]) for lit in lits):
            exposed_and_changed += 1
    assert exposed_and_changed >= 1
    print("clear %d / 400, certain %d / %d targets, exposed and changed %d" % (clear, n_c, n_t, exposed_and_changed))


def test_witness_is_the_literal_loop_with_ties_by_descending_flat_index(random_sweeps):
    for k, a, lits in random_sweeps:
        rev, rec = lits[1], a["record"][0]
        assert np.array_equal(a["R_rev"], rev["R"].astype(bool)) and np.array_equal(a["targets_rev"], rev["targets"]), k
        assert rec["n_targets_reversed"] == len(rev["targets"]), k
        assert rec["n_targets_changed_reversed"] == len(_tset(rev["targets"]) ^ _tset(lits[0]["targets"])), k
        assert rec["n_marks_changed_reversed"] == int((rev["R"] != lits[0]["R"]).sum()), k
    img = R.tiled_case()
    for mp in (1, 15, 1000):
        a = A.audit(img, mp)
        rev = R.literal(img, mp, tie_rng=A.ReversedTies())
        assert np.array_equal(a["R_rev"], rev["R"].astype(bool)) and np.array_equal(a["targets_rev"], rev["targets"])


@pytest.mark.parametrize("name", list(R.SHAPES) + list(R.facts_cases()))
def test_sound_and_equal_to_order_free_at_every_max_points(name):
    """the sweeps the device sees: mean_h is order-free on each; at every max_points of the GPU test the forward part equals
    order_free(), the witness literal() reversed, and the bracket holds them and a shuffled order"""
    img = {**R.small_cases(), **R.facts_cases()}[name]
    pre = A.prepare(img)
    assert R.mean_h_margin(pre["im"])
    pre0 = R.prepare(img)
    mps = sorted(set(R.max_points_of(int(pre["sure"].sum()))) | set(R.max_points_of(int(pre["possible"].sum()))))
    for mp in mps:
        for mr in (0, 3) if mp == 8 else (0,):
            a = A.audit(img, mp, mr, pre=pre)
            ref = R.order_free(img, mp, mr, pre=pre0)
            assert np.array_equal(a["R"], ref["R"].astype(bool)) and np.array_equal(a["targets"], ref["targets"]), (name, mp)
            assert tuple(a["record"][0][["n_candidates", "n_fresh"]].tolist()) == tuple(ref["counts"][:2]), (name, mp)
            if img.size > 40000:
                continue                                                    # literal() is slow there
            sure = _tset(a["targets"][a["certain"] == 1])
            rev = R.literal(img, mp, mr, tie_rng=A.ReversedTies(), im=pre["im"])
            assert np.array_equal(a["R_rev"], rev["R"].astype(bool)) and np.array_equal(a["targets_rev"], rev["targets"]), (name, mp)
            for lit in (rev, R.literal(img, mp, mr, tie_rng=np.random.default_rng(mp), im=pre["im"])):
                Ro = lit["R"].astype(bool)
                assert not (a["R_in"] & ~Ro).any() and not (Ro & ~a["R_out"]).any() and sure <= _tset(lit["targets"]), (name, mp)


def test_mean_h_condition_on_the_random_sweeps_the_device_sees():
    """random_case(0 .. 199) go to the device except the four whose mean_h depends on the order of the fp64 sum (DESIGN.md
    section 4.10b, point 3: a separate open point); the batch and pitch sweeps are asserted in test_cen2019_cpu.py"""
    assert [k for k in range(200) if not R.mean_h_margin(R.images(R.random_case(k)[0]))] == list(A.RANDOM_WITHOUT_MARGIN)
    assert len(A.device_random_cases()) == 196


def test_wrap_case_cut_inside_the_tie_of_the_two_peaks():
    """the two peaks (rows 0 and 4, bin 11) carry the sweep's largest h, alone in their runs: both sure.  max_points = 1: the
    first of them in the order is K and the only mark, so the band is the two of them and the reversed witness marks the
    other one"""
    img = R.wrap_case()
    a = A.audit(img, 1)
    rec = a["record"][0]
    assert rec["n_band"] == 2 and rec["n_marks_in"] == 0 and rec["n_marks_out"] == 2 and rec["n_marks"] == 1
    assert np.argwhere(a["R"]).tolist() == [[0, 11]] and np.argwhere(a["R_rev"]).tolist() == [[4, 11]]
    assert rec["n_marks_changed_reversed"] == 2 and rec["h_hi"] == rec["h_lo"] == A.prepare(img)["h"].max()
    # max_points = 2: both are processed under every order, but the bracket does not see that (h_hi == h_lo, a band of the two):
    # exposed is the conservative answer, and the witness shows no change
    b = A.audit(img, 2)["record"][0]
    assert b["n_band"] == 2 and b["n_marks_in"] == 0 and b["n_marks"] == b["n_marks_out"] == 2
    assert b["n_marks_changed_reversed"] == 0 and b["n_targets_changed_reversed"] == 0 and b["n_targets"] == 2


def test_tiled_case_with_a_cut_inside_a_tie_is_exposed():
    img = R.tiled_case()
    a = A.audit(img, 15)
    rec = a["record"][0]
    assert rec["n_band"] >= 2 and rec["n_marks_in"] < rec["n_marks_out"]
    assert rec["n_marks_changed_reversed"] > 0
    full = A.audit(img, 1000)["record"][0]                                  # nothing is cut: every order processes everything
    assert full["n_band"] == 0 and np.isneginf(full["h_hi"]) and np.isneginf(full["h_lo"])


def test_straddle_case_fields():
    """straddle_case(): 6 x 24, T = 5, row 2 one run with no neighbour.  Bin 9, beside the dark bin 10, has the row's largest
    g and so its largest h (s < 0): the top own h sits at r >= T alone, no order can mark beyond bin 9, the sweep is clear.
    straddle_tied_case(): bins 2, 4 (< T) and 9 (>= T) tie for it.  R_in marks bins 0 .. 9, R_out the whole row (14 bins
    more), this library's order the whole row, the reversed order bins 0 .. 9."""
    img = R.straddle_case()
    pre = A.prepare(img)
    a = A.audit(img, 1000, pre=pre)
    rec = a["record"][0]
    assert pre["neg"][2].all() and int(np.argmax(np.where(pre["cand"][2], pre["h"][2], -np.inf))) == 9
    assert rec["n_rows_straddle_tied"] == 0 and rec["n_band"] == 0 and np.isneginf(rec["h_hi"]) and np.isneginf(rec["h_lo"])
    assert rec["n_marks_in"] == rec["n_marks"] == rec["n_marks_out"] and rec["n_marks_changed_reversed"] == 0
    assert a["R"][2, :10].all() and not a["R"][2, 10:].any() and rec["n_targets_certain"] == rec["n_targets"]
    img = A.straddle_tied_case()
    pre = A.prepare(img)
    assert R.mean_h_margin(pre["im"]) and pre["neg"][2].all()
    h2 = np.where(pre["cand"][2], pre["h"][2], -np.inf)
    assert np.nonzero(h2 == h2.max())[0].tolist() == [2, 4, 9]
    a = A.audit(img, 1000, pre=pre)
    rec = a["record"][0]
    assert rec["n_rows_straddle_tied"] == 1 and rec["n_band"] == 0
    assert a["R_in"][2, :10].all() and not a["R_in"][2, 10:].any() and a["R_out"][2].all()
    assert a["R"][2].all() and np.array_equal(a["R_rev"][2], a["R_in"][2])
    assert rec["n_marks_out"] - rec["n_marks_in"] == 14 and rec["n_marks"] == rec["n_marks_out"] and rec["n_marks_changed_reversed"] == 14
    assert np.array_equal(R.literal(img)["R"].astype(bool), a["R"])
    assert np.array_equal(R.literal(img, tie_rng=A.ReversedTies())["R"].astype(bool), a["R_rev"])
    assert rec["n_targets"] == 5 and rec["n_targets_reversed"] == 6 and rec["n_targets_changed_reversed"] == 1


def test_flat_case_is_all_zero_with_nan_levels():
    a = A.audit(R.flat_case())
    rec = a["record"][0]
    assert all(int(rec[n]) == 0 for n in A.RECORD_DTYPE.names[:14]) and np.isnan(rec["h_hi"]) and np.isnan(rec["h_lo"])
    assert len(a["targets"]) == 0 and not a["marks"].any()


def test_max_points_0_processes_nothing():
    rec = A.audit(R.small_cases()["8x40"], 0)["record"][0]
    assert rec["n_band"] == rec["n_marks_out"] == rec["n_targets"] == 0 and np.isposinf(rec["h_hi"]) and np.isposinf(rec["h_lo"])


def test_full_sweep():
    """the one slow case: a 400 x 3360 synthetic sweep.  max_points 1000: clear, 1000 marks, 123 targets; 10000: a band of
    15 candidates, every one of the 636 targets certain."""
    img = R.synth_image(3, 3360)
    pre = A.prepare(img)
    assert R.mean_h_margin(pre["im"])
    a = A.audit(img, 1000, pre=pre)["record"][0]
    assert a["n_marks_in"] == a["n_marks"] == a["n_marks_out"] == 1000 and a["n_targets"] == a["n_targets_certain"] == 123
    b = A.audit(img, 10000, pre=pre)["record"][0]
    assert b["n_band"] == 15 and b["n_targets"] == b["n_targets_certain"] == 636
    ref = R.order_free(img, 10000)
    assert np.array_equal(A.audit(img, 10000, pre=pre)["targets"], ref["targets"])


def test_cpp_mirror_compiles_against_the_cv_bridge_standin(tmp_path):
    exe = str(tmp_path / "cen2019_audit_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "cen2019_audit_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)
