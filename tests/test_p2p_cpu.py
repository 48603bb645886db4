"""CPU: the NumPy definition of p2pQuality / keypointRepetability / scanEvaluator (tests/p2p_cpu.py) against an
independent double loop, the reference's quirks (the +3 divisor, the strict radius test) and the text of eval.txt."""
import math
import re

import numpy as np

from tests import p2p_cpu as R

F = np.float32


def _brute(ref, src, T, radius):
    """scalar double loop over np.float32 values: nothing shared with R.nearest / R.transform"""
    r2 = F(float(radius) * float(radius))
    res, per_point = [], []
    for p in src:
        x, y, z = float(p[0]), float(p[1]), float(p[2])
        qx = F(((T[0] * x + T[1] * y) + 0.0 * z) + T[2])
        qy = F(((T[3] * x + T[4] * y) + 0.0 * z) + T[5])
        qz = F(p[2])
        best = None
        for c in ref:
            dx, dy, dz = F(qx - F(c[0])), F(qy - F(c[1])), F(qz - F(c[2]))
            d = F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
            if d < r2 and (best is None or d < best):
                best = d
        per_point.append(F(-1) if best is None else best)
        if best is not None:
            res.append(float(best))
    total = 0.0
    for v in res:
        total += v
    return np.array(per_point, F), len(res), total, total / (len(res) + 3)


def test_definition_equals_brute_force():
    rng = np.random.default_rng(5)
    for n_ref, n_src, radius, span in [(40, 30, 3.0, 10.0), (1, 7, 0.5, 1.0), (57, 64, 1.0, 4.0), (30, 20, 3.0, 200.0)]:
        ref = (rng.standard_normal((n_ref, 4)) * [span, span, 0.5, 1.0]).astype(F)
        src = (rng.standard_normal((n_src, 4)) * [span, span, 0.5, 1.0]).astype(F)
        T = R.tchange((1.0, -2.0, 0.3), (1.5, -1.0, 0.1), (0.2, -0.1, 0.02))
        got = R.p2p(ref, src, T, radius)
        pp, matched, total, mean = _brute(ref, src, T, radius)
        assert np.array_equal(got["per_point"].view(np.uint32), pp.view(np.uint32))
        assert (got["matched"], got["n_src"]) == (matched, n_src)
        assert got["sum"] == total and got["mean"] == mean
        assert got["repeatability"] == [matched / n_src, float(matched), float(n_src)]


def test_tchange_is_inverse_times_source_times_offset():
    ref_pose, src_pose, off = (3.0, -1.0, 0.7), (2.0, 0.5, -0.4), (0.1, 0.2, 0.05)

    def mat(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        return np.array([[c, -s, p[0]], [s, c, p[1]], [0, 0, 1.0]])
    want = np.linalg.inv(mat(ref_pose)) @ mat(src_pose) @ mat(off)
    np.testing.assert_allclose(R.tchange(ref_pose, src_pose, off).reshape(2, 3), want[:2], rtol=0, atol=1e-14)
    assert np.array_equal(R.tchange((0, 0, 0), (0, 0, 0)), [1, 0, 0, 0, 1, 0])


def test_plus_three_divisor_and_leading_zeros():
    ref = np.array([[0, 0, 0, 1], [10, 0, 0, 1]], F)
    src = np.array([[1, 0, 0, 1], [10, 2, 0, 1], [50, 50, 0, 1]], F)
    r = R.p2p(ref, src, R.tchange((0, 0, 0), (0, 0, 0)), 3.0)
    assert r["residuals"] == [0.0, 0.0, 0.0, 1.0, 4.0]
    assert r["matched"] == 2 and r["sum"] == 5.0 and r["mean"] == 5.0 / 5.0 and r["quality"] == [1.0, 0.0, 0.0]
    assert r["repeatability"] == [2.0 / 3.0, 2.0, 3.0]
    none = R.p2p(ref, src[2:], R.tchange((0, 0, 0), (0, 0, 0)), 3.0)
    assert none["matched"] == 0 and none["mean"] == 0.0 and none["residuals"] == [0.0, 0.0, 0.0]
    empty = R.p2p(ref, np.zeros((0, 4), F), R.tchange((0, 0, 0), (0, 0, 0)), 3.0)
    assert math.isnan(empty["repeatability"][0]) and empty["repeatability"][1:] == [0.0, 0.0]


def test_radius_test_is_strict():
    ref = np.zeros((1, 4), F)
    ident = R.tchange((0, 0, 0), (0, 0, 0))
    at = R.p2p(ref, np.array([[3, 0, 0, 0]], F), ident, 3.0)
    assert at["matched"] == 0 and at["per_point"][0] == F(-1)          # 9.0f is not < 9.0f
    below = np.nextafter(F(3), F(0))
    inside = R.p2p(ref, np.array([[below, 0, 0, 0]], F), ident, 3.0)
    assert inside["matched"] == 1 and inside["per_point"][0] == F(below * below) < F(9)
    # z enters the distance: (0, 0, 3) is as far as (3, 0, 0)
    assert R.p2p(ref, np.array([[0, 0, 3, 0]], F), ident, 3.0)["matched"] == 0
    assert R.p2p(ref, np.array([[0, 0, below, 0]], F), ident, 3.0)["matched"] == 1


def test_create_perturbations():
    v = R.create_perturbations(4, 2 * math.pi, 0.1, 0.0)
    assert len(v) == 5 and v[0] == [0.0, 0.0, 0.0]
    for i in range(4):
        a = i / 4.0 * (2 * math.pi)
        assert v[1 + i] == [0.1 * math.cos(a), 0.1 * math.sin(a), 0.0]
    np.testing.assert_allclose(v[1:], [[0.1, 0, 0], [0, 0.1, 0], [-0.1, 0, 0], [0, -0.1, 0]], atol=1e-16)
    d = R.create_perturbations()                                         # ScanEvaluator.h:63-78
    th = 0.57 * math.pi / 180.0
    assert d == [[0.0, 0.0, 0.0], [0.5, 0.0, th], [0.5 * math.cos(math.pi / 4), 0.5 * math.sin(math.pi / 4), th]]
    assert [R.aligned(e) for e in v] == [True, False, False, False, False]
    assert [R.aligned(e) for e in d] == [True, False, False]
    assert R.aligned([0.00003, -0.00003, 0.00003]) and not R.aligned([0.00005, -0.00005, 0.0])


def _sequence(n=4):
    rng = np.random.default_rng(11)
    world = (rng.uniform(-20, 20, (60, 4)) * [1, 1, 0, 1]).astype(F)
    scans = []
    for k in range(n):
        T = (0.8 * k, 0.1 * k, 0.02 * k)
        c, s = math.cos(T[2]), math.sin(T[2])
        cloud = world.copy()
        dx, dy = world[:, 0] - T[0], world[:, 1] - T[1]
        cloud[:, 0], cloud[:, 1] = c * dx + s * dy, -s * dx + c * dy
        scans.append({"T": T, "cloud": cloud, "pose_id": 100 + k})
    return scans


def test_eval_txt():
    scans = _sequence(4)
    for spacing in (1, 2):
        dps = R.evaluate(scans, "P2P", 3.0, spacing, offset_rotation_steps=2)
        lines = R.eval_text(dps).split("\n")
        assert lines[-1] == "" and len(lines) - 2 == len(dps) == (4 - spacing) * 3
        assert lines[0] == "index,ref_id,src_id,distance, score1,score2,score3,aligned,error x,error y,error theta"
        rows = [ln.split(",") for ln in lines[1:-1]]
        assert [int(r[0]) for r in rows] == [1 + i // 3 for i in range(len(rows))]
        ks = [spacing + i // 3 for i in range(len(rows))]
        assert [int(r[1]) for r in rows] == [100 + k - 1 for k in ks]       # ref = the back of the window
        assert [int(r[2]) for r in rows] == [100 + k for k in ks]
        assert [r[7] for r in rows] == ["1", "0", "0"] * (4 - spacing)
        for r, d in zip(rows, dps):
            assert len(r) == 11
            for col in (3, 4, 5, 6, 8, 9, 10):
                assert re.fullmatch(r"-?\d+\.\d{6}", r[col]), r[col]
            assert r[3] == "%f" % math.hypot(0.8, 0.1) and r[4] == "%f" % d["score"][0] and r[5] == r[6] == "0.000000"
            assert r[8:] == ["%f" % e for e in d["perturbation"]]
    # the clouds are one world seen from exact poses: the aligned row scores best
    dps = R.evaluate(scans, "P2P", 3.0, 1)
    for i in range(0, len(dps), 3):
        assert dps[i]["aligned"] and dps[i]["score"][0] < min(dps[i + 1]["score"][0], dps[i + 2]["score"][0])
    rep = R.evaluate(scans, "keypoint_repetability", 3.0, 1)
    assert rep[0]["score"][2] == 60.0 and rep[0]["score"][0] == rep[0]["score"][1] / 60.0 and rep[0]["residuals"] == [0.0, 0.0, 0.0]


def test_synthetic_sequence_scores_the_aligned_row_best():
    """the property tests/test_gpu_p2p.py asserts of the kernel's rows holds for the definition first"""
    dps = R.evaluate(R.synthetic_sequence(8), "P2P", 3.0, 1)
    assert len(dps) == 7 * 3
    for i in range(0, len(dps), 3):
        assert dps[i]["aligned"] and dps[i]["score"][0] < min(dps[i + 1]["score"][0], dps[i + 2]["score"][0])
