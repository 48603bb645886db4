"""NumPy models of cfear_loop_stats_batch and cfear_loop_curves_batch (csrc/loopeval.hip), a literal transcription of the
reference's per-candidate loop, and the inputs the CPU and GPU tests share.  No device, no sklearn."""
import math

import numpy as np

from tbv_slam_public_amd import _lib as L

STATS_DEFAULTS = dict(max_distance=6.0, max_registration_translation=4.0, max_registration_rotation_deg=2.5,
                      no_loop_distance=100000.0, min_index_gap=10)
CURVES_DEFAULTS = dict(p_threshold=0.9, drop_intermediate=1, reference_endpoints=1)
LDS_ROWS = L.LOOPEVAL_LDS_ROWS


# ---- loop rows ---------------------------------------------------------------------------------------------------------------
def _terror(pf, pt, g):
    """diff = Tguess^-1 (Tfrom^-1 Tto) in the order of include/cfear_hip.h, with libm's cos / sin / atan2."""
    dx, dy = pt[0] - pf[0], pt[1] - pf[1]
    cf, sf, ct, st, cg, sg = math.cos(pf[2]), math.sin(pf[2]), math.cos(pt[2]), math.sin(pt[2]), math.cos(g[2]), math.sin(g[2])
    cgd, sgd = cf * ct + sf * st, cf * st - sf * ct
    xgd, ygd = cf * dx + sf * dy, cf * dy - sf * dx
    cd, sd = cg * cgd + sg * sgd, cg * sgd - sg * cgd
    ex, ey = xgd - g[0], ygd - g[1]
    return cg * ex + sg * ey, cg * ey - sg * ex, math.atan2(sd, cd)


def _flags(r, closest, p):
    r["transl_error"] = math.sqrt(r["diff"][0] * r["diff"][0] + r["diff"][1] * r["diff"][1])
    r["rot_error"] = 180.0 / math.pi * math.fabs(r["diff"][2])
    r["is_loop"] = closest < p["max_distance"]
    r["candidate_close"] = (r["transl_error"] < p["max_registration_translation"]) and (r["rot_error"] < p["max_registration_rotation_deg"])
    r["prediction_pos_ok"] = (not r["is_loop"]) or r["candidate_close"]


def loop_stats_model(off, gt, has, cands, **par):
    p = dict(STATS_DEFAULTS, **par)
    gt = np.asarray(gt, np.float64).reshape(-1, 3)
    out = np.zeros(len(cands), L.LOOP_ROW_DTYPE)
    for i, c in enumerate(cands):
        n0 = int(off[c["graph"]])
        g, h = gt[n0:int(off[c["graph"] + 1])], has[n0:int(off[c["graph"] + 1])]
        fr, to = int(c["from"]), int(c["to"])
        r = out[i]
        r["diff"] = _terror(g[fr], g[to], c["guess_xyt"])
        closest, idx, cand = p["no_loop_distance"], fr, -1.0
        if h[fr]:
            if h[to]:
                dx, dy = g[to, 0] - g[fr, 0], g[to, 1] - g[fr, 1]
                cand = math.sqrt((dx * dx + dy * dy) + 0.0)
            k = np.arange(0, max(fr - p["min_index_gap"], 0))
            k = k[h[k] != 0]
            if k.size:
                dx, dy = g[fr, 0] - g[k, 0], g[fr, 1] - g[k, 1]
                d = np.sqrt((dx * dx + dy * dy) + 0.0)
                j = int(np.argmin(d))                            # the first minimum: the lowest k
                if d[j] < closest:
                    closest, idx = float(d[j]), int(k[j])
        r["closest_loop_distance"], r["candidate_loop_distance"], r["id_close"] = closest, cand, idx
        r["close_xy"] = g[idx, :2]
        _flags(r, closest, p)
    return out


def loop_stats_transcription(off, gt, has, cands, **par):
    """PoseGraph::UpdateStatistics, posegraph.cpp:332-371, line by line for planar poses (idx_ = position in the graph)."""
    p = dict(STATS_DEFAULTS, **par)
    gt = np.asarray(gt, np.float64).reshape(-1, 3)
    out = np.zeros(len(cands), L.LOOP_ROW_DTYPE)
    for i, c in enumerate(cands):
        n0, n1 = int(off[c["graph"]]), int(off[c["graph"] + 1])
        nearest_loop_distance = p["no_loop_distance"]
        candidate_loop_distance = -1.0
        frm, to = int(c["from"]), int(c["to"])
        Tposefrom, Tposeto = gt[n0 + frm], gt[n0 + to]
        close = frm
        if has[n0 + frm]:
            if has[n0 + to]:
                candidate_loop_distance = math.sqrt((Tposefrom[0] - Tposeto[0]) ** 2 + (Tposefrom[1] - Tposeto[1]) ** 2 + 0.0)
            for idx in range(n1 - n0):
                if not idx < frm:
                    break
                idx_diff = math.fabs(float(frm) - float(idx))
                if idx != frm and idx_diff > p["min_index_gap"] and has[n0 + idx]:
                    Tsearch = gt[n0 + idx]
                    ddx, ddy = Tposefrom[0] - Tsearch[0], Tposefrom[1] - Tsearch[1]
                    distance = math.sqrt((ddx * ddx + ddy * ddy) + 0.0)
                    if distance < nearest_loop_distance:
                        nearest_loop_distance = distance
                        close = idx
        r = out[i]
        r["diff"] = _terror(Tposefrom, Tposeto, c["guess_xyt"])
        r["closest_loop_distance"], r["candidate_loop_distance"], r["id_close"] = nearest_loop_distance, candidate_loop_distance, close
        r["close_xy"] = gt[n0 + close, :2]
        _flags(r, nearest_loop_distance, p)
    return out


def lap(n, seed, radius=20.0, laps=2.0):
    """n planar poses on `laps` turns of a noisy circle: later nodes pass close to earlier ones."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, 2.0 * math.pi * laps, n, endpoint=False)
    r = radius + rng.normal(0.0, 0.5, n)
    return np.stack([r * np.cos(a), r * np.sin(a), a + math.pi / 2 + rng.normal(0.0, 0.05, n)], 1)


def _tie_graph(n, near):
    """n nodes far away from the origin except `near` (node -> (x, y)); the last node sits at the origin."""
    g = np.stack([100.0 + np.arange(n), 50.0 + 0.0 * np.arange(n), 0.25 * np.ones(n)], 1)
    for k, xy in near.items():
        g[k, :2] = xy
    g[n - 1, :2] = (0.0, 0.0)
    return g


def stats_cases():
    """(graphs, has_gt, candidates, expected id_close of the tie candidates {candidate index: node})."""
    rng = np.random.default_rng(11)
    graphs, has, cands, ties = [], [], [], {}

    def add_graph(g, h=None):
        graphs.append(np.asarray(g, np.float64).reshape(-1, 3))
        has.append(np.ones(len(graphs[-1]), np.uint8) if h is None else np.asarray(h, np.uint8))
        return len(graphs) - 1

    def add(graph, fr, to, nr=0, guess=None, noise=(0.0, 0.0, 0.0)):
        g = graphs[graph]
        if guess is None:                                        # the true relative pose, perturbed
            c, s = math.cos(g[fr, 2]), math.sin(g[fr, 2])
            dx, dy = g[to, 0] - g[fr, 0], g[to, 1] - g[fr, 1]
            guess = (c * dx + s * dy + noise[0], c * dy - s * dx + noise[1], g[to, 2] - g[fr, 2] + noise[2])
        cands.append((graph, fr, to, nr, guess))
        return len(cands) - 1

    g0 = add_graph(lap(150, 3))
    for fr in (0, 10, 11, 12, 80, 149):
        add(g0, fr, max(fr - 11, 0), noise=(0.3, -0.2, 0.01))
    add(g0, 100, 100, guess=(0.0, 0.0, 0.0))                     # from == to, identity guess
    for nr, noise in enumerate(((0.1, 0.1, 0.001), (3.0, 3.5, 0.01), (0.5, 0.5, 0.2))):     # three guesses of one query
        add(g0, 140, 65, nr, noise=noise)
    add_graph(np.zeros((0, 3)))                                  # 0 and 1 nodes between others
    g1 = add_graph([[1.0, 2.0, 0.5]])
    add(g1, 0, 0, guess=(0.0, 0.0, 0.0))
    for n in (75, 76, 77):                                       # 64, 65 and 66 eligible nodes: the wave and its second stride
        g = add_graph(lap(n, 20 + n, laps=1.0))
        graphs[g][n - 12] = graphs[g][n - 1] + (0.5, 0.25, 0.0)  # the last eligible node is the nearest
        add(g, n - 1, n - 12, noise=(0.2, 0.1, 0.002))
        add(g, n - 1, 0)
    # equal distances: exact on these coordinates (9 + 16 = 16 + 9 = 25 + 0)
    g = add_graph(_tie_graph(140, {3: (3.0, 4.0), 20: (4.0, 3.0)}))                       # two, different lanes
    ties[add(g, 139, 20)] = 3
    g = add_graph(_tie_graph(140, {5: (5.0, 0.0), 69: (0.0, 5.0), 30: (-3.0, 4.0)}))       # three; 5 and 69 share a lane
    ties[add(g, 139, 69)] = 5
    g = add_graph(_tie_graph(140, {40: (3.0, 4.0), 70: (4.0, 3.0)}))                      # the lower index in the higher lane
    ties[add(g, 139, 70)] = 40
    g = add_graph(_tie_graph(200, {7: (0.0, -5.0), 71: (-5.0, 0.0), 135: (-4.0, -3.0)}))   # three in one lane's stride
    ties[add(g, 199, 7)] = 7
    # holes in has_gt, the nearest node among them; from / to without ground truth
    h = (rng.random(150) < 0.6).astype(np.uint8)
    h[[149, 148, 60]] = 1
    h[[74, 75, 120]] = 0
    g = add_graph(lap(150, 3), h)
    add(g, 149, 74, noise=(0.1, 0.0, 0.0))                       # to without ground truth
    add(g, 148, 60)
    add(g, 120, 30, noise=(0.0, 0.2, 0.0))                       # from without ground truth
    add(g, 149, 60, 1)
    off = np.concatenate([[0], np.cumsum([len(x) for x in graphs])]).astype(np.int64)
    arr = np.zeros(len(cands), L.LOOP_CANDIDATE_DTYPE)
    for i, c in enumerate(cands):
        arr[i] = (c[0], c[1], c[2], c[3], np.asarray(c[4], np.float64))
    return off, np.concatenate(graphs, 0), np.concatenate(has), arr, ties


# ---- curves --------------------------------------------------------------------------------------------------------------------
def clf_curve(y, s):
    """sklearn.metrics._ranking._binary_clf_curve for unit weights."""
    s = s + 0.0                                                  # -0.0 reads as 0.0
    o = np.argsort(-s, kind="stable")
    y, s = y[o], s[o]
    idx = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y.astype(np.float64))[idx]
    return 1 + idx - tps, tps, s[idx]


def trapezoid(y, x):
    return float((np.trapezoid if hasattr(np, "trapezoid") else np.trapz)(y, x))


def curves_one(y, s, ok=None, **par):
    """One experiment -> (dict of the six arrays, record fields) or None where the library refuses the experiment."""
    p = dict(CURVES_DEFAULTS, **par)
    y = np.asarray(y)
    s = np.asarray(s, np.float64)
    if y.size == 0 or (y > 1).any() or np.isnan(s).any() or y.sum() in (0, y.size):
        return None
    fps, tps, thr = clf_curve(y.astype(np.int64), s)
    rf, rt, rth = fps, tps, thr
    if p["drop_intermediate"] and fps.size > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        rf, rt, rth = fps[keep], tps[keep], thr[keep]
    rt, rf, rth = np.r_[0, rt], np.r_[0, rf], np.r_[np.inf, rth]
    fpr, tpr = rf / rf[-1], rt / rt[-1]
    precision = np.r_[(tps / (tps + fps))[::-1], 1.0]
    recall = np.r_[(tps / tps[-1])[::-1], 0.0]
    if p["reference_endpoints"]:                                 # 3_loop_closure.py:157,164-165
        tpr[-1] = tpr[-2]
        recall[0] = recall[1]
        precision[0] = precision[1]
    pred = s >= p["p_threshold"]
    yc = y.astype(bool) & ~(pred & (np.zeros(y.size, bool) if ok is None else np.asarray(ok) == 0))   # CorrectLabelForPosition
    tn, fp, fn, tp = int((~yc & ~pred).sum()), int((~yc & pred).sum()), int((yc & ~pred).sum()), int((yc & pred).sum())
    rec = dict(auc=trapezoid(tpr, fpr), accuracy=(tn + tp) / y.size, precision=tp / (tp + fp) if tp + fp else 0.0,
               recall=tp / (tp + fn) if tp + fn else 0.0, n_pos=int(y.sum()), n_neg=int(y.size - y.sum()), confusion=(tn, fp, fn, tp),
               n_thresholds=thr.size, n_roc=fpr.size, n_pr=precision.size, status=L.OK)
    return dict(roc_fpr=fpr, roc_tpr=tpr, roc_thr=rth, pr_precision=precision, pr_recall=recall, pr_thr=thr[::-1]), rec


CURVE_ARRAYS = ("roc_fpr", "roc_tpr", "roc_thr", "pr_precision", "pr_recall", "pr_thr")


def loop_curves_model(off, y, score, ok=None, **par):
    """cfear_loop_curves_batch in the layout api.loop_curves_flat returns: NaN where nothing is written."""
    n_exp = len(off) - 1
    arrays = {k: np.full(len(score) + n_exp, np.nan) for k in CURVE_ARRAYS}
    rec = np.zeros(n_exp, L.LOOP_CURVES_RESULT_DTYPE)
    for e in range(n_exp):
        a, b = int(off[e]), int(off[e + 1])
        got = curves_one(y[a:b], score[a:b], None if ok is None else ok[a:b], **par)
        if got is None:
            rec[e]["status"] = L.ERR_INVALID_ARGUMENT
            continue
        for k, v in got[0].items():
            arrays[k][a + e:a + e + v.size] = v
        for k, v in got[1].items():
            rec[e][k] = v
    return arrays, rec


CURVE_MODES = ("distinct", "decimal", "masked", "equal")


def curve_case(n, mode, seed=0, p_threshold=0.9):
    """(y, score, pos_ok) of n rows: all scores distinct; rounded to one decimal; half zeroed by a mask, with -0.0 among the
    zeros; all equal.  Both classes are present, one score equals p_threshold where the mode allows."""
    rng = np.random.default_rng([seed, n, CURVE_MODES.index(mode)])
    y = (rng.random(n) < 0.3).astype(np.uint8)
    y[0], y[-1] = 1, 0
    s = rng.random(n)
    ok = (rng.random(n) < 0.8).astype(np.uint8)
    if mode == "distinct":
        assert np.unique(s).size == n
    elif mode == "decimal":
        s = np.round(s, 1)
    elif mode == "masked":
        s = s * (rng.random(n) < 0.5)
        z = np.flatnonzero(s == 0.0)
        s[z[::2]] = -0.0
    else:
        s = np.full(n, 0.5)
    if mode in ("distinct", "masked") and n > 2:
        s[n // 2] = p_threshold
    return y, s, ok


# every size at which the kernel takes another path: the wave, the workgroup's tile, the LDS sort's limit, several chunks
CURVE_CASES = [(n, mode) for n in (2, 3, 5, 64, 65, 256, 257) for mode in CURVE_MODES] + [
    (LDS_ROWS - 1, "decimal"), (LDS_ROWS, "distinct"), (LDS_ROWS + 1, "masked"), (4 * LDS_ROWS + 3, "distinct"),
    (4 * LDS_ROWS + 3, "decimal")]


def curve_batch(cases):
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in cases])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(c[k], dt) for c in cases]) if cases else np.zeros(0, dt)
    return off, cat(0, np.uint8), cat(1, np.float64), cat(2, np.uint8)


# ---- a loop.csv-like table for LoopClosureEval ----------------------------------------------------------------------------------
def synthetic_table(seed=5, n_queries=40, nr_guess=3):
    """Rows of the four (odometry_coupled, raw, augment) combinations the eight settings need, nr_guess rows a query."""
    rng = np.random.default_rng(seed)
    cols = {k: [] for k in ("diff.x", "diff.y", "diff.z", "closest_loop_distance", "candidate_loop_distance", "id_from", "id_to",
                            "id_close", "guess_nr", "odom-bounds", "sc-sim", "alignment_quality", "SC - odometry_coupled_closure",
                            "Scan Context - raw_scan_context", "SC - augment_sc")}
    for coupled, raw, augment in ((0, 1, 0), (0, 0, 0), (0, 0, 1), (1, 0, 1)):
        for q in range(n_queries):
            closest = rng.uniform(0.0, 12.0)
            loop = closest < 6.0
            for g in range(nr_guess):
                close = rng.random() < (0.7 if loop else 0.2)
                scale = 1.0 if close else 8.0
                cols["diff.x"].append(rng.normal(0.0, scale))
                cols["diff.y"].append(rng.normal(0.0, scale))
                cols["diff.z"].append(rng.normal(0.0, 0.01 * scale))
                cols["closest_loop_distance"].append(closest)
                cols["candidate_loop_distance"].append(rng.uniform(0.0, 20.0))
                cols["id_from"].append(q + 20)
                cols["id_to"].append(q + 20 if q % 13 == 0 else int(rng.integers(0, q + 9)))
                cols["id_close"].append(int(rng.integers(0, q + 9)))
                cols["guess_nr"].append(g)
                cols["odom-bounds"].append(float(np.clip(rng.normal(0.7 if loop else 0.4, 0.2), 0.0, 1.0)))
                cols["sc-sim"].append(float(rng.normal(0.35 if loop and close else 0.6, 0.15)))
                cols["alignment_quality"].append(float(rng.normal(1.5 if loop and close else -1.0, 1.2)))
                cols["SC - odometry_coupled_closure"].append(coupled)
                cols["Scan Context - raw_scan_context"].append(raw)
                cols["SC - augment_sc"].append(augment)
    ints = ("id_from", "id_to", "id_close", "guess_nr", "SC - odometry_coupled_closure", "Scan Context - raw_scan_context", "SC - augment_sc")
    return {k: np.array(v, np.int64 if k in ints else np.float64) for k, v in cols.items()}
