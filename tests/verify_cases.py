"""The loop-candidate verification matrix: a pool of about two dozen distinct candidates over one five-node scene (plus dense
nodes), each with the CPU oracle's answer computed ONCE, and tile(), which repeats the pool into batches of any length.  Shared
by tests/test_gpu_verify_matrix.py; the CPU-only checks of what the pool is meant to contain live in Pool.check().

  nodes        oracle k-strongest -> peaks -> cells of synth.scene_v1(3, 5), as tests/test_gpu_verify.py::nodes, plus
               node 5 / 6 = node 4 / 0 with an EMPTY peak cloud and node 7 = node 1 with its cells 500 m away in its own frame
               (no registration and no CFEAR cost with any partner at any guess)
  dense nodes  ~1 600 cells (synth.scene_dense, as tests/test_gpu_register.py::_dense_cells) and 3 000 cells (three dense
               worlds side by side, the construction of test_large_registrations_on_every_form)
  predict_hint a restatement of the launch-hint thresholds (JobSizes::add over mt_fit, csrc/reg_layout.hpp) -- used ONLY to
               choose inputs; the GPU tests assert what the library reports (profile names, reg["reserved"]).
               tests/test_reg_layout_cpu.py holds _mt_fit and predict_hint to the header itself, on the CPU: for every
               max_cells from 0 to 3200, cost and loss, against a stand-alone program that includes reg_layout.hpp."""
import numpy as np

RANGE_RES = 0.0438

# ---- the launch hint of a two-scan batch whose largest scan holds max_cells cells (cfear_reg_pair_geometry) ------------------
K_LDS_CU, K_LDS_PAIRS = 160 * 1024, 20 * 1024
K_FIXED_LDS, K_PTRS, K_START_PAD, K_PART_BIG = 1792, 6, 32 * 32 + 8, 10 * 4 * 16 * 8
DENSE_FIELDS = {"P2P": 3, "P2L": 5, "P2D": 6}


def _mt_fit(lds_total, last, sum_pad, max_pad, n_src, fields, allow_gmatch):
    """mt_fit -> (can, good)."""
    off = K_FIXED_LDS + last * (12 * 8 + K_PTRS * 8 + 16) + (((last + 1) * 4 + 15) & ~15)
    off += n_src * 16
    n_pairs = last * n_src
    match_bytes = ((n_pairs + 7) & ~7) * 2
    need_one = K_START_PAD * 2 + max_pad * 10
    gmatch = allow_gmatch and ((off + match_bytes + 15) & ~15) + need_one > lds_total
    if not gmatch:
        off += match_bytes
    off = (off + 15) & ~15
    tables_all = last * K_START_PAD * 2 + sum_pad * 10
    per = fields * 8 + 2
    can = sum_pad <= 65535 and n_src < 65536 and off + need_one <= lds_total and off + 4096 <= lds_total
    region = lds_total - off if can else 0
    dense_all = ((n_pairs + 3) & ~3) * per
    resident = can and tables_all + dense_all + 16 <= region
    dense_cap = ((n_pairs + 3) & ~3) if resident else (region // per) & ~3
    good = can and (resident or (tables_all <= 2 * region and 5 * dense_cap >= 2 * n_pairs))
    return can, good


def predict_hint(max_cells, cost="P2L", huber=True):
    """RegLaunchHint of verify_device_chain for a batch whose largest scan has max_cells cells: dict(small_pairs, big_pass,
    whole_cu)."""
    pad = (max_cells + 7) & ~7
    fields = DENSE_FIELDS[cost]
    regular = K_LDS_CU // 4 if huber else (K_LDS_CU // 3) & ~255
    return dict(whole_cu=not _mt_fit(K_LDS_CU // 2 - 256 - K_PART_BIG, 1, pad, pad, max_cells, fields, True)[0],
                small_pairs=_mt_fit(K_LDS_PAIRS, 1, pad, pad, max_cells, fields, False)[1],
                big_pass=not _mt_fit(regular, 1, pad, pad, max_cells, fields, False)[1])


def coral_scratch_bytes(cap):
    """coral_scratch_bytes (csrc/coral.hip): 48 bytes per merged point of the batch's largest job, rounded up to 256."""
    return (cap * 48 + 255) // 256 * 256


def coral_chunk(cap):
    """Jobs per CorAl launch: the scratch of one launch is bounded to 1 GiB (coral_launch)."""
    return max(1, (1 << 30) // coral_scratch_bytes(cap))


# ---- nodes ---------------------------------------------------------------------------------------------------------------
def _node(img, T, radius=3.0, rr=RANGE_RES):
    from oracle import pyoracle as O
    sr, si, cnt = O.kstrongest(img, 40, 60)
    pk = O.peaks(img, 40, sr, cnt)
    cells = O.surface_points(O.kstrongest_cloud(sr, si, cnt, rr, 2.5), radius, 1.0, weight_intensity=True)
    peaks = np.ascontiguousarray(O.kstrongest_cloud(sr, si, cnt, rr, 2.5, mask=pk), dtype=np.float32)
    return dict(cells=cells, peaks=peaks, T=np.asarray(T, np.float64))


def base_nodes():
    from tbv_slam_public_amd import synth
    imgs, gt, sc = synth.scene_v1(3, 5)
    nodes = [_node(imgs[f], gt[f], rr=float(sc.range_res)) for f in range(5)]
    empty = np.zeros((0, 4), np.float32)
    nodes.append(dict(nodes[4], peaks=empty))                                    # 5
    nodes.append(dict(nodes[0], peaks=empty.copy()))                             # 6
    away = nodes[1]["cells"].copy()
    away["mean"][:, 0] += 500.0
    nodes.append(dict(nodes[1], cells=away))                                     # 7
    return nodes


def dense_nodes():
    """[0..2]: ~1 600 cells each (big_pass); [3], [4]: 3 000 cells, three dense worlds side by side (whole_cu: a pair's tables
    and source means no longer fit half a CU's LDS).  Peak clouds thinned: a pair's merged cloud stays far below
    cfear_coral_max_points()."""
    from oracle import pyoracle as O
    from tbv_slam_public_amd import synth
    imgs, gt, _ = synth.scene_dense(7, 3)
    nodes = [_node(imgs[f], gt[f]) for f in range(3)]
    worlds = [synth.scene_dense(seed, 2) for seed in (9, 10, 11)]
    for f in range(2):
        parts = []
        for w, (im, _, _) in enumerate(worlds):
            sr, si, cnt = O.kstrongest(im[f], 40, 60)
            c = O.surface_points(O.kstrongest_cloud(sr, si, cnt, RANGE_RES, 2.5), 2.5, 1.0, (0, 0), True).copy()
            c["mean"][:, 0] += 600.0 * w
            parts.append(c[:1000])
        nd = _node(worlds[0][0][f], worlds[0][1][f])
        nodes.append(dict(nd, cells=np.concatenate(parts)))
    for nd in nodes:
        nd["peaks"] = np.ascontiguousarray(nd["peaks"][::3])
    return nodes


def attach_scans(nodes, ctx=None):
    """One MapPointNormal per distinct cell array (needs the GPU) -> new node dicts with "scan"."""
    from tbv_slam_public_amd import api
    scans = {}
    out = []
    for nd in nodes:
        key = id(nd["cells"])
        if key not in scans:
            scans[key] = api.MapPointNormal(cells=nd["cells"], ctx=ctx)
        out.append(dict(nd, scan=scans[key]))
    return out


# ---- candidates ------------------------------------------------------------------------------------------------------------
def cand(nodes, f, t, err, sc_sim, odom_bounds, from_pose=None, name=""):
    """Candidate f -> t whose guess is the true relative pose plus err, with the query node at from_pose (its own by default)."""
    from oracle import pyoracle as O
    t_true = O.xyt_compose(O.xyt_inverse(nodes[f]["T"]), nodes[t]["T"])
    return dict(f=f, t=t, t_be_guess=t_true + np.asarray(err, np.float64), sc_sim=float(sc_sim), odom_bounds=float(odom_bounds),
                from_pose=np.asarray(nodes[f]["T"] if from_pose is None else from_pose, np.float64), name=name)


def oracle_answer(nodes, c, sampling=False):
    from oracle import pyoracle as O
    return O.verify_loop_candidate(nodes[c["f"]]["cells"], nodes[c["f"]]["peaks"], c["from_pose"], nodes[c["t"]]["cells"],
                                   nodes[c["t"]]["peaks"], c["t_be_guess"], c["sc_sim"], c["odom_bounds"],
                                   use_covariance_sampling=sampling)


def revised_yaw(c, e):
    """Yaw of Trevised = Tto * Talign^-1 (the covariance is rotated by its inverse, loopclosure.cpp:93)."""
    return float(c["from_pose"][2] + c["t_be_guess"][2] - e["t_be"][2])


def base_cands(nodes):
    far_a, far_b, far_c = (2500.0, -1800.0, 3.6), (-1200.0, 900.0, -2.5), (4000.0, 3000.0, -3.9)
    return [
        # the six of tests/test_gpu_verify.py::_candidates
        cand(nodes, 4, 0, (0.5, -0.4, 0.03), 0.15, 0.0, name="good 4-0"),
        cand(nodes, 4, 1, (-0.3, 0.2, -0.02), 0.25, 0.1, name="good 4-1"),
        cand(nodes, 4, 2, (9.0, 6.0, 0.6), 0.30, 0.0, name="wrong guess"),
        cand(nodes, 3, 0, (0.2, 0.1, 0.01), 0.10, 0.0, name="good 3-0"),
        cand(nodes, 3, 1, (400.0, 0.0, 0.0), 0.10, 0.0, name="no overlap"),
        cand(nodes, 2, 0, (0.0, 0.0, 0.0), 0.40, 0.9, name="features disagree"),
        # the query node far from the origin and turned: Talign and R C R^T away from the identity
        cand(nodes, 4, 0, (0.3, -0.2, 0.02), 0.05, 0.0, from_pose=far_a, name="far a, yaw 3.6"),
        cand(nodes, 3, 1, (-0.2, 0.3, -0.01), 0.05, 0.0, from_pose=far_b, name="far b, yaw -2.5"),
        cand(nodes, 2, 0, (0.1, 0.1, 0.01), 0.02, 0.0, from_pose=far_c, name="far c, yaw -3.9"),
        cand(nodes, 4, 3, (0.2, 0.0, 0.0), 0.05, 0.0, from_pose=(0.0, 0.0, 1.2), name="yaw 1.2"),
        cand(nodes, 1, 0, (0.0, 0.3, 0.02), 0.05, 0.0, from_pose=(150.0, 80.0, -0.9), name="yaw -0.9"),
        cand(nodes, 3, 1, (400.0, 0.0, 0.0), 0.10, 0.0, from_pose=far_a, name="no overlap, far"),
        # empty peak clouds
        cand(nodes, 5, 0, (0.5, -0.4, 0.03), 0.15, 0.0, name="empty from_peaks"),
        cand(nodes, 4, 6, (0.5, -0.4, 0.03), 0.15, 0.0, name="empty to_peaks"),
        # the echoed features at their ends
        cand(nodes, 4, 0, (0.1, 0.1, 0.0), 0.0, 0.0, name="sc 0 ob 0"),
        cand(nodes, 4, 0, (0.1, 0.1, 0.0), 1.0, 0.0, name="sc 1 ob 0"),
        cand(nodes, 4, 0, (0.1, 0.1, 0.0), 0.0, 1.0, name="sc 0 ob 1"),
        cand(nodes, 4, 0, (0.1, 0.1, 0.0), 1.0, 1.0, name="sc 1 ob 1"),
        # nothing to register against and nothing to score: cells 500 m away in the candidate's own frame
        cand(nodes, 3, 7, (0.2, 0.1, 0.01), 0.10, 0.0, name="cells away"),
        # more of the ordinary kind, other pairs and guesses
        cand(nodes, 2, 1, (0.4, 0.4, -0.03), 0.12, 0.05, name="good 2-1"),
        cand(nodes, 1, 0, (-0.6, 0.1, 0.02), 0.20, 0.0, name="good 1-0"),
        cand(nodes, 3, 2, (0.0, -0.5, 0.04), 0.08, 0.2, name="good 3-2"),
        cand(nodes, 0, 4, (0.3, 0.3, 0.0), 0.18, 0.0, name="good 0-4"),
        cand(nodes, 4, 0, (3.0, -2.0, 0.15), 0.10, 0.0, name="loose guess"),
    ]


def dense_cands(nodes, off=0):
    """(big_pass candidates over the ~1 600-cell nodes, the whole_cu candidate over the 3 000-cell ones); the dense nodes start
    at nodes[off]."""
    return ([cand(nodes, off + 1, off + 0, (0.3, -0.2, 0.008), 0.1, 0.0, name="dense 1-0"),
             cand(nodes, off + 2, off + 1, (-0.2, 0.1, -0.005), 0.1, 0.0, name="dense 2-1")],
            [cand(nodes, off + 4, off + 3, (0.25, -0.15, 0.006), 0.1, 0.0, name="huge 4-3")])


class Pool:
    """nodes + distinct candidates + the oracle's answer to each, computed on first use and kept."""

    def __init__(self, nodes, cands):
        self.nodes, self.cands = nodes, cands
        self._exp = {}

    def __len__(self):
        return len(self.cands)

    def expected(self, sampling=False):
        if sampling not in self._exp:
            self._exp[sampling] = [oracle_answer(self.nodes, c, sampling) for c in self.cands]
        return self._exp[sampling]

    def check(self):
        """What the base pool is meant to contain, from the oracle alone."""
        exp = self.expected(False)
        failed = [e for e in exp if not e["reg_ok"]]
        assert failed and all((e["t_be"] == 0).all() and (e["cov"] == np.eye(6)).all() for e in failed)
        assert any((e["cfear"] == 0).all() for e in exp) and any((e["cfear"] != 0).all() for e in failed)
        assert sum(e["reg_ok"] for e in exp) >= 18
        yaws = [abs(c["from_pose"][2]) for c in self.cands]
        assert max(yaws) > np.pi and max(np.hypot(c["from_pose"][0], c["from_pose"][1]) for c in self.cands) > 1000.0
        assert any(len(self.nodes[c["f"]]["peaks"]) == 0 for c in self.cands) and any(len(self.nodes[c["t"]]["peaks"]) == 0 for c in self.cands)
        assert {(c["sc_sim"], c["odom_bounds"]) for c in self.cands} >= {(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)}
        p = np.array([e["probability"] for e in exp])
        assert (p > 0.8).sum() >= 6 and (p < 0.8).sum() >= 6 and np.abs(p - 0.8).min() > 1e-3      # no candidate on the threshold

    def check_sampling(self):
        """Issue 6: some accepted candidate has |inverse yaw| > 0.5 rad and a sampled covariance whose x and y variances differ
        by more than 10 %, else R C R^T is not under test."""
        hits = [c["name"] for c, e in zip(self.cands, self.expected(True))
                if e["cov_sampled"] and e["probability"] > 0.8 and abs(np.remainder(revised_yaw(c, e) + np.pi, 2 * np.pi) - np.pi) > 0.5
                and abs(e["cov"][0, 0] - e["cov"][1, 1]) > 0.1 * max(e["cov"][0, 0], e["cov"][1, 1])]
        assert hits
        return hits


def tile(pool, n, groups="cycle", seed=0):
    """n candidates that cycle over the pool -> (cands with "group", pool index of each).  groups: "cycle" = one query per pool
    cycle (grouped, ascending); "shuffled" = the same ids in random order; or a sequence of n ids."""
    idx = np.arange(n) % len(pool)
    if isinstance(groups, str):
        g = np.arange(n) // len(pool)
        if groups == "shuffled":
            g = np.random.default_rng(seed).permutation(g) - 3
        else:
            assert groups == "cycle"
    else:
        g = np.asarray(groups)
        assert g.shape == (n,)
    return [dict(pool.cands[i], group=int(q)) for i, q in zip(idx, g)], idx


def make_jobs(nodes, cands, peaks_on="host", overrides=None):
    """Job dicts for api.verify_loop_candidates.  Each distinct peak cloud is ONE host array or ONE device tensor shared by all
    its copies ("mixed": the even nodes' clouds on the device).  overrides: {job index: dict of job keys to replace}."""
    dev = {}

    def pk(i):
        if peaks_on == "host" or (peaks_on == "mixed" and i % 2 == 1):
            return nodes[i]["peaks"]
        if i not in dev:
            import torch
            dev[i] = torch.from_numpy(np.ascontiguousarray(nodes[i]["peaks"])).cuda()
        return dev[i]
    jobs = [dict(from_scan=nodes[c["f"]]["scan"], to_scan=nodes[c["t"]]["scan"], from_peaks=pk(c["f"]), to_peaks=pk(c["t"]),
                 from_pose=c["from_pose"], t_be_guess=c["t_be_guess"], sc_sim=c["sc_sim"], odom_bounds=c["odom_bounds"],
                 group=c["group"]) for c in cands]
    for j, o in (overrides or {}).items():
        jobs[j] = dict(jobs[j], **o)
    return jobs
