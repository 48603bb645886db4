"""CPU: loop candidates of batched graphs verified from the detector's rows (cfear_verify_sc_rows,
cfear_verify_graph_candidates) -- what can be checked without a device.
  A  the Python restatement of loopclosure.cpp:653-724 (tests/loop_rows_ref.py) on hand-made rows: the row mapping, the
     narrowing, the guess, the skip rule, the query and the odometry bound;
  B  every refusal the calls decide on the host, with ctx = NULL, each message naming its culprit; the outputs untouched;
  C  the symbols declared, exported and built, the records' layouts, and the C++ mirror compiled against the stand-ins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import loop_rows_ref as R
from oracle import pyoracle as O
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_loop_verify_params_default", "cfear_verify_graph_candidates", "cfear_verify_sc_rows"]


# ---- A -------------------------------------------------------------------------------------------------------------------
def _hand_rows():
    """Two graphs of 4 and 3 nodes detecting 3 and 3 of them, two records per row."""
    rows = np.zeros((6, 2), L.SC_CANDIDATE_DTYPE)
    n_out = np.array([0, 1, 2, 0, 0, 2], np.int32)

    def put(d, s, nn, md, mdo, yaw, taug):
        rows[d, s]["nn_idx"], rows[d, s]["min_dist"], rows[d, s]["min_dist_odom"] = nn, md, mdo
        rows[d, s]["yaw_diff_rad"], rows[d, s]["Taug"] = yaw, taug
    put(1, 0, 0, 0.1234567890123, 0.2, 0.3, (0.0, 2.0, 0.0))
    put(1, 1, 0, 9.0, 9.0, 9.0, (9.0, 9.0, 9.0))                      # past n_out[1]: ignored
    put(2, 0, 1, 0.3, 0.75, -1.5, (0.0, -4.0, 0.0))                   # over 0.7
    put(2, 1, 0, 0.4, 0.7, 0.25, (0.5, 0.0, 0.5))                     # exactly 0.7 is not over it
    put(5, 0, 1, 0.5, 0.1, 0.0, (0.0, 0.0, 0.0))
    put(5, 1, 0, 0.6, 0.9, 3.0, (0.0, 4.0, 0.0))
    node_off = np.array([0, 4, 7])
    rel = np.zeros((7, 3))
    rel[:, 0] = [1.0, 2.0, 40.0, 0.0, 3.0, 50.0, 0.0]
    rel[:, 2] = [0.1, -0.2, 0.3, 0.0, 0.5, 1.0, 0.0]
    return rows, n_out, node_off, np.array([3, 3]), rel


def test_restatement_maps_rows_to_candidates():
    rows, n_out, node_off, nd, rel = _hand_rows()
    c = R.rows_to_candidates(rows, n_out, node_off, nd, rel)
    assert [(x["graph"], x["from"], x["to"], x["guess_nr"]) for x in c] == [(0, 1, 0, 0), (0, 2, 1, 0), (0, 2, 0, 1), (1, 2, 1, 0), (1, 2, 0, 1)]
    assert [x["query"] for x in c] == [1, 2, 2, 6, 6]                       # one group per query node, flat over the batch
    assert not any(x["skip"] for x in c)                                    # speedup is off by default
    # the similarity is narrowed to float and widened again (:677)
    assert c[0]["sc_sim"] == float(np.float32(0.1234567890123)) != 0.1234567890123
    # Taug^-1 * Rz(yaw): a lateral shift of +2 m comes back as -2 m, the yaw is the float's value
    assert c[0]["guess_xyt"].tolist() == [0.0, -2.0, float(np.float32(0.3))]
    assert c[1]["guess_xyt"].tolist() == [0.0, 4.0, -1.5]
    g = O.xyt_compose(O.xyt_inverse(np.array([0.5, 0.0, 0.5])), np.array([0.0, 0.0, 0.25]))
    assert c[2]["guess_xyt"].tolist() == g.tolist() and g[2] == -0.25
    # VerifyByOdometry over rel[to .. from - 1] of the candidate's own graph
    assert c[0]["odom_bounds"] == O.verify_by_odometry(rel[0:1])
    assert c[2]["odom_bounds"] == O.verify_by_odometry(rel[0:2])
    assert c[3]["odom_bounds"] == O.verify_by_odometry(rel[5:6]) and c[3]["odom_bounds"] > 0.99     # 50 m in one step
    assert c[4]["odom_bounds"] == O.verify_by_odometry(rel[4:6])


def test_restatement_guess_skip_and_odometry_switches():
    rows, n_out, node_off, nd, rel = _hand_rows()
    c = R.rows_to_candidates(rows, n_out, node_off, nd, rel, transl_guess=False, speedup=True)
    assert [x["skip"] for x in c] == [0, 1, 0, 0, 1]                        # 0.75 and 0.9 are over 0.7; 0.7 is not
    assert c[0]["guess_xyt"].tolist() == [0.0, 0.0, float(np.float32(0.3))]
    # a skipped row reports min_dist unnarrowed and min_dist_odom as its odometry term (:684), and has no odometry bound
    assert c[1]["sc_sim"] == 0.3 and c[1]["odom_term"] == 0.75 and c[1]["odom_bounds"] is None
    assert c[4]["sc_sim"] == 0.6 and c[4]["sc_sim"] != float(np.float32(0.6))
    rec = R.skipped_record(c[1])
    assert rec["alignment_quality"] == -20.0 and rec["odom_bounds"] == 0.75 and rec["rank"] == -1 and not rec["accepted"]
    # the rule needs odometry_coupled_closure as well (:682)
    assert not any(x["skip"] for x in R.rows_to_candidates(rows, n_out, node_off, nd, rel, speedup=True, odometry_coupled_closure=False))
    off = R.rows_to_candidates(rows, n_out, node_off, nd, None, verify_via_odometry=False)
    assert [x["odom_bounds"] for x in off] == [1.0] * 5
    # n_detect defaults to every node: the second graph's rows then start at row 4
    c = R.rows_to_candidates(np.concatenate([rows, rows[:1]]), np.array([0, 1, 2, 0, 0, 0, 2], np.int32), node_off, None, rel)
    assert [(x["graph"], x["from"]) for x in c] == [(0, 1), (0, 2), (0, 2), (1, 2), (1, 2)]


# ---- B -------------------------------------------------------------------------------------------------------------------
class _Batch:
    """Three graphs of 2, 0 and 3 nodes as flat host tables, a candidate list and detector rows; ctx = NULL."""

    def __init__(self):
        self.lib = L.lib()
        self.par = api.loop_verify_params()
        self.node_off = np.array([0, 2, 2, 5], np.int32)
        self.peak_off = np.array([0, 3, 3, 7, 8, 12], np.int64)
        self.xyzi = np.zeros((12, 4), np.float32)
        self.poses = np.zeros((5, 3))
        self.rel = np.zeros((5, 3))
        self.g = L.LoopGraphs()
        self.g.n_graphs = 3
        for name, arr in (("node_off", self.node_off), ("peak_off", self.peak_off), ("peaks_xyzi", self.xyzi), ("poses_xyt", self.poses),
                          ("rel_xyt", self.rel)):
            setattr(self.g, name, arr.ctypes.data)
        self.cands = api.loop_verify_candidates([{"graph": 0, "from": 1, "to": 0}, {"graph": 2, "from": 2, "to": 0, "guess_nr": 1},
                                                 {"graph": 2, "from": 2, "to": 1}])
        self.n_detect = np.array([2, 0, 3], np.int32)
        self.rows = np.zeros((5, 3), L.SC_CANDIDATE_DTYPE)
        self.n_out = np.array([0, 1, 0, 1, 2], np.int32)
        self.rows[4, 1]["nn_idx"] = 1
        self.res = np.full(15 * 480, 0x5A, np.uint8)
        self.lst = np.full(15 * 64, 0x5A, np.uint8)
        self.loops = np.full(15 * 40, 0x5A, np.uint8)
        self.n = C.c_int32(-7)

    def list_call(self, n=3, cands=True, res=True):
        rc = self.lib.cfear_verify_graph_candidates(None, C.byref(self.g), self.cands.ctypes.data if cands else None, n, C.byref(self.par),
                                                    self.res.ctypes.data if res else None, self.lst.ctypes.data, self.loops.ctypes.data)
        return rc, self.lib.cfear_last_error(None).decode()

    def rows_call(self, rows=True, n_out=True, nc=3, res=True):
        rc = self.lib.cfear_verify_sc_rows(None, C.byref(self.g), self.rows.ctypes.data if rows else None,
                                           self.n_out.ctypes.data if n_out else None, self.n_detect.ctypes.data, nc, C.byref(self.par),
                                           self.res.ctypes.data if res else None, self.lst.ctypes.data, self.loops.ctypes.data, C.byref(self.n))
        return rc, self.lib.cfear_last_error(None).decode()


def test_refusals_are_decided_before_the_context_is_needed():
    t = _Batch()
    INV = L.ERR_INVALID_ARGUMENT
    # without a device there is no scan table: a batch with nothing else wrong is refused for that, after everything else
    TABLE = "null scan table: it must hold one entry per node (5)"
    assert t.list_call() == (INV, TABLE) and t.rows_call() == (INV, TABLE)

    def refused(word, call=None, **kw):
        for c in ([call] if call else [t.list_call, t.rows_call]):
            rc, msg = c(**kw)
            assert rc == INV and word in msg and msg != TABLE, (rc, msg)

    def with_(arr, idx, val, word, call=None):
        old = arr[idx].copy() if isinstance(arr[idx], np.ndarray) else arr[idx]
        arr[idx] = val
        refused(word, call)
        arr[idx] = old

    # the graphs
    with_(t.node_off, 0, 1, "graph 0: node_off must start at 0")
    with_(t.node_off, 2, 1, "graph 1: node_off descends")
    with_(t.peak_off, 0, 1, "graph 0, node 0: peak_off must start at 0")
    with_(t.peak_off, 4, 2, "graph 2, node 1: peak_off descends")
    with_(t.poses, (3, 1), np.nan, "graph 2, node 1: a pose that is not finite")
    with_(t.poses, (1, 2), np.inf, "graph 0, node 1: a pose that is not finite")
    with_(t.rel, (2, 0), np.nan, "graph 2, node 0: a relative motion that is not finite")
    for last in (1, 4):                                                    # the entry of a graph's last node is ignored
        t.rel[last, 0] = np.nan
        assert t.list_call()[1] == TABLE
        t.rel[last, 0] = 0.0
    for name, word in (("node_off", "node_off holds n_graphs + 1 entries"), ("peak_off", "null peak_off or poses_xyt"),
                       ("poses_xyt", "null peak_off or poses_xyt"), ("rel_xyt", "rel_xyt may be null only with verify_via_odometry = 0"),
                       ("peaks_xyzi", "null peaks_xyzi with points")):
        old = getattr(t.g, name)
        setattr(t.g, name, None)
        refused(word)
        setattr(t.g, name, old)
    t.par.verify_via_odometry = 0                                          # ... and then rel_xyt is not looked at
    t.g.rel_xyt = None
    assert t.list_call()[1] == TABLE and t.rows_call()[1] == TABLE
    t.par.verify_via_odometry = 1
    t.g.rel_xyt = t.rel.ctypes.data
    t.g.n_graphs = -1
    refused("null or negative argument")
    t.g.n_graphs = 3
    # the parameters
    t.par.verify.use_covariance_sampling = 1
    refused("use_covariance_sampling is not available")
    t.par.verify.use_covariance_sampling = 0
    t.par.odom_sigma_error = float("nan")
    refused("odom_sigma_error is NaN")
    t.par.odom_sigma_error = 0.03
    # the candidate list
    for field, j, val, word in (("graph", 1, 3, "candidate 1: its graph does not exist"), ("graph", 0, -1, "candidate 0: its graph does not exist"),
                                ("graph", 2, 1, "candidate 2: its from node does not exist"),         # graph 1 has no nodes
                                ("from", 0, 2, "candidate 0: its from node does not exist"), ("to", 2, -1, "candidate 2: its to node does not exist"),
                                ("to", 1, 3, "candidate 1: its to node does not exist"), ("to", 1, 2, "candidate 1: to must lie before from"),
                                ("guess_nr", 2, -1, "candidate 2: guess_nr is negative"), ("sc_sim", 1, np.nan, "candidate 1: its sc_sim is not finite"),
                                ("guess_xyt", 2, (0.0, np.inf, 0.0), "candidate 2: its guess is not finite")):
        with_(t.cands[field], j, val, word, t.list_call)
    refused("null candidates with a positive count", t.list_call, cands=False)
    refused("null results with candidates", res=False)
    refused("null or negative argument", t.list_call, n=-1)
    # the rows
    with_(t.n_detect, 2, 4, "graph 2: n_detect 4 outside [0, 3]", t.rows_call)
    with_(t.n_detect, 0, -1, "graph 0: n_detect -1 outside [0, 2]", t.rows_call)
    with_(t.n_out, 3, 4, "graph 2, node 1: n_out 4 outside [0, 3]", t.rows_call)
    with_(t.n_out, 1, -1, "graph 0, node 1: n_out -1 outside [0, 3]", t.rows_call)
    with_(t.n_out, 2, 1, "graph 2, node 0: candidate 0 names a node that is not before its query", t.rows_call)
    with_(t.rows["nn_idx"], (4, 1), 2, "graph 2, node 2: candidate 1 names a node that is not before its query", t.rows_call)
    with_(t.rows["Taug"], (3, 0), (0.0, np.nan, 0.0), "graph 2, node 1: candidate 0 is not finite", t.rows_call)
    with_(t.rows["min_dist"], (4, 0), np.inf, "graph 2, node 2: candidate 0 is not finite", t.rows_call)
    t.rows[4, 2]["nn_idx"] = 77                                            # records past n_out are not looked at
    assert t.rows_call()[1] == TABLE
    refused("null rows or n_out", t.rows_call, rows=False)
    refused("null rows or n_out", t.rows_call, n_out=False)
    refused("n_candidates must be at least 1", t.rows_call, nc=0)
    rc = t.lib.cfear_verify_sc_rows(None, C.byref(t.g), t.rows.ctypes.data, t.n_out.ctypes.data, t.n_detect.ctypes.data, 3, C.byref(t.par),
                                    t.res.ctypes.data, None, None, None)
    assert rc == INV and "null n_list" in t.lib.cfear_last_error(None).decode()
    assert t.lib.cfear_verify_graph_candidates(None, None, None, 0, C.byref(t.par), None, None, None) == INV
    assert t.lib.cfear_verify_graph_candidates(None, C.byref(t.g), None, 0, None, None, None, None) == INV
    # nothing to verify: neither outputs nor a table are asked for, and the null context is what is left to refuse
    assert t.list_call(n=0, cands=False, res=False) == (INV, TABLE)
    t.g.n_graphs = 0
    assert t.list_call(n=0, cands=False, res=False) == (INV, "null context")
    assert t.rows_call(rows=False, n_out=False, res=False) == (INV, "null context")
    # no refusal wrote a byte
    assert (t.res == 0x5A).all() and (t.lst == 0x5A).all() and (t.loops == 0x5A).all() and t.n.value in (-7, 0)


# ---- C -------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_built_and_layouts():
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert C.sizeof(L.LoopGraphs) == 56 and C.sizeof(L.LoopVerifyParams) == 184 and L.LOOP_VERIFY_CANDIDATE_DTYPE.itemsize == 64
    assert [(n, getattr(L.LoopGraphs, n).offset) for n, _ in L.LoopGraphs._fields_] == [
        ("n_graphs", 0), ("pad", 4), ("node_off", 8), ("table", 16), ("peaks_xyzi", 24), ("peak_off", 32), ("poses_xyt", 40), ("rel_xyt", 48)]
    d = L.LOOP_VERIFY_CANDIDATE_DTYPE
    assert [(n, d.fields[n][1]) for n in d.names] == [("graph", 0), ("from", 4), ("to", 8), ("guess_nr", 12), ("query", 16), ("skip", 20),
                                                      ("guess_xyt", 24), ("sc_sim", 48), ("odom_term", 56)]
    for struct, mirror in (("cfear_loop_graphs", [n for n, _ in L.LoopGraphs._fields_]), ("cfear_loop_verify_candidate", list(d.names)),
                           ("cfear_loop_verify_params", [n for n, _ in L.LoopVerifyParams._fields_])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")
                 for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", line.strip().replace("*", " "))]
        assert names == mirror, struct
    p = api.loop_verify_params()
    assert (p.odom_sigma_error, p.verify_via_odometry, p.transl_guess, p.speedup, p.odometry_coupled_closure) == (0.03, 1, 1, 0, 1)
    assert p.verify.model_threshold == 0.8 and L.LOOP_SPEEDUP_ODOM == R.SPEEDUP_ODOM
    assert "#define CFEAR_LOOP_SPEEDUP_ODOM 0.7" in hdr and lib.cfear_abi_version() == 1
    assert api.loop_verify_params(speedup=1, model_threshold=0.5).verify.model_threshold == 0.5


def test_cpp_mirror_compiles_and_refuses_without_a_gpu(tmp_path):
    exe = str(tmp_path / "loop_verify_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "loop_verify_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().splitlines()
    INV = str(L.ERR_INVALID_ARGUMENT)
    assert lines[0] == INV + " candidate 1: to must lie before from"
    assert lines[1] == INV + " graph 0: n_detect 3 outside [0, 2]"
    assert lines[2] == INV + " null scan table: it must hold one entry per node (5)"
    assert lines[3].split() == ["0.03", "1", "1", "0", "1", "0.7"]
