"""CPU: covariance sampling on the device (cfear_cov_fit_records, cfear_covariance_by_sampling_candidates,
cfear_verify_sample_covariances) -- what can be checked without one.
  A  the three symbols declared, exported and built; the signature file compiled against the stand-ins;
  B  every refusal the calls decide on the host, with ctx = NULL, each with its message, the null context last, the outputs
     untouched.  (Pointers in different memories, and a candidate that names a scan outside its table, need a device:
     tests/test_gpu_covfit_device.py, tests/test_gpu_cov_candidates.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_cov_fit_records", "cfear_covariance_by_sampling_candidates", "cfear_verify_sample_covariances"]
INV = L.ERR_INVALID_ARGUMENT


# ---- A -------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_built():
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    hpp = open(os.path.join(ROOT, "include", "cfear_hip.hpp")).read()
    for s in NEW:
        assert s + "(" in hpp, s                                             # the thin mirrors call them
    for f in ("cov_fit_records", "covariance_by_sampling_candidates", "verify_sample_covariances"):
        assert callable(getattr(api, f))


def test_signature_file_compiles_and_refuses_without_a_gpu(tmp_path):
    exe = str(tmp_path / "covsample_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "covsample_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().splitlines()
    assert lines[0] == "%d samples_per_axis must be in [1,15]" % INV
    assert lines[1] == "%d null context" % INV
    assert lines[2] == "%d candidate 1: to must lie before from" % INV
    assert lines[3] == "%d null scan table: it must hold one entry per node (5)" % INV
    assert lines[4] == "%d null argument" % INV
    assert lines[5].split() == ["0.4", "0.0044", "3", "4"]


# ---- B -------------------------------------------------------------------------------------------------------------------
def _msg(lib):
    return lib.cfear_last_error(None).decode()


def test_fit_refusals_are_decided_before_the_context_is_needed():
    lib = L.lib()
    sp = api.n_scan_normal_reg.sampling_params()
    regs, samples = np.zeros(2, L.RESULT_DTYPE), np.zeros((2, 27), L.RESULT_DTYPE)
    cov, ok = np.full((2, 36), 7.0), np.full(2, 7, np.int32)

    def call(regs_=True, samples_=True, n=2, sp_=True, cov_=True, ok_=True):
        rc = lib.cfear_cov_fit_records(None, regs.ctypes.data if regs_ else None, samples.ctypes.data if samples_ else None, n,
                                       C.byref(sp) if sp_ else None, cov.ctypes.data if cov_ else None, ok.ctypes.data if ok_ else None)
        return rc, _msg(lib)

    for kw in (dict(regs_=False), dict(samples_=False), dict(sp_=False), dict(cov_=False), dict(ok_=False), dict(n=-1)):
        assert call(**kw) == (INV, "null argument"), kw
    for bad in (0, 16, -3):
        sp.samples_per_axis = bad
        assert call() == (INV, "samples_per_axis must be in [1,15]"), bad
        assert call(n=0) == (INV, "samples_per_axis must be in [1,15]")      # ... whatever the job count
    for good in (1, 15, 3):
        sp.samples_per_axis = good
        assert call() == (INV, "null context") and call(n=0) == (INV, "null context")
    assert (cov == 7.0).all() and (ok == 7).all()


def test_candidate_refusals_are_decided_before_the_context_is_needed():
    """Without a device there is no scan table; any address stands in for the handle: it is not looked at before the context."""
    lib = L.lib()
    sp = api.n_scan_normal_reg.sampling_params()
    par = L.RegParams()
    lib.cfear_reg_params_default(C.byref(par))
    table = np.zeros(64, np.uint8)
    cands, regs = np.zeros(3, L.CANDIDATE_DTYPE), np.zeros(3, L.RESULT_DTYPE)
    cov, ok = np.full((3, 36), 7.0), np.full(3, 7, np.int32)

    def call(table_=True, cands_=True, n=3, par_=True, regs_=True, sp_=True, cov_=True, ok_=True):
        rc = lib.cfear_covariance_by_sampling_candidates(None, table.ctypes.data if table_ else None, cands.ctypes.data if cands_ else None, n,
                                                         C.byref(par) if par_ else None, regs.ctypes.data if regs_ else None,
                                                         C.byref(sp) if sp_ else None, cov.ctypes.data if cov_ else None,
                                                         ok.ctypes.data if ok_ else None)
        return rc, _msg(lib)

    for kw in (dict(table_=False), dict(cands_=False), dict(regs_=False), dict(sp_=False), dict(cov_=False), dict(ok_=False), dict(n=-1)):
        assert call(**kw) == (INV, "null argument"), kw
    assert call(par_=False) == (INV, "null parameters")
    sp.samples_per_axis = 16
    assert call() == (INV, "samples_per_axis must be in [1,15]")
    sp.samples_per_axis = 3
    par.cost = 3
    assert call() == (INV, "bad cost/loss/weight option")
    par.cost = L.P2L
    par.radius = 0.0
    assert call() == (INV, "bad iteration limits / radius")
    par.radius = 2.0
    assert call() == (INV, "null context") and call(n=0, cands_=False) == (INV, "null context")
    assert (cov == 7.0).all() and (ok == 7).all()


class _Verified:
    """Three graphs of 2, 0 and 3 nodes, a verified list of three candidates and their records; ctx = NULL."""

    def __init__(self):
        self.lib = L.lib()
        self.par = api.loop_verify_params()
        self.node_off = np.array([0, 2, 2, 5], np.int32)
        self.poses = np.zeros((5, 3))
        self.g = L.LoopGraphs()
        self.g.n_graphs = 3
        self.g.node_off, self.g.poses_xyt = self.node_off.ctypes.data, self.poses.ctypes.data
        self.list = api.loop_verify_candidates([{"graph": 0, "from": 1, "to": 0}, {"graph": 2, "from": 2, "to": 0, "guess_nr": 1},
                                                {"graph": 2, "from": 2, "to": 1}])
        self.res = np.zeros(3, L.VERIFY_RESULT_DTYPE)
        self.res["reg_ok"] = 1
        self.res["cov"] = 0.25
        self.before = self.res.tobytes()

    def call(self, n=3, lst=True, res=True, g=True, par=True):
        rc = self.lib.cfear_verify_sample_covariances(None, C.byref(self.g) if g else None, self.list.ctypes.data if lst else None, n,
                                                      C.byref(self.par) if par else None, self.res.ctypes.data if res else None)
        return rc, self.lib.cfear_last_error(None).decode()


def test_verified_refusals_are_decided_before_the_context_is_needed():
    t = _Verified()
    TABLE = "null scan table: it must hold one entry per node (5)"
    assert t.call() == (INV, TABLE)                                          # nothing else wrong: refused for that, then for the context

    def refused(word, **kw):
        rc, msg = t.call(**kw)
        assert rc == INV and word in msg and msg != TABLE, (rc, msg)

    def with_(arr, idx, val, word):
        old = arr[idx].copy() if isinstance(arr[idx], np.ndarray) else arr[idx]
        arr[idx] = val
        refused(word)
        arr[idx] = old

    refused("null or negative argument", g=False)
    refused("null or negative argument", par=False)
    refused("null or negative argument", n=-1)
    t.g.n_graphs = -1
    refused("null or negative argument")
    t.g.n_graphs = 3
    t.g.node_off = None
    refused("node_off holds n_graphs + 1 entries")
    t.g.node_off = t.node_off.ctypes.data
    with_(t.node_off, 0, 1, "graph 0: node_off must start at 0")
    with_(t.node_off, 2, 1, "graph 1: node_off descends")
    t.g.poses_xyt = None
    refused("null poses_xyt with nodes")
    t.g.poses_xyt = t.poses.ctypes.data
    with_(t.poses, (3, 1), np.nan, "graph 2, node 1: a pose that is not finite")
    with_(t.poses, (1, 2), np.inf, "graph 0, node 1: a pose that is not finite")
    for bad in (0, 16):
        t.par.verify.sampling.samples_per_axis = bad
        refused("samples_per_axis must be in [1,15]")
    t.par.verify.sampling.samples_per_axis = 3
    refused("null list or results with a positive count", lst=False)
    refused("null list or results with a positive count", res=False)
    for field, j, val, word in (("graph", 1, 3, "candidate 1: its graph does not exist"), ("graph", 2, 1, "candidate 2: its from node does not exist"),
                                ("from", 0, 2, "candidate 0: its from node does not exist"), ("to", 2, -1, "candidate 2: its to node does not exist"),
                                ("to", 1, 2, "candidate 1: to must lie before from"), ("guess_nr", 2, -1, "candidate 2: guess_nr is negative"),
                                ("sc_sim", 1, np.nan, "candidate 1: its sc_sim is not finite"),
                                ("guess_xyt", 2, (0.0, np.inf, 0.0), "candidate 2: its guess is not finite")):
        with_(t.list[field], j, val, word)
    # a registered pose that is not finite is refused where the candidate takes part, and only there
    t.res["reg"]["pose"][1, 2] = np.nan
    refused("candidate 1: its registered pose is not finite")
    t.list["skip"][1] = 1
    assert t.call() == (INV, TABLE)
    t.list["skip"][1] = 0
    t.res["reg_ok"][1] = 0
    assert t.call() == (INV, TABLE)
    t.res["reg_ok"][1] = 1
    t.res["reg"]["pose"][1, 2] = 0.0
    # use_covariance_sampling is not read
    t.par.verify.use_covariance_sampling = 1
    assert t.call() == (INV, TABLE)
    t.par.verify.use_covariance_sampling = 0
    # nothing to sample: neither records nor a table are asked for, and the null context is what is left to refuse
    assert t.call(n=0, lst=False, res=False) == (INV, TABLE)
    t.g.n_graphs = 0
    assert t.call(n=0, lst=False, res=False) == (INV, "null context")
    assert t.res.tobytes() == t.before                                       # no refusal wrote a byte
