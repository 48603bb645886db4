"""CPU: what the vicinity-closure call (cfear_closure_candidates_batch, csrc/closure.hip) needs no device for -- the Python
model it is compared with on the GPU (tests/closure_cpu.py) against a literal O(N^3) transcription of the reference's loop,
the laps the GPU tests use, the ABI, the defaults, the argument refusals (they are made before a context is needed) and the
marshalling of api.closure_candidates."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closure_cpu as M
from tbv_slam_public_amd import _lib as L
from tbv_slam_public_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,circumference,thr", [(120, 100.0, M.DEFAULTS["gtvicinity"]), (97, 20.0, M.SMALL), (64, 20.0, M.SMALL),
                                                 (33, 20.0, dict(M.SMALL, min_d_travel=0.0))])
def test_model_equals_the_cubic_transcription(n, circumference, thr):
    pos, steps, _ = M.lap(n, M.LAP_SEED, circumference)
    a, b = M.candidates(pos, steps, "gtvicinity", **thr), M.gtvicinity_cubic(pos, steps, **thr)
    assert a.tobytes() == b.tobytes()
    assert 0 < (a["to"] >= 0).sum() < n


def test_model_on_duplicates_and_zero_steps():
    """min_d_travel = 0 with repeated poses and zero steps: 0/0 and x/0 never win, in the model as in the transcription."""
    pos = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [0.5, 0, 0]], np.float64)
    steps = np.array([0.0, 0.0, 0.0, 1.0, 0.0])
    thr = dict(min_d_travel=0.0, max_d_travel=10.0, max_d_close=5.0)
    a = M.candidates(pos, steps, "gtvicinity", **thr)
    assert a.tobytes() == M.gtvicinity_cubic(pos, steps, **thr).tobytes()
    assert a["to"].tolist() == [4, 4, 4, 4, -1] and a["rel"][0] == 0.5 and a["rel"][2] == 0.5
    m = M.candidates(pos, steps, "mini", **thr)
    assert m["to"].tolist() == a["to"].tolist() and not m["exhausted"].any()


def test_lap_counts():
    """The laps the GPU tests sweep: every case has origins with and without a candidate."""
    for n, want, exhausted in ((300, 215, 0), (700, 615, 249)):
        pos, steps, rel = M.lap(n, M.LAP_SEED)
        assert (pos * 8 == np.round(pos * 8)).all() and steps[-1] == 0.0 and (steps[:-1] > 0).all()
        for mode in ("gtvicinity", "mini"):
            c = M.candidates(pos, steps, mode, **M.DEFAULTS[mode])
            assert (c["to"] >= 0).sum() == want, (n, mode)
            assert c["exhausted"].sum() == (exhausted if mode == "mini" else 0)
    for n in (2, 3, 63, 64, 65):
        pos, steps, _ = M.lap(n, M.LAP_SEED)
        for mode in ("gtvicinity", "mini"):
            assert (M.candidates(pos, steps, mode, **M.DEFAULTS[mode])["to"] >= 0).sum() == 0      # hence the scaled cases
    for n, circumference, thr in M.small_cases():
        pos, steps, _ = M.lap(n, M.LAP_SEED, circumference)
        for mode in ("gtvicinity", "mini"):
            c = M.candidates(pos, steps, mode, **thr)
            assert 0 < (c["to"] >= 0).sum() < n, (n, mode)


def test_abi_names_the_closure_call_and_its_structs():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_[a-z0-9_]+)\s*\(", hdr))
    assert {"cfear_closure_params_default", "cfear_closure_candidates_batch"} <= declared & set(L.EXPORTS)
    assert hasattr(lib, "cfear_closure_candidates_batch") and lib.cfear_abi_version() == 1
    assert C.sizeof(L.ClosureParams) == 40 and C.sizeof(L.ClosureCandidate) == 40 == L.CLOSURE_CANDIDATE_DTYPE.itemsize
    assert [(f, getattr(L.ClosureParams, f).offset) for f, _ in L.ClosureParams._fields_] == [
        ("mode", 0), ("verify_via_odometry", 4), ("min_d_travel", 8), ("max_d_travel", 16), ("max_d_close", 24), ("odom_sigma_error", 32)]
    for name, off in (("to", 0), ("exhausted", 4), ("eucl", 8), ("trav", 16), ("rel", 24), ("odom_bounds", 32)):
        assert getattr(L.ClosureCandidate, name).offset == off == L.CLOSURE_CANDIDATE_DTYPE.fields[name][1]
    consts = dict(re.findall(r"#define (CFEAR_CLOSURE_[A-Z]+) (\d+)", hdr))
    assert int(consts["CFEAR_CLOSURE_ORIGINS"]) == L.CLOSURE_ORIGINS and int(consts["CFEAR_CLOSURE_TILE"]) == L.CLOSURE_TILE
    assert (int(consts["CFEAR_CLOSURE_GTVICINITY"]), int(consts["CFEAR_CLOSURE_MINI"])) == (L.CLOSURE_MODE["gtvicinity"], L.CLOSURE_MODE["mini"])


def test_defaults_follow_the_reference():
    for mode, want in (("gtvicinity", (40.0, 4200.0, 15.0)), ("mini", (25.0, 500.0, 15.0))):       # loopclosure.h:84-86, :95-97
        p = api.closure_params(mode)
        assert (p.min_d_travel, p.max_d_travel, p.max_d_close) == want == tuple(M.DEFAULTS[mode].values())
        assert (p.mode, p.verify_via_odometry, p.odom_sigma_error) == (L.CLOSURE_MODE[mode], 1, 0.03)   # :122-123
    assert api.closure_params("mini", max_d_close=3, verify_via_odometry=0).max_d_close == 3.0
    for bad in (dict(mode="scancontext"), dict(no_such_field=1)):
        with pytest.raises(L.CfearError):
            api.closure_params(**bad)


def _call(pos, steps, off, par, rel=None, ctx=None):
    out = np.full(len(pos), 7, L.CLOSURE_CANDIDATE_DTYPE)
    bad = C.c_int32(5)
    rc = L.lib().cfear_closure_candidates_batch(ctx, pos.ctypes.data, steps.ctypes.data, None if rel is None else rel.ctypes.data,
                                                off.ctypes.data, len(pos), len(off) - 1, C.byref(par), out.ctypes.data, C.byref(bad))
    return rc, bad.value, out


def test_refusals_need_no_device():
    """Every check is made before a context is asked for: the refusals name the graph, and nothing is written."""
    pos = np.concatenate([M.lap(5, 1)[0], M.lap(1, 2)[0], M.lap(6, 3)[0]])
    steps = np.concatenate([M.lap(5, 1)[1], M.lap(1, 2)[1], M.lap(6, 3)[1]])
    off = np.array([0, 5, 5, 6, 12], np.int64)                                 # an empty and a one-node graph among them
    par = api.closure_params("mini")
    untouched = np.full(len(pos), 7, L.CLOSURE_CANDIDATE_DTYPE).tobytes()
    rc, bad, out = _call(pos, steps, off, par)
    assert (rc, bad) == (L.ERR_INVALID_ARGUMENT, -1) and out.tobytes() == untouched        # valid: only the context is missing

    def edited(arr, idx, v):
        a = arr.copy()
        a[idx] = v
        return a
    cases = [(pos, steps, edited(off, 0, 1), par, 0), (pos, steps, edited(off, 4, 11), par, 3), (pos, steps, edited(off, 2, 4), par, 1),
             (pos, edited(steps, 8, -1.0), off, par, 3), (pos, edited(steps, 2, np.inf), off, par, 0), (pos, edited(steps, 1, np.nan), off, par, 0),
             (edited(pos, (5, 1), np.nan), steps, off, par, 2), (edited(pos, (11, 2), -np.inf), steps, off, par, 3),
             (pos, steps, off, api.closure_params("mini", max_d_close=np.nan), -1), (pos, steps, off, api.closure_params("mini", min_d_travel=np.nan), -1),
             (pos, steps, off, api.closure_params("gtvicinity", max_d_travel=np.nan), -1)]
    unknown = api.closure_params("mini")
    unknown.mode = 2
    cases.append((pos, steps, off, unknown, -1))
    for k, (p_, s_, o_, par_, want) in enumerate(cases):
        rc, bad, out = _call(p_, s_, o_, par_)
        assert (rc, bad) == (L.ERR_INVALID_ARGUMENT, want), k
        assert out.tobytes() == untouched, k
    # each graph's LAST step entry is unused and may hold anything
    rc, bad, _ = _call(pos, edited(steps, 4, np.nan), off, par)
    assert (rc, bad) == (L.ERR_INVALID_ARGUMENT, -1)


def test_marshalling_errors_need_no_device():
    pos, steps, rel = M.lap(6, 1)
    assert api.closure_candidates([]) == []
    poses = np.zeros((4, 3))
    poses[:, 0] = [0.0, 1.0, 2.0, 3.5]
    cons = [dict(id_begin=k + 1, id_end=k, t_be=np.concatenate(api.pose3d_from_xyt([poses[k, 0] - poses[k + 1, 0], 0.0, 0.125])), type=0)
            for k in range(3)]
    for graphs in ([(pos,)], [(pos, steps[:3])], [(pos, steps, rel[:2])], [(pos[:, :2], steps)], [(pos, steps, rel), (pos, steps)],
                   [(poses, cons[:2])], [(poses, cons + [dict(id_begin=3, id_end=1, t_be=[0, 0, 0])])], [(poses, [dict(id_begin=1)])]):
        with pytest.raises(L.CfearError) as e:
            api.closure_candidates(graphs)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
    p3, s3, r3 = api._closure_graph_arrays((poses, cons + [dict(id_begin=3, id_end=0, t_be=[0, 0, 0], type=1)]), "g")
    assert p3.tolist() == [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3.5, 0, 0]] and s3.tolist() == [1.0, 1.0, 1.5, 0.0]
    assert np.allclose(r3, [[-1, 0, 0.125], [-1, 0, 0.125], [-1.5, 0, 0.125], [0, 0, 0]], atol=1e-15)
    # steps and motions one per node or one per step
    a, b = api._closure_graph_arrays((pos, steps, rel), "g"), api._closure_graph_arrays((pos, steps[:-1], rel[:-1]), "g")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_closure_verify_jobs():
    cands = np.zeros(4, L.CLOSURE_CANDIDATE_DTYPE)
    cands["to"] = [3, -1, 3, -1]
    cands["odom_bounds"] = [0.25, 0.0, 0.5, 0.0]
    nodes = [dict(scan="s%d" % k, peaks="p%d" % k) for k in range(4)]
    poses = np.arange(12.0).reshape(4, 3)
    jobs = api.closure_verify_jobs(cands, nodes, poses, group_base=100)
    assert [(j["from"], j["to"], j["group"], j["odom_bounds"], j["sc_sim"]) for j in jobs] == [(3, 0, 100, 0.25, 0.0), (3, 2, 102, 0.5, 0.0)]
    assert jobs[0]["from_scan"] == "s3" and jobs[0]["to_peaks"] == "p0" and jobs[1]["to_scan"] == "s2"
    assert jobs[0]["from_pose"].tolist() == [9.0, 10.0, 11.0] and tuple(jobs[0]["t_be_guess"]) == (0.0, 0.0, 0.0)


def test_cpp_signature_compiles_and_refuses(tmp_path):
    exe = str(tmp_path / "closure_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "closure_signature.cpp"), "-o", exe, "-L", so_dir, "-lcfear_hip",
                           "-Wl,-rpath," + so_dir])
    out = subprocess.check_output([exe]).decode().split()
    assert out == [str(L.ERR_INVALID_ARGUMENT), "1", str(L.ERR_INVALID_ARGUMENT), "-1", "25", "500", "15"]
