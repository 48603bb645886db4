"""CPU: the offset tables of the batched graph and trajectory entry points (tbv_slam_public_amd/csrc/batch_tables.hpp).

The six entry points that take offsets [n + 1] refuse a malformed table before they need a context, so they are called with
ctx = NULL and the message is read at cfear_last_error(NULL).  Which range a call blames for a table with several faults
differs between the entry points (closure tests the end before the ranges, the loop rows read the table front to back); the
literals below were taken from the library as it was before the checks were folded into one helper, and pin that.
cfear_pgo_solve_batch needs its context first: its tables are in tests/test_gpu_pgo_batch.py.  The helper itself, the flat
grid and the table layout are exercised by a stand-alone program (tests/cpp/batch_tables_check.cpp), plain and under the
host sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tbv_slam_public_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, CAP = L.ERR_INVALID_ARGUMENT, L.ERR_CAPACITY
BIG = 2 ** 31                                   # items in one range that every entry point's capacity limit refuses

# name -> (offsets, total); three ranges unless the name says otherwise
TABLES = {
    "fine": ([0, 3, 5, 8], 8),
    "empty ranges": ([0, 0, 8, 8], 8),
    "start not 0": ([1, 3, 5, 8], 8),
    "end short of total": ([0, 3, 5, 7], 8),
    "end past total": ([0, 3, 5, 9], 8),
    "descends": ([0, 5, 3, 8], 8),
    "leaves then descends": ([0, 3, 9, 8], 8),
    "first range leaves, second descends": ([0, 9, 8, 8], 8),
    "descends and wrong end": ([0, 5, 3, 7], 8),
    "start not 0 and descends": ([2, 1, 5, 8], 8),
    "no ranges, start not 0": ([2], 0),
    "no ranges, start not 0 but equal to total": ([2], 2),
    "no ranges": ([0], 0),
    "second range over capacity": ([0, 2, 2 + BIG, 3 + BIG], 3 + BIG),
}


def _ptr(x):
    return None if x is None else x.ctypes.data


def _message():
    return L.lib().cfear_last_error(None).decode()


def _index(msg):
    m = re.search(r"(?:graph|experiment) (-?\d+)", msg)
    return int(m.group(1)) if m else msg


def closure(off, total):
    off = np.array(off, np.int64)
    n = min(total, 16)
    pos, steps, out = np.zeros((n + 1, 3)), np.ones(n + 1), np.zeros(n + 1, L.CLOSURE_CANDIDATE_DTYPE)
    par, bad = L.ClosureParams(), C.c_int32(-7)
    L.lib().cfear_closure_params_default(C.byref(par), 0)
    rc = L.lib().cfear_closure_candidates_batch(None, _ptr(pos), _ptr(steps), None, _ptr(off), total, len(off) - 1, C.byref(par), _ptr(out),
                                                C.byref(bad))
    return rc, bad.value, _index(_message())


def loop_stats(off, total):
    off = np.array(off, np.int64)
    n = min(total, 16)
    gt, has = np.zeros((n + 1, 3)), np.zeros(n + 1, np.uint8)
    par, bad = L.LoopStatsParams(), C.c_int64(-7)
    L.lib().cfear_loop_stats_params_default(C.byref(par))
    rc = L.lib().cfear_loop_stats_batch(None, _ptr(off), _ptr(gt), _ptr(has), total, len(off) - 1, None, 0, C.byref(par), None, C.byref(bad))
    return rc, bad.value, _index(_message())


def loop_curves(off, total):
    off = np.array(off, np.int64)
    n = min(total, 16)
    y, score = np.zeros(n + 1, np.uint8), np.zeros(n + 1)
    curves = [np.zeros(n + len(off) + 1) for _ in range(6)]
    res = np.zeros(len(off), L.LOOP_CURVES_RESULT_DTYPE)
    par, bad = L.LoopCurvesParams(), C.c_int32(-7)
    L.lib().cfear_loop_curves_params_default(C.byref(par))
    rc = L.lib().cfear_loop_curves_batch(None, _ptr(off), _ptr(y), _ptr(score), None, total, len(off) - 1, C.byref(par),
                                         *[_ptr(c) for c in curves], _ptr(res), C.byref(bad))
    return rc, bad.value, _index(_message())


def graph_align(off, total):
    off = np.array(off, np.int64)
    n = min(total, 16)
    poses, gt, has = np.zeros((n + 1, 7)), np.zeros((n + 1, 7)), np.zeros(n + 1, np.uint8)
    summ = np.zeros(len(off), L.GRAPH_ALIGN_SUMMARY_DTYPE)
    rc = L.lib().cfear_graph_align_batch(None, _ptr(poses), _ptr(gt), _ptr(has), _ptr(off), total, len(off) - 1, _ptr(summ))
    return rc, None, _index(_message())


def _graph_map(node_off, n_nodes, cloud_off, n_points):
    node_off, cloud_off = np.array(node_off, np.int64), np.array(cloud_off, np.int64)
    n = min(n_nodes, 16)
    poses, xyzi, out = np.zeros((n + 1, 7)), np.zeros((min(n_points, 16) + 1, 4), np.float32), np.zeros((1, 4), np.float32)
    summ = np.zeros(len(node_off), L.GRAPH_MAP_SUMMARY_DTYPE)
    par = L.GraphMapParams(1, 0)
    rc = L.lib().cfear_graph_map_batch(None, _ptr(poses), None, None, _ptr(node_off), n_nodes, len(node_off) - 1, _ptr(xyzi), _ptr(cloud_off),
                                       n_points, C.byref(par), _ptr(out), 0, None, 0, _ptr(summ))
    return rc, None, _index(_message())


def graph_map_nodes(off, total):
    """the table under test is node_offsets; every node's cloud is empty"""
    return _graph_map(off, total, np.zeros(min(total, 16) + 1, np.int64), 0)


def graph_map_clouds(off, total):
    """the table under test is cloud_offsets: one graph that holds all its nodes"""
    return _graph_map([0, len(off) - 1], len(off) - 1, off, total)


A_NODE = "node_offsets must run from 0 to n_nodes without descending"
A_CLOUD = "cloud_offsets must run from 0 to n_points without descending"
NULL_CTX = "null context"

# entry point -> table -> (status, failed_* out-parameter or None where the call has none, the index in the message or the
# whole message where it has none).  A fine table gets as far as the missing context, which closure and the two loop calls
# report without a message of their own: the message is then the previous call's, None here.
EXPECTED = {
    "closure": {                                                  # the start and the end first, then range by range
        "fine": (INV, -1, None),
        "empty ranges": (INV, -1, None),
        "start not 0": (INV, 0, 0),
        "end short of total": (INV, 2, 2),
        "end past total": (INV, 2, 2),
        "descends": (INV, 1, 1),
        "leaves then descends": (CAP, 1, 1),                      # a range that leaves the arrays and holds nodes is a capacity error
        "first range leaves, second descends": (CAP, 0, 0),
        "descends and wrong end": (INV, 2, 2),
        "start not 0 and descends": (INV, 0, 0),
        "no ranges, start not 0": (INV, -1, -1),
        "no ranges, start not 0 but equal to total": (INV, -1, -1),
        "no ranges": (INV, -1, None),
        "second range over capacity": (CAP, 1, 1),
    },
    "loop_stats": {                                               # front to back; failed_candidate is not about the table
        "fine": (INV, -1, None),
        "empty ranges": (INV, -1, None),
        "start not 0": (INV, -1, 0),
        "end short of total": (INV, -1, 2),
        "end past total": (INV, -1, 2),
        "descends": (INV, -1, 1),
        "leaves then descends": (INV, -1, 1),
        "first range leaves, second descends": (INV, -1, 0),
        "descends and wrong end": (INV, -1, 1),
        "start not 0 and descends": (INV, -1, 0),
        "no ranges, start not 0": (INV, -1, -1),
        "no ranges, start not 0 but equal to total": (INV, -1, -1),
        "no ranges": (INV, -1, None),
        "second range over capacity": (CAP, -1, 1),
    },
    "loop_curves": {                                              # front to back
        "fine": (INV, -1, None),
        "empty ranges": (INV, -1, None),
        "start not 0": (INV, 0, 0),
        "end short of total": (INV, 2, 2),
        "end past total": (INV, 2, 2),
        "descends": (INV, 1, 1),
        "leaves then descends": (INV, 1, 1),
        "first range leaves, second descends": (INV, 0, 0),
        "descends and wrong end": (INV, 1, 1),
        "start not 0 and descends": (INV, 0, 0),
        "no ranges, start not 0": (INV, -1, -1),
        "no ranges, start not 0 but equal to total": (INV, -1, -1),
        "no ranges": (INV, -1, None),
        "second range over capacity": (CAP, 1, 1),
    },
}
for _name, _text in (("graph_align", A_NODE), ("graph_map_nodes", A_NODE), ("graph_map_clouds", A_CLOUD)):   # one message, no index
    EXPECTED[_name] = {t: (INV, None, NULL_CTX if t in ("fine", "empty ranges", "no ranges") else _text) for t in TABLES}
EXPECTED["graph_align"]["second range over capacity"] = (CAP, None, 1)
del EXPECTED["graph_map_nodes"]["second range over capacity"]
EXPECTED["graph_map_clouds"]["second range over capacity"] = (INV, None, NULL_CTX)     # a cloud's size is checked behind the context
# 2^31 nodes pass the node table's check, and the cloud table that is checked next would need an entry for every one of them
UNREACHABLE = ("graph_map_nodes", "second range over capacity")
CALLS = {f.__name__: f for f in (closure, loop_stats, loop_curves, graph_align, graph_map_nodes, graph_map_clouds)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_malformed_offset_tables_are_refused_without_a_device_and_blame_the_same_range_as_before(name):
    assert sorted(EXPECTED[name]) == sorted(t for t in TABLES if (name, t) != UNREACHABLE)
    for table, want in EXPECTED[name].items():
        got = CALLS[name](*TABLES[table])
        if want[2] is None:
            got = got[:2] + (None,)
        assert got == want, (name, table, got, want)


def test_batch_tables_header_stands_alone(tmp_path):
    """The offsets check on the tables above, the flat grid at lengths 0, 1, 255, 256 and 257 with tile 256, and the 16-byte
    padding of a 72-byte record table: compiled without HIP, run plainly and under the host sanitizers."""
    src = os.path.join(ROOT, "tests", "cpp", "batch_tables_check.cpp")
    for flags in ([], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]):
        exe = str(tmp_path / ("batch_tables_check" + ("_san" if flags else "")))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split()[-1] == "ok", r.stdout + r.stderr
