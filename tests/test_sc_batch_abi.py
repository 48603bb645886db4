"""CPU: the C-ABI of batched Scan Context (cfear_sc_detect_batch) -- the symbol declared in include/cfear_hip.h, listed in
_lib.EXPORTS and present in the built library, cfear_sc_batch's size and offsets, the ABI version, the C++ wrapper compiled,
and the refusals the call decides on the host, which it decides before it needs a context: with ctx = NULL a bad batch is
refused for its own reason (read back with cfear_last_error(NULL)) and a good one for the missing context."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    assert "cfear_sc_detect_batch" in declared
    assert "cfear_sc_detect_batch" in L.EXPORTS
    assert hasattr(L.lib(), "cfear_sc_detect_batch")
    assert "#define CFEAR_SC_NODES_CLOUD 0" in hdr and "#define CFEAR_SC_NODES_RAW 1" in hdr
    assert (L.SC_NODES_CLOUD, L.SC_NODES_RAW) == (0, 1)
    assert "CFEAR_OPT_COUNT = 6" in hdr                            # no new context option


def test_struct_layout_and_abi_version():
    from tbv_slam_public_amd import _lib as L
    B = L.ScBatch
    assert C.sizeof(B) == 96 and C.sizeof(B) % 8 == 0
    got = [(n, getattr(B, n).offset) for n, _ in B._fields_]
    assert got == [("n_graphs", 0), ("mode", 4), ("node_off", 8), ("n_detect", 16), ("ids", 24), ("T", 32), ("Tinv", 40),
                   ("xyzi", 48), ("point_off", 56), ("n_aggregate", 64), ("pad", 68), ("imgs", 72), ("desc", 80), ("raw", 88)]
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    body = re.search(r"typedef struct cfear_sc_batch \{(.*?)\} cfear_sc_batch;", hdr, re.S).group(1)
    names = [n for line in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";")
             for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip().replace("*", " "))]
    assert names == [n for n, _ in B._fields_]                     # the header's members, in the mirror's order
    assert C.sizeof(L.ScManagerParams) == 88 and C.sizeof(L.ScRawParams) == 24 and L.SC_CANDIDATE_DTYPE.itemsize == 64
    assert L.lib().cfear_abi_version() == 1


def test_cpp_batch_wrapper_compiles(tmp_path):
    exe = str(tmp_path / "sc_batch_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "sc_batch_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)


class _Batch:
    """Three small graphs (2, 0 and 3 nodes) as flat host tables; `call` passes them with ctx = NULL."""

    def __init__(self):
        from tbv_slam_public_amd import _lib as L
        from tbv_slam_public_amd import api
        self.L, self.lib = L, L.lib()
        self.p = api.sc_manager_params()
        self.node_off = np.array([0, 2, 2, 5], np.int32)
        self.n_detect = np.array([2, 0, 3], np.int32)
        self.ids = np.array([0, 1, 0, 2, 5], np.int32)
        self.T = np.zeros((5, 8))
        self.Tinv = np.zeros((5, 8))
        self.point_off = np.array([0, 3, 3, 7, 8, 12], np.int64)
        self.xyzi = np.zeros((12, 4), np.float32)
        self.imgs = np.zeros((5, 300, 100), np.uint8)
        self.desc = L.PolarDesc()
        self.desc.rows, self.desc.cols, self.desc.stride, self.desc.batch, self.desc.batch_stride = 300, 100, 100, 5, 30000
        self.raw = api.sc_raw_params(transpose=1)
        self.out = np.full((5, 3), 0x5A, np.uint8).repeat(64, 1).view(L.SC_CANDIDATE_DTYPE)
        self.n_out = np.full(5, 0x5A5A5A5A, np.int32)
        self.b = L.ScBatch()
        self.b.n_graphs, self.b.mode, self.b.n_aggregate = 3, L.SC_NODES_CLOUD, 1
        for n in ("node_off", "n_detect", "ids", "T", "Tinv", "point_off", "xyzi", "imgs"):
            setattr(self.b, n, getattr(self, n).ctypes.data)
        self.b.desc, self.b.raw = C.pointer(self.desc), C.pointer(self.raw)

    def call(self, out=True, n_out=True):
        rc = self.lib.cfear_sc_detect_batch(None, C.byref(self.p), C.byref(self.b), self.out.ctypes.data if out else None,
                                            self.n_out.ctypes.data if n_out else None)
        return rc, self.lib.cfear_last_error(None).decode()


def test_refusals_are_decided_before_the_context_is_needed():
    t = _Batch()
    L = t.L
    INV, CAP = L.ERR_INVALID_ARGUMENT, L.ERR_CAPACITY
    # a good batch, in both modes, gets as far as the missing context
    assert t.call() == (INV, "null context")
    t.b.mode = L.SC_NODES_RAW
    assert t.call() == (INV, "null context")
    t.b.mode = L.SC_NODES_CLOUD

    def refused(status, word, **kw):
        rc, msg = t.call(**kw)
        assert rc == status and word in msg and msg != "null context", (rc, msg)

    def with_(arr, idx, val, status, word):
        old = arr[idx]
        arr[idx] = val
        refused(status, word)
        arr[idx] = old

    with_(t.node_off, 2, 1, INV, "graph 1: node_off decreases")
    with_(t.node_off, 0, 1, INV, "node_off[0]")
    with_(t.point_off, 4, 2, INV, "graph 2, node 1: point_off")
    with_(t.n_detect, 2, 4, INV, "graph 2: n_detect 4")
    with_(t.n_detect, 0, -1, INV, "graph 0: n_detect -1")
    with_(t.ids, 4, 2, INV, "graph 2, node 2: ids must increase")
    with_(t.ids, 2, 7, INV, "graph 2, node 1: ids must increase")
    t.ids[2] = 1                                                   # the ids of one graph do not bind the next
    assert t.call()[1] == "null context"
    t.ids[2] = 0
    for mode in (2, -1):
        t.b.mode = mode
        refused(INV, "unknown node mode")
    t.b.mode = L.SC_NODES_CLOUD
    refused(INV, "null output", out=False)
    refused(INV, "null output", n_out=False)
    for name, word in (("node_off", "null node_off"), ("T", "null T"), ("Tinv", "null Tinv"), ("point_off", "point_off"),
                       ("xyzi", "graph 0, node 0: null cloud")):
        old = getattr(t.b, name)
        setattr(t.b, name, None)
        refused(INV, word)
        setattr(t.b, name, old)
    t.b.n_aggregate = -1
    refused(INV, "n_aggregate")
    t.b.n_aggregate = 1
    t.b.n_graphs = -1
    refused(INV, "node_off")
    t.b.n_graphs = 3
    # raw mode: null sweeps, a sweep count that is not the node count
    t.b.mode = L.SC_NODES_RAW
    old = t.b.imgs
    t.b.imgs = None
    refused(INV, "null sweeps")
    t.b.imgs = old
    t.desc.batch = 4
    refused(INV, "4 sweeps for 5 nodes")
    t.desc.batch = 5
    t.b.mode = L.SC_NODES_CLOUD
    # the manager's and the kernels' limits, as cfear_sc_detect_sequence refuses them
    for field, val, status in (("num_candidates_from_tree", 65, CAP), ("num_candidates_from_tree", 0, INV), ("n_candidates", 0, INV),
                               ("odom_sigma_error", 0.0, INV)):
        old = getattr(t.p, field)
        setattr(t.p, field, val)
        assert t.call()[0] == status and t.call()[1] != "null context", field
        setattr(t.p, field, old)
    from tbv_slam_public_amd import api
    for kw, status in ((dict(num_ring=41, num_sector=125), CAP), (dict(num_ring=2, num_sector=2560), CAP),
                       (dict(num_ring=0), CAP), (dict(search_ratio=float("nan")), INV)):
        t.p.sc = api.sc_params(**kw)
        assert t.call()[0] == status and t.call()[1] != "null context", kw
    t.p.sc = api.sc_params()
    # nothing detected: the outputs are not asked for
    t.n_detect[:] = 0
    assert t.call(out=False, n_out=False) == (INV, "null context")
    t.b.n_graphs = 0
    assert t.call(out=False, n_out=False) == (INV, "null context")
    # no refusal wrote a byte
    assert (t.out.view(np.uint8) == 0x5A).all() and (t.n_out == 0x5A5A5A5A).all()
