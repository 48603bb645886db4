"""CPU: the C-ABI of whole-graph Scan Context -- the new symbols declared in include/cfear_hip.h, listed in _lib.EXPORTS and
present in the built library, struct sizes, the chunk hook -- the node matrices api.sc_node_affines builds, pushed through
the kernel's operation order, against examples/loop_closure_demo.py's transform_cloud, and the C++ wrapper compiled."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_sc_local_map_descriptors", "cfear_sc_detect_sequence"]


def test_new_symbols_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared, s
        assert s in L.EXPORTS, s
        assert hasattr(lib, s), s
    assert "CFEAR_OPT_SC_QUERY_CHUNK = 4" in hdr and L.OPT_SC_QUERY_CHUNK == 4 and L.OPT_COUNT == 5


def test_struct_sizes_and_abi_version():
    from tbv_slam_public_amd import _lib as L
    assert C.sizeof(L.ScNode) == 152
    assert L.ScNode.T.offset == 16 and L.ScNode.Tinv.offset == 80 and L.ScNode.id.offset == 144
    assert C.sizeof(L.ScParams) == 48 and C.sizeof(L.ScManagerParams) == 88 and C.sizeof(L.ScCloud) == 16   # unchanged
    assert L.SC_CANDIDATE_DTYPE.itemsize == 64
    assert L.lib().cfear_abi_version() == 1


def _kernel_order(xyzi, T):
    """sc_local_map_kernel's transform: ((m0 x + m1 y) + m2 z) + m3 in double, each row rounded to float; z, i carried."""
    x, y, z = (xyzi[:, c].astype(np.float64) for c in range(3))
    out = xyzi.copy()
    out[:, 0] = (((T[0] * x + T[1] * y) + T[2] * z) + T[3]).astype(np.float32)
    out[:, 1] = (((T[4] * x + T[5] * y) + T[6] * z) + T[7]).astype(np.float32)
    return out


def test_node_affines_through_the_kernel_order_reproduce_the_demo_transform():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import loop_closure_demo as demo
    from tbv_slam_public_amd import api
    rng = np.random.default_rng(5)
    poses = np.stack([rng.uniform(-300, 300, 40), rng.uniform(-300, 300, 40), rng.uniform(-7, 7, 40)], 1)
    poses[0] = (0.0, 0.0, 0.0)
    poses[1] = (12.5, -3.0, np.pi)
    T, Ti = api.sc_node_affines(poses)
    assert T.shape == Ti.shape == (40, 8) and T.dtype == np.float64
    assert (T[:, 2] == 0).all() and (T[:, 6] == 0).all() and (T[:, 3] == poses[:, 0]).all() and (T[:, 7] == poses[:, 1]).all()
    cloud = np.zeros((500, 4), np.float32)
    cloud[:, :2] = rng.uniform(-80, 80, (500, 2))
    cloud[:, 2] = rng.choice([0.0, -0.0, 1.5], 500)
    cloud[:, 3] = np.floor(rng.uniform(0, 100, 500))
    for j in range(40):
        i = (j * 7 + 3) % 40
        want = demo.transform_cloud(demo.transform_cloud(cloud, poses[j]), demo.xyt_inverse(poses[i]))
        got = _kernel_order(_kernel_order(cloud, T[j]), Ti[i])
        assert got.dtype == want.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def test_cpp_sequence_wrapper_compiles(tmp_path):
    exe = str(tmp_path / "sc_sequence_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "sc_sequence_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)
