"""CPU: the C-ABI of the odometry grid and of the row-key derivation -- declared in include/cfear_hip.h, listed in
_lib.EXPORTS and present in the built library; calls without an object are refused without touching a device; the ctypes
records have the header's sizes; the C++ mirror (OdometryGrid) compiles against the reference-side stand-ins and its plan,
host code, runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_kstrong_rowkeys_derive", "cfear_odometry_grid_plan", "cfear_odometry_grid_create", "cfear_odometry_grid_process",
       "cfear_odometry_grid_destroy"]


def test_new_symbols_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert "typedef struct cfear_odometry_grid cfear_odometry_grid;" in hdr
    assert C.sizeof(L.RowkeysClass) == 20 and L.GRID_STREAM_DTYPE.itemsize == 32 and C.sizeof(L.GridTotals) == 32


def test_calls_without_an_object_are_refused():
    from tbv_slam_public_amd import _lib as L
    lib = L.lib()
    out = C.c_void_p()
    d = L.PolarDesc(400, 3360, 3360, 1, 400 * 3360)
    p = L.OdometryParams()
    lib.cfear_odometry_params_default(C.byref(p))
    assert lib.cfear_odometry_grid_create(None, C.byref(d), C.byref(p), 1, None, None, 1, C.byref(out)) == L.ERR_INVALID_ARGUMENT
    assert not out.value
    assert lib.cfear_odometry_grid_process(None, None, None) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_odometry_grid_destroy(None) == L.OK
    cls = (L.RowkeysClass * 1)()
    assert lib.cfear_kstrong_rowkeys_derive(None, None, None, None, 1, 1, 1, 0.0, cls, 1, None, None) == L.ERR_INVALID_ARGUMENT
    # the plan needs neither a context nor a device; every output is optional
    assert lib.cfear_odometry_grid_plan(C.byref(d), C.byref(p), 1, None, None, 1, None, None, None, 0) == L.OK
    assert lib.cfear_odometry_grid_plan(None, C.byref(p), 1, None, None, 1, None, None, None, 0) == L.ERR_INVALID_ARGUMENT


def test_cpp_mirror_compiles_and_plans_without_a_gpu(tmp_path):
    exe = str(tmp_path / "grid_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "grid_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    import torch
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    lines = r.stdout.decode().splitlines()
    # 2 sequences x 3 configurations; per sequence one sweep and two classes (CFEAR-1 and k = 12 share one), all derived;
    # surface: res 3 with weights | CFEAR-1; matcher: CFEAR-3's | CFEAR-1's
    assert lines[0].split() == ["6", "2", "4", "4", "2", "2"], lines
    assert "configuration 2: keep_nodes" in lines[1]
    if not torch.cuda.is_available():
        assert r.returncode == 2 and b"device" in r.stderr.lower(), (r.returncode, r.stderr)
        return
    assert r.returncode == 0, r.stderr
    assert lines[2].split() == ["1"] * 6                                   # the first frame becomes the first keyframe
    assert len(lines[3].split()) == 6, lines                               # every stream reports its second frame
