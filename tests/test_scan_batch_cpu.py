"""CPU: the C-ABI of the scan batch -- the new symbols declared in include/cfear_hip.h, listed in _lib.EXPORTS and present in
the built library; calls without a context or a batch are refused without touching a device; the C++ mirror (ScanBatch)
compiles against the reference-side stand-ins."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_scan_create_batch", "cfear_scan_batch_size", "cfear_scan_batch_get", "cfear_scan_batch_destroy"]


def test_new_symbols_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert "typedef struct cfear_scan_batch cfear_scan_batch;" in hdr and "#define CFEAR_ABI_VERSION 1" in hdr
    assert lib.cfear_abi_version() == 1


def test_calls_without_a_context_or_a_batch_are_refused():
    from tbv_slam_public_amd import _lib as L
    lib = L.lib()
    fp = L.FeatureParams()
    out, s = C.c_void_p(), C.c_void_p()
    status = (C.c_int32 * 1)()
    off, ln = (C.c_int64 * 1)(0), (C.c_int32 * 1)(0)
    assert lib.cfear_scan_create_batch(None, None, off, ln, 1, C.byref(fp), None, 16, C.byref(out), status) == L.ERR_INVALID_ARGUMENT
    assert not out.value
    assert lib.cfear_scan_batch_size(None) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_scan_batch_get(None, 0, C.byref(s)) == L.ERR_INVALID_ARGUMENT
    assert lib.cfear_scan_batch_destroy(None) == L.OK


def test_cpp_mirror_compiles_against_the_stand_ins(tmp_path):
    """include/cfear_hip.hpp (ScanBatch) is syntactically sound with the reference-side stand-ins; without a GPU the program
    reports the missing device and exits 2, with one it serves two lattices around an empty cloud."""
    exe = str(tmp_path / "scan_batch_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "scan_batch_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    import torch
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if not torch.cuda.is_available():
        assert r.returncode == 2 and b"device" in r.stderr.lower(), (r.returncode, r.stderr)
        return
    assert r.returncode == 0, r.stderr
    st0, st1, st2, n0, n2, null1, refused = [int(v) for v in r.stdout.replace(b"|", b" ").split()]
    assert (st0, st1, st2) == (0, -6, 0) and n0 > 0 and n2 > 0 and null1 == 1 and refused == 1
