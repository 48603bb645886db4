"""CPU: the C-ABI additions of the raw-sweep Scan Context -- struct sizes, TBV's defaults, the new symbols declared in
include/cfear_hip.h, listed in _lib.EXPORTS and present in the built library -- and the C++ mirror's cv::Mat entry
compiled against the cv_bridge stand-in."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cfear_sc_raw_params_default", "cfear_sc_raw_descriptors", "cfear_sc_manager_add_raw"]


def test_struct_sizes_and_abi_version():
    from tbv_slam_public_amd import _lib as L
    assert C.sizeof(L.ScRawParams) == 24
    assert C.sizeof(L.ScParams) == 48 and C.sizeof(L.ScManagerParams) == 88      # unchanged
    assert C.sizeof(L.PolarDesc) == 24
    assert L.lib().cfear_abi_version() == 1


def test_defaults_are_tbv_settings():
    from tbv_slam_public_amd import _lib as L
    p = L.ScRawParams(radar_threshold=5.0, transpose=7, normalize=7, interpolation=7, pad=7)
    L.lib().cfear_sc_raw_params_default(C.byref(p))
    assert (p.radar_threshold, p.transpose, p.normalize, p.interpolation, p.pad) == (0.0, 1, 0, 3, 0)
    from tbv_slam_public_amd import api
    q = api.sc_raw_params(interpolation="area", radar_threshold=64.5)
    assert q.interpolation == L.SC_INTER_AREA and q.radar_threshold == 64.5
    with pytest.raises(KeyError):
        api.sc_raw_params(nonsense=1)


def test_new_symbols_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared, s
        assert s in L.EXPORTS, s
        assert hasattr(lib, s), s
    assert "#define CFEAR_SC_INTER_AREA 3" in hdr


def test_cpp_raw_entry_compiles_against_the_cv_bridge_standin(tmp_path):
    exe = str(tmp_path / "sc_raw_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"),
                           os.path.join(ROOT, "tests", "cpp", "sc_raw_signature.cpp"), "-o", exe, "-L", so_dir,
                           "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)
