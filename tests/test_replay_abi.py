"""CPU: the C-ABI of the replay -- the symbol declared in include/cfear_hip.h, listed in _lib.EXPORTS and present in the
built library, the record's layout in the header, ctypes and NumPy, the chunk option numbered apart from the pinned enum,
refusals that need no device, and the C++ mirror (OdometryReplay) compiled against the reference-side stand-ins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_record_and_option():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    assert "cfear_odometry_replay_clouds" in declared and "cfear_odometry_replay_clouds" in L.EXPORTS
    assert hasattr(L.lib(), "cfear_odometry_replay_clouds") and L.lib().cfear_abi_version() == 1
    body = re.search(r"typedef struct cfear_replay_frame \{(.*?)\} cfear_replay_frame;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().split("[")[0] for decl in re.findall(r"(?:double|int32_t)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == list(L.REPLAY_FRAME_DTYPE.names) and L.REPLAY_FRAME_DTYPE.itemsize == 160
    assert "#define CFEAR_OPT_REPLAY_CHUNK %d\n" % L.OPT_REPLAY_CHUNK in hdr and L.OPT_REPLAY_CHUNK >= 6    # apart from enum cfear_option


def test_call_without_a_context_is_refused():
    from tbv_slam_public_amd import _lib as L
    par = L.OdometryParams()
    L.lib().cfear_odometry_params_default(C.byref(par))
    arr = (L.ScCloud * 2)()
    out = np.zeros(2, L.REPLAY_FRAME_DTYPE)
    trace, seq = np.zeros((2, 3)), np.array([0, 2], np.int32)
    assert L.lib().cfear_odometry_replay_clouds(None, arr, C.byref(par), trace.ctypes.data, seq.ctypes.data, 1, 0, out.ctypes.data) == L.ERR_INVALID_ARGUMENT
    assert not out.view(np.uint8).any()


def test_summary_is_plain_numpy():
    from tbv_slam_public_amd import _lib as L, api
    rec = np.zeros(6, L.REPLAY_FRAME_DTYPE)
    rec["n_targets"][1:] = 1
    rec["exposed"] = -1
    rec["dev"][2] = (0.0, 2e-3, 0.0)
    rec["dev"][5] = (0.0, 0.0, -3e-4)
    rec["exposed"][5] = 1
    s = api.replay_summary(rec, 1e-4, 1e-5, seq_offsets=[0, 3, 6])
    assert (s["n_no_job"], s["n_equal"], s["n_differ_exposed"], s["n_differ_not_exposed"]) == (1, 3, 1, 1)
    assert s["first_not_exposed"] == [2, -1] and s["worst_dev_differ_exposed"][2] == 3e-4 and s["worst_dev_differ_not_exposed"][1] == 2e-3


def test_cpp_mirror_compiles_against_the_stand_ins(tmp_path):
    exe = str(tmp_path / "replay_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "replay_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    import torch
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    lines = r.stdout.split()
    assert lines[0] == b"160"
    if not torch.cuda.is_available():
        assert r.returncode == 2, (r.returncode, r.stderr)
        return
    assert r.returncode == 0, r.stderr
    v = [int(x) for x in lines[1:]]
    assert v[0:3] == [1, 1, 0]                                             # the first keyframe, without a job
    assert v[4:6] == [0, 1] and v[7:9] == [0, 1]                           # two frames standing still on it: no keyframes, one target each
