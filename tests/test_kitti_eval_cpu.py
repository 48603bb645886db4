"""CPU: the KITTI odometry metric.  tests/kitti_eval_cpu.py (the NumPy restatement the GPU tests check the kernels with)
reproduces the REFERENCE'S OWN recorded outputs -- tests/golden/ref_kitti_eval*.npz holds the inputs and outputs of its
eval_odom.py --align 6dof runs, copied as numbers by tests/golden/copy_reference_trajectories.py; the host helpers of the
C-ABI (KITTI reader / writer, planar conversion, the refusals) and the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kitti_eval_cpu as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ("ref_kitti_eval.npz", "ref_kitti_eval_job4.npz")
KEEP = (0, 1, 3, 4, 5, 7)
NEW = ["cfear_eval_params_default", "cfear_eval_trajectories", "cfear_eval_check", "cfear_kitti_read", "cfear_kitti_write",
       "cfear_kitti_from_xyt"]
# The restatement against the record: measured 7.1e-15 (t_err / len) and 6.9e-15 (r_err / len), EXPERIMENTS.md
# "Trajectory evaluation".  The two sides round ~40 operations on values <= 1e3 m, divided by >= 100 m, differently (LAPACK's
# LU and BLAS products against cofactors and written-out sums), so the bound is ten units of 1e3 * 2^-53 / 100 = 1.1e-15.
ROW_TOL = 1.1e-14


def load_golden(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))

    def poses(q):
        a = np.zeros((len(q), 12))
        a[:, 10] = 1.0
        a[:, KEEP] = q / 1e6
        return a
    return poses(z["est"]), poses(z["gt"]), z["rows"], str(z["result"])


@pytest.mark.parametrize("name", GOLDEN)
def test_restatement_reproduces_the_reference_record(name):
    est, gt, rows, result = load_golden(name)
    o = K.evaluate(est, gt, 10, "6dof")
    assert o["n_rows"] == len(rows)
    assert (o["first_frame"] == rows[:, 0]).all() and (o["length"] == rows[:, 3]).all()
    assert (o["speed"] == rows[:, 4]).all()                        # speed is a function of last_frame: last_frame is the record's
    dt, dr = np.abs(o["t_err"] - rows[:, 2]).max(), np.abs(o["r_err"] - rows[:, 1]).max()
    print(name, "rows", len(rows), "max |t_err/len - record|", dt, "max |r_err/len - record|", dr)
    assert dt <= ROW_TOL and dr <= ROW_TOL
    assert "".join(K.result_lines(0, o)) == result                 # the 11 figures as write_result formats them
    assert o["seg_count"].sum() == len(rows)


def test_golden_poses_are_what_a_pose_file_parses_to():
    est, gt, _, _ = load_golden(GOLDEN[0])
    assert "%.6f" % est[1, 0] == "0.997305" and "%.6f" % est[1, 1] == "-0.073367"      # the issue's non-orthonormal example
    assert est[1, 0] ** 2 + est[1, 4] ** 2 != 1.0
    _, gt4, _, _ = load_golden(GOLDEN[1])
    assert not (gt4[0] == np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0])).all()        # job_4 exercises the normalisation


def test_real_inverse_not_transpose():
    rng = np.random.default_rng(3)
    P = np.zeros((50, 12))
    A = rng.normal(size=(50, 3, 3)) + 2 * np.eye(3)
    P.reshape(50, 3, 4)[:, :, :3] = A
    P.reshape(50, 3, 4)[:, :, 3] = rng.normal(size=(50, 3)) * 100
    I = K.mul(K.inv(P), P).reshape(50, 3, 4)
    assert np.abs(I[:, :, :3] - np.eye(3)).max() < 1e-12 and np.abs(I[:, :, 3]).max() < 1e-10
    full = np.zeros((50, 4, 4))
    full[:, :3] = P.reshape(50, 3, 4)
    full[:, 3, 3] = 1
    assert np.abs(K.inv(P).reshape(50, 3, 4) - np.linalg.inv(full)[:, :3]).max() < 1e-10


def test_alignment_does_not_depend_on_the_sign_of_the_third_singular_pair():
    rng = np.random.default_rng(0)
    th = 0.7
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    x = np.concatenate([rng.normal(size=(2, 200)) * 50, np.zeros((1, 200))])
    y = R @ x
    cov = (y - y.mean(1, keepdims=True)) @ (x - x.mean(1, keepdims=True)).T / 200
    r = K.umeyama_rotation(cov)
    assert np.abs(r - R).max() < 1e-12 and abs(np.linalg.det(r) - 1) < 1e-12
    assert (cov[2] == 0).all() and (cov[:, 2] == 0).all()          # planar: the third singular value is exactly 0


def test_new_symbols_declared_exported_and_built():
    from tbv_slam_public_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cfear_hip.h")).read()
    declared = set(re.findall(r"\b(cfear_\w+)\s*\(", hdr))
    lib = L.lib()
    for s in NEW:
        assert s in declared and s in L.EXPORTS and hasattr(lib, s), s
    assert lib.cfear_abi_version() == 1
    assert C.sizeof(L.EvalParams) == 72 and L.EVAL_SUMMARY_DTYPE.itemsize == 360 and L.EVAL_ROW_DTYPE.itemsize == 48
    p = L.EvalParams()
    lib.cfear_eval_params_default(C.byref(p))
    assert (p.step_size, p.alignment, list(p.lengths)) == (10, L.EVAL_ALIGN["6dof"], [100.0 * k for k in range(1, 9)])


def test_refusals_return_their_status():
    from tbv_slam_public_amd import _lib as L, api
    lib = L.lib()

    def check(p, le, lg):
        le, lg = np.array(le, np.int32), np.array(lg, np.int32)
        return lib.cfear_eval_check(C.byref(p), le.ctypes.data, lg.ctypes.data, len(le))
    assert check(api.eval_params(), [2, 4000], [2, 4000]) == L.OK
    assert check(api.eval_params(1, "none"), [2], [2]) == L.OK
    assert check(api.eval_params(), [100, 50], [100, 51]) == L.ERR_INVALID_ARGUMENT        # the pair differs in length
    assert check(api.eval_params(), [100, 1], [100, 1]) == L.ERR_INVALID_ARGUMENT          # fewer than 2 poses
    assert check(api.eval_params(step_size=0), [100], [100]) == L.ERR_INVALID_ARGUMENT
    for al in ("scale", "7dof", "scale_7dof"):
        assert check(api.eval_params(alignment=al), [100], [100]) == L.ERR_INVALID_ARGUMENT
    with pytest.raises(L.CfearError):
        api.eval_params(alignment="similarity")
    # the Python entry refuses before it needs a device
    P = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0.0]), (5, 1))
    for kw, e, g in ((dict(), [P], [P[:4]]), (dict(), [P[:1]], [P[:1]]), (dict(step_size=0), [P], [P]),
                     (dict(alignment="7dof"), [P], [P]), (dict(), P, P[:4])):
        with pytest.raises(L.CfearError) as ei:
            api.eval_trajectories(e, g, **kw)
        assert ei.value.status == L.ERR_INVALID_ARGUMENT
    # a null context is refused as well
    assert lib.cfear_eval_trajectories(None, None, None, None, None, 0, None, None, None, 0, None) == L.ERR_INVALID_ARGUMENT


def test_kitti_reader_and_writer(tmp_path):
    from tbv_slam_public_amd import _lib as L, api
    est, _, _, _ = load_golden(GOLDEN[0])
    p12 = str(tmp_path / "00.txt")
    api.kitti_write(p12, est[:300])
    text = open(p12).read()
    lines = text.splitlines()
    assert len(lines) == 300 and lines[1].startswith("0.997305 -0.073367 0.000000 ") and not lines[1].endswith(" ")
    assert all(len(ln.split(" ")) == 12 and all(re.fullmatch(r"-?\d+\.\d{6}", t) for t in ln.split(" ")) for ln in lines)
    back = api.kitti_read(p12)
    assert (back == est[:300]).all()                                # 6-decimal values survive the round trip bit for bit
    # the 13-number form: the frame index first
    p13 = str(tmp_path / "01.txt")
    with open(p13, "w") as f:
        for i, ln in enumerate(lines):
            f.write("%d %s\n" % (i, ln))
    assert (api.kitti_read(p13) == est[:300]).all()
    # full precision input, extra blanks, an empty last line
    p = str(tmp_path / "02.txt")
    with open(p, "w") as f:
        f.write("  ".join(repr(float(v)) for v in np.arange(12) / 7.0) + " \n\n")
    assert (api.kitti_read(p) == (np.arange(12) / 7.0)[None]).all()
    for bad in ("1 2 3\n", "a b c d e f g h i j k l\n", "5 " + lines[0] + "\n", lines[0] + " 1 2\n"):
        with open(p, "w") as f:
            f.write(bad)
        with pytest.raises(L.CfearError) as ei:
            api.kitti_read(p)
        assert ei.value.status == L.ERR_FORMAT
    with pytest.raises(L.CfearError) as ei:
        api.kitti_read(str(tmp_path / "missing.txt"))
    assert ei.value.status == L.ERR_IO


def test_planar_conversion():
    from tbv_slam_public_amd import _lib as L, api
    xyt = np.array([[1.5, -2.0, 0.3], [0.0, 0.0, 0.0], [7.0, 8.0, -3.0]])
    P = api.kitti_from_xyt(xyt).reshape(3, 3, 4)
    c, s = np.cos(xyt[:, 2]), np.sin(xyt[:, 2])
    assert (P[:, 0, 0] == c).all() and (P[:, 0, 1] == -s).all() and (P[:, 1, 0] == s).all() and (P[:, 1, 1] == c).all()
    assert (P[:, :2, 3] == xyt[:, :2]).all() and (P[:, 2] == [0, 0, 1, 0]).all() and (P[:, :2, 2] == 0).all()
    # strided input: the pose field of consecutive cfear_frame_info records
    info = np.zeros(3, L.FRAMEINFO_DTYPE)
    info["pose"] = xyt
    out = np.zeros((3, 12))
    assert L.lib().cfear_kitti_from_xyt(info.ctypes.data, 3, L.FRAMEINFO_DTYPE.itemsize // 8, out.ctypes.data) == L.OK
    assert (out.reshape(3, 3, 4) == P).all()


def test_cpp_eval_wrapper_compiles(tmp_path):
    """Compile and link only: running it needs a GPU (tests/test_gpu_kitti_eval.py::test_cpp_wrapper_runs)."""
    import subprocess
    exe = str(tmp_path / "eval_signature")
    so_dir = os.path.join(ROOT, "tbv_slam_public_amd")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "standin"), os.path.join(ROOT, "tests", "cpp", "eval_signature.cpp"),
                           "-o", exe, "-L", so_dir, "-lcfear_hip", "-Wl,-rpath," + so_dir])
    assert os.path.exists(exe)
