"""CPU: the matcher's launch arithmetic (tbv_slam_public_amd/csrc/reg_layout.hpp) and the planar pose algebra (pose2d.hpp) as
a stand-alone program, tests/cpp/registration_check.cpp, compiled without HIP: once plain and once under the host sanitizers.

Run without arguments the program checks the LDS map's invariants, the job stride, the scratch size and the pose identities.
Run with `hint` it prints mt_fit and the launch hint for the sizes on its standard input, and every line must agree with
tests/verify_cases.py's restatement of the same arithmetic (_mt_fit, predict_hint), which chooses the GPU tests' inputs: a
drift on either side fails here."""
import os
import subprocess

import pytest

from tests import verify_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("registration_check")
    src = os.path.join(ROOT, "tests", "cpp", "registration_check.cpp")
    exes = []
    for flags in ([], SAN):
        exe = str(d / ("registration_check" + ("_san" if flags else "")))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *flags, src, "-o", exe])
        exes.append(exe)
    return exes


def test_registration_headers_stand_alone(programs):
    for exe in programs:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split()[-1] == "ok", r.stdout + r.stderr


def test_verify_cases_restates_the_launch_hint(programs):
    cases = [(n, cost, huber) for n in range(3201) for cost in ("P2P", "P2L", "P2D") for huber in (1, 0)]
    text = "".join("%d %s %d\n" % c for c in cases)
    outs = []
    for exe in programs:
        r = subprocess.run([exe, "hint"], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-400:] + r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert len(lines) == len(cases)
    for (n, cost, huber), line in zip(cases, lines):
        got = [bool(int(x)) for x in line.split()]
        pad, f = (n + 7) & ~7, V.DENSE_FIELDS[cost]
        regular = V.K_LDS_CU // 4 if huber else (V.K_LDS_CU // 3) & ~255
        want = []
        for lds, gm in ((V.K_LDS_PAIRS, False), (regular, False), (V.K_LDS_CU // 2 - 256 - V.K_PART_BIG, True),
                        (V.K_LDS_CU - 256 - V.K_PART_BIG, True)):
            want += list(V._mt_fit(lds, 1, pad, pad, n, f, gm))
        h = V.predict_hint(n, cost, bool(huber))
        want += [h["small_pairs"], h["big_pass"], h["whole_cu"]]
        assert got == want, (n, cost, huber, got, want)
