"""CPU: the owners of long-lived device memory (tbv_slam_public_amd/csrc/owned.hpp), bound to counting stand-ins for the HIP
free functions by a stand-alone program (tests/cpp/owned_check.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owned_moves_and_early_returns(tmp_path):
    """An owner moved from and reset, a slab that travels from a scan into the free list and back, an early return between an
    allocation and its hand-over, a handle struct whose stream goes last: every block is freed exactly once and the counts
    balance at exit.  Run plainly and under the host AddressSanitizer (which adds leaks and uses after free)."""
    src = os.path.join(ROOT, "tests", "cpp", "owned_check.cpp")
    for flags in ([], ["-fsanitize=address", "-fno-omit-frame-pointer", "-g"]):
        exe = str(tmp_path / ("owned_check" + ("_asan" if flags else "")))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        allocs, frees = (int(x) for x in r.stdout.split()[:2])
        assert allocs == frees == 18, r.stdout
