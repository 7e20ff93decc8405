"""The dual sweep's workgroup -> tile order (csrc/dual_order.hpp) on the host: dual_order_check.cpp includes the header
without any HIP code and checks, for gx in 1..40, 64, 512, gy in 1..8, 32, the x-fastest order and the band order
with XB = 1, 2, 4, that the map is a bijection onto the tiles, that order 0 is the formula the sweep always had and
that the partial row is recovered.  Built with the host compiler under AddressSanitizer + UBSan and run as its own
program.  No GPU needed."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pdhg-optimal-control_amd", "csrc")


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler found (CXX, g++, c++, clang++)")


def test_dual_tile_is_a_bijection(tmp_path):
    exe = str(tmp_path / "dual_order_check")
    cmd = [_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "dual_order_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 bad" in r.stdout, r.stdout
