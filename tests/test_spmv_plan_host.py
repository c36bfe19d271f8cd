"""lambda-lanczos_amd/csrc/spmv_plan.hpp — the host arithmetic that lays out the propagation-blocked and the 2-D tiled SpMV
images (block geometry, column map and x-slice tables, the two segment orders, the arena; tile walk, tile list and the launch order
of a sharded context) — against properties that follow from what the kernels read, by brute force over every column, segment slot
and tile of small shapes (tests/cpp/spmv_plan_test.cpp states them).  The header is the one the builders include; it builds with a
plain host compiler, once more with the address and undefined-behaviour sanitizers, and both programs run as ordinary child
processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_spmv_plan_properties(tmp_path, sanitize):
    exe = str(tmp_path / "spmv_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "spmv_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
