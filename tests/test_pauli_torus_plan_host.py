"""lambda-lanczos_amd/csrc/pauli_torus_plan.hpp — the host arithmetic of an Lx x Ly torus's translation group (T_x, T_y, the codes
and characters of its elements, the admission of a representative and the slices creation joins into a block's basis) — and the
torus group of csrc/pauli_expect_block_plan.hpp, by brute force (tests/cpp/pauli_torus_plan_test.cpp and
tests/cpp/pauli_expect_block_plan_torus_test.cpp state the properties).  The headers are the ones pauli_operators.cpp and
pauli_expect_block.hip include; they build with a plain host compiler, once more with the address and undefined-behaviour
sanitizers, and the programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
@pytest.mark.parametrize("name", ["pauli_torus_plan_test", "pauli_expect_block_plan_torus_test"])
def test_pauli_torus_plan_properties(tmp_path, name, sanitize):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
