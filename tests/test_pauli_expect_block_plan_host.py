"""lambda-lanczos_amd/csrc/pauli_expect_block_plan.hpp — the host planning of ll_pauli_expect_block (the images of a string under a
ring's symmetry group, their merged signed multiplicities, the term tables of the group average, the zero rules, the batches and
the map back to the caller's order) — by brute force over all strings on 4 to 6 sites and all group choices
(tests/cpp/pauli_expect_block_plan_test.cpp states the properties).  The header is the one pauli_expect_block.hip includes; it
builds with a plain host compiler, once more with the address and undefined-behaviour sanitizers, and both programs run as
ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pauli_expect_block_plan_properties(tmp_path, sanitize):
    exe = str(tmp_path / "pauli_expect_block_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "pauli_expect_block_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
