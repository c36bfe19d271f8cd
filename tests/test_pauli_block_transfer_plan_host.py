"""lambda-lanczos_amd/csrc/pauli_block_transfer_plan.hpp — the host planning of ll_pauli_block_transfer (the rotated images of a
string with their phases, the integer drop rule, the merged weights, the term tables, the sector rule and the admitted block
pairs) — by brute force over all strings on 4 to 6 sites and all momenta (tests/cpp/pauli_block_transfer_plan_test.cpp states
the properties).  The header is the one pauli_block_transfer.hip includes; it builds with a plain host compiler, once more with
the address and undefined-behaviour sanitizers, and both programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pauli_block_transfer_plan_properties(tmp_path, sanitize):
    exe = str(tmp_path / "pauli_block_transfer_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "pauli_block_transfer_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
