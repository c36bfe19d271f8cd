"""lambda-lanczos_amd/csrc/raw_basis.hpp and scalar_types.hpp — the host algebra that turns the coefficients of a GEMV over the
orthonormal Lanczos vectors into coefficients over the raw vectors of the pair and block forms, and prepares the packed triangle
for the in-place flush — on a construction where the orthonormal vectors are unit vectors (tests/cpp/raw_basis_test.cpp states the
cases and derives the bounds).  The headers are the ones the loop includes; they build with a plain host compiler, once more with
the address and undefined-behaviour sanitizers, and both programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_raw_basis_algebra_on_unit_vectors(tmp_path, sanitize):
    exe = str(tmp_path / "raw_basis_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "raw_basis_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
