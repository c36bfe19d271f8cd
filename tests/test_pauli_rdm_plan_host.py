"""lambda-lanczos_amd/csrc/pauli_rdm_plan.hpp — the host planning of ll_pauli_rdm (the site checks, the deposit masks below and
above the tile, the super-tiles, the tile and batch sizes inside the LDS budget, the thread-to-entry map, the popcount a sector's
environment configuration admits) — against properties that follow from what the kernels read, by brute force over site lists of
every m at up to 12 sites and several tile sizes (tests/cpp/pauli_rdm_plan_test.cpp states them).  The header is the one
pauli_rdm.hip includes; it builds with a plain host compiler, once more with the address and undefined-behaviour sanitizers, and
both programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pauli_rdm_plan_properties(tmp_path, sanitize):
    exe = str(tmp_path / "pauli_rdm_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "pauli_rdm_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_von_neumann_entropy_of_known_spectra(tmp_path, sanitize):
    """include/lambda_lanczos_hip/entropy.hpp (host only: cyclic Jacobi on a Hermitian matrix) on U diag(p) U^H with a fixed
    unitary, within 8 eta(64 eps ||rho||_F) of -sum p ln p (tests/cpp/entropy_test.cpp)."""
    exe = str(tmp_path / "entropy_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "entropy_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert "\n0 failures" in r.stdout and "WRONG" not in r.stdout
