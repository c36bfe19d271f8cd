"""lambda-lanczos_amd/csrc/pauli_rdm_tiled_plan.hpp — the host planning of ll_pauli_rdm_tiled (the internal row order, the
macro-tiles, the panel load map, split-K, the MFMA lane maps, the sector's admission and skip rules) — against properties that
follow from what the kernels read, by brute force over m = 4 .. 9 at up to 12 sites, and a CPU emulation of the kernel pair through
the same functions on integer data (tests/cpp/pauli_rdm_tiled_plan_test.cpp states them).  The header is the one
pauli_rdm_tiled.hip includes; it builds with a plain host compiler, once more with the address and undefined-behaviour
sanitizers, and both programs run as ordinary child processes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pauli_rdm_tiled_plan_properties(tmp_path, sanitize):
    exe = str(tmp_path / "pauli_rdm_tiled_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + sanitize +
                   [os.path.join(ROOT, "tests", "cpp", "pauli_rdm_tiled_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout
