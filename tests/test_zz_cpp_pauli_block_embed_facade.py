"""expand, project and reduced_density_matrix of the three block operators through the C++ facade
(tests/cpp/pauli_block_embed_facade_test.cpp): compiles with a plain host compiler against the C ABI (CPU); on a ring of 12 spins a
momentum block into its sector and the full space and a symmetric block into the full space against the embedding formed in the
program from its definition, the round trip, device pointers against vectors, the entropy through entropy.hpp and a refusal (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pauli_block_embed_facade_test.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(OUT_DIR, "pauli_block_embed_facade_test")
LIB_DIR = os.path.join(ROOT, "lambda-lanczos_amd", "lib")


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
           "-L" + LIB_DIR, "-llanczos_hip", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_pauli_block_embed_facade_compiles_with_host_compiler():
    build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_pauli_block_embed_facade_values():
    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
