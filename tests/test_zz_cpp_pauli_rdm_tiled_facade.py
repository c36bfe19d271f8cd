"""PauliOperator<T>::reduced_density_matrix_tiled and PauliSectorOperator<T>::reduced_density_matrix_tiled through the C++ facade
(tests/cpp/pauli_rdm_tiled_facade_test.cpp): compiles with a plain host compiler against the C ABI (CPU); one full-space case of
three macro-tiles and one sector case against values computed in the program from the definition, a device psi against a host psi,
the Hermitian mirror and the sector's exact zeros, both entry points at four sites and two refusals (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pauli_rdm_tiled_facade_test.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(OUT_DIR, "pauli_rdm_tiled_facade_test")
LIB_DIR = os.path.join(ROOT, "lambda-lanczos_amd", "lib")


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
           "-L" + LIB_DIR, "-llanczos_hip", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_pauli_rdm_tiled_facade_compiles_with_host_compiler():
    build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_pauli_rdm_tiled_facade_values():
    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
