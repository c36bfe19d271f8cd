"""PauliTorusOperator<T> through the C++ facade (tests/cpp/pauli_torus_facade_test.cpp): compiles with a plain host compiler
against the C ABI (CPU); LambdaLanczos<double> on the block (mx, my) = (0, 0) of the 4 x 4 Heisenberg torus at n_down = 8 with the
device operator against the recorded ground energy and against the S_z-sector operator, the staggered <Z_0 Z_r> of that state, and
the refusals of an open cylinder and of a real type at a complex momentum (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pauli_torus_facade_test.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(OUT_DIR, "pauli_torus_facade_test")
LIB_DIR = os.path.join(ROOT, "lambda-lanczos_amd", "lib")


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
           "-L" + LIB_DIR, "-llanczos_hip", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_pauli_torus_facade_compiles_with_host_compiler():
    build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_pauli_torus_facade_eigen_solve():
    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
