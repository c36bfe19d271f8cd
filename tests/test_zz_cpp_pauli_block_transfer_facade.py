"""transfer of the momentum-block operators and spectral.hpp through the C++ facade
(tests/cpp/pauli_block_transfer_facade_test.cpp): compiles with a plain host compiler against the C ABI (CPU); on a ring of 6 spins
the values the program prints — a full-space pair in complex double, a sector pair in double, the continued fraction — against the
Python reference (generators.pauli_block_transfer_np at the contract of test_gpu_pauli_block_transfer.py; continued_fraction at
the bound of test_spectral_host.py), and the program's own checks: device pointers, no terms, a refusal (GPU)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pauli_block_transfer_facade_test.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(OUT_DIR, "pauli_block_transfer_facade_test")
LIB_DIR = os.path.join(ROOT, "lambda-lanczos_amd", "lib")
EPS = 2.0 ** -52


def build():
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), SRC, "-o", EXE,
           "-L" + LIB_DIR, "-llanczos_hip", "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_pauli_block_transfer_facade_compiles_with_host_compiler():
    build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_pauli_block_transfer_facade_values():
    import lambda_lanczos_amd as L
    from lambda_lanczos_amd import generators as G

    build()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
    phi, norm2, cf, spec = {"full": [], "sector": []}, {}, [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "phi":
            assert int(w[2]) == len(phi[w[1]])
            phi[w[1]].append(complex(float(w[3]), float(w[4])))
        elif w[0] == "norm2":
            norm2[w[1]] = float(w[2])
        elif w[0] == "cf":
            cf.append(complex(float(w[2]), float(w[3])))
        elif w[0] == "spec":
            spec.append(float(w[2]))
    n_sites = 6
    cases = {"full": ("momentum_full", (n_sites, 0), (n_sites, 2), [(0, 1, -0.5), (1, 3, 1.25)],
                      lambda i: np.sin(0.37 * (i + 1)) + 0.2 + 1j * (np.cos(1.3 * i) - 0.1)),
             "sector": ("momentum", (n_sites, 3, 3), (n_sites, 3, 0), [(0, 1, 1.0)], lambda i: np.sin(0.61 * (i + 1)) + 0.3)}
    for name, (kind, ss, st, terms, start) in cases.items():
        basis = G.full_momentum_basis(*ss) if kind == "momentum_full" else G.momentum_basis(*ss)
        c = start(np.arange(basis[0].shape[0], dtype=np.float64))
        want, mag = G.pauli_block_transfer_np(kind, ss, st, terms, c, return_magnitude=True)
        got = np.array(phi[name])
        assert got.shape == want.shape
        # c is formed by two libms: one more eps of |c| on every gathered term
        bound = (2.0 * (n_sites * len(terms) + 8) + 24.0 + 2.0) * EPS * mag + EPS * np.abs(want) + 1e-300
        assert np.all(np.abs(got - want) <= bound), (name, float(np.max(np.abs(got - want) / bound)))
        sq = float(np.sum(np.abs(got) ** 2))
        assert abs(norm2[name] - sq) <= 2.0 * (got.shape[0] + 8) * EPS * sq and sq > 0
    alpha, beta = np.cos(np.arange(5.0)), 0.5 + 0.1 * np.arange(5.0)
    omega = 0.3 * np.arange(4.0) - 1.0
    T = np.diag(alpha) + np.diag(beta[:4], 1) + np.diag(beta[:4], -1)

    def resolvent(z):   # (2.5 x_1, the bound of test_spectral_host.py: 8 m eps kappa norm2 ||x||)
        x = np.array([np.linalg.solve(zz * np.eye(5) - T, np.eye(5)[0]) for zz in z])
        kappa = (np.max(np.abs(z)) + np.max(np.sum(np.abs(T), axis=1))) / 0.1
        return 2.5 * x[:, 0], 8 * 5 * EPS * kappa * 2.5 * np.linalg.norm(x, axis=1)

    z = omega + 0.1j
    ref, bound = resolvent(z)
    assert np.all(np.abs(np.array(cf) - ref) <= bound)
    assert np.all(np.abs(np.array(cf) - L.continued_fraction(alpha, beta, z, 2.5)) <= bound)
    ref, bound = resolvent(z - 0.25)
    assert np.all(np.abs(np.array(spec) + ref.imag / np.pi) <= bound)
    assert np.all(np.abs(np.array(spec) - L.spectral_function(alpha, beta, omega, 0.1, e0=-0.25, norm2=2.5)) <= bound)
