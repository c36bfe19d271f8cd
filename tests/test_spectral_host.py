"""CPU-side checks of the spectral-function surface: continued_fraction and spectral_function (host arithmetic on the coefficients
of a Lanczos run) against numpy's dense resolvent; ll_pauli_block_transfer is declared in include/lanczos_hip.h, exported by the
library and bound in the ctypes table as an untyped addition within ABI minor 5; an all-null call is refused before any device
call.  No device compute here."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import lambda_lanczos_amd as L
from lambda_lanczos_amd import _capi as capi

EPS = 2.0 ** -52


def _tridiagonal(m, seed):
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(-2.0, 2.0, m)
    beta = rng.uniform(0.1, 1.5, m)            # m entries, as a run writes them: the last one is not an element of T
    T = np.diag(alpha) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    return alpha, beta, T


@pytest.mark.parametrize("m", [1, 2, 50])
def test_continued_fraction_is_the_resolvent_entry(m):
    """continued_fraction == norm2 e_1^T (z - T)^-1 e_1 with x = (z - T)^-1 e_1 from numpy.linalg.solve, to
        |cf - norm2 x_1| <= 8 m eps kappa norm2 ||x||_2,     kappa = (max |z| + ||T||_inf) / eta.
    z - T = (omega - T) + i eta is normal with every singular value >= eta and norm <= |z| + ||T||, so kappa bounds its
    condition.  Both evaluations are backward stable on it: the bottom-up recurrence d_k = z - alpha_k - beta_k^2 / d_{k+1} keeps
    Im d_k >= eta (no small pivot) and each of its m steps — a complex division, two subtractions — is the exact step for
    entries perturbed by at most 4 u relative (u = eps / 2); LU with partial pivoting on a tridiagonal has growth <= 2 and a
    backward error of a few m u ||A||.  A backward error delta ||A|| moves the solution by kappa delta ||x||: with
    delta <= 8 m u on each side, 16 m u = 8 m eps in all.  The bound is relative to ||x||, not to |x_1|: the first entry may be
    the small one."""
    alpha, beta, T = _tridiagonal(m, 7 + m)
    eta, norm2 = 0.1, 2.75
    z = np.linspace(-4.0, 4.0, 41) + 1j * eta
    kappa = (np.max(np.abs(z)) + np.max(np.sum(np.abs(T), axis=1))) / eta
    e1 = np.zeros(m)
    e1[0] = 1.0
    x = np.array([np.linalg.solve(zz * np.eye(m) - T, e1) for zz in z])
    for b in (beta, beta[:m - 1]):               # with or without the residual norm at the end
        got = L.continued_fraction(alpha, b, z, norm2)
        assert got.shape == z.shape and got.dtype == np.complex128
        err = np.abs(got - norm2 * x[:, 0])
        bound = 8 * m * EPS * kappa * norm2 * np.linalg.norm(x, axis=1)
        print("continued fraction: m", m, "worst error / bound", float(np.max(err / bound)))
        assert np.all(err <= bound)
    assert L.continued_fraction(alpha, beta, z[3], norm2) == L.continued_fraction(alpha, beta, z, norm2)[3]   # a scalar z
    with pytest.raises(ValueError):
        L.continued_fraction([], [], z)
    if m > 2:
        with pytest.raises(ValueError):
            L.continued_fraction(alpha, beta[:m - 2], z)


def test_spectral_function_integrates_to_norm2():
    """-Im G / pi is a sum of Lorentzians of width eta with the weights norm2 |s_1k|^2 at the eigenvalues e_k of T (all within
    ||T||_inf = R of 0): over [-W, W] each misses at most 2 eta / (pi (W - R)) of its weight (the two tails of
    (1 / pi) atan), and the trapezoid rule on a Lorentzian with the step h = eta / 4 errs by O(e^(-2 pi eta / h)) ~ 1e-11."""
    m, eta, norm2, e0 = 50, 0.1, 1.7, -0.5
    alpha, beta, T = _tridiagonal(m, 3)
    R = float(np.max(np.sum(np.abs(T), axis=1)))
    W = 200.0
    omega = np.arange(-W, W + eta / 8, eta / 4)
    a = L.spectral_function(alpha, beta, omega, eta, e0=0.0, norm2=norm2)
    assert a.dtype == np.float64 and np.all(a > 0.0)
    total = float(np.sum(a[1:] + a[:-1]) * 0.5 * (eta / 4))
    assert 0.0 <= norm2 - total <= norm2 * (2 * eta / (np.pi * (W - R)) + 1e-9), (total, norm2)
    # e0 shifts the frequency axis (dyadic frequencies and e0: the shift is exact)
    dyadic = np.arange(-4.0, 4.0, 0.25)
    assert np.array_equal(L.spectral_function(alpha, beta, dyadic - e0, eta, e0=e0, norm2=norm2),
                          L.spectral_function(alpha, beta, dyadic, eta, norm2=norm2))
    assert np.array_equal(L.spectral_function(alpha, beta, dyadic, eta, norm2=norm2),
                          -L.continued_fraction(alpha, beta, dyadic + 1j * eta, norm2).imag / np.pi)


def test_the_entry_point_is_declared_exported_and_bound():
    with open(capi.HEADER_PATH) as f:
        text = f.read()
    declared = set(re.findall(r"^\s*int\s+(ll_[a-z0-9_]+)\s*\(", text, flags=re.M))
    lib = capi.lib()
    name = "ll_pauli_block_transfer"
    assert name in declared and hasattr(lib, name) and name in capi.PROTOTYPES
    assert not name.endswith(("_d", "_z", "_s", "_c"))   # untyped: the typed families keep their count
    head = text[:text.index("enum {")]
    assert "additive under minor 5" in head and name in head
    res, argtypes = capi.PROTOTYPES[name]
    assert res is C.c_int and len(argtypes) == 8


def test_an_all_null_call_is_refused_before_any_device_call():
    lib = capi.lib()
    assert lib.ll_partition(-1, 0, 0, None, None) == capi.LL_ERR_INVALID   # another text: what is read below is this call's
    assert lib.ll_pauli_block_transfer(None, None, None, 0, None, None, None, None) == capi.LL_ERR_INVALID
    assert lib.ll_last_error().decode() == "invalid argument: ll_pauli_block_transfer: null argument"


def test_the_abi_is_still_minor_five():
    lib = capi.lib()
    assert lib.ll_version() == 5 and capi.ABI_VERSION == (0, 5)
    assert lib.ll_abi_check(0, 5, C.sizeof(capi.RunStats), C.sizeof(capi.LanczosParams)) == capi.LL_OK


def test_the_python_surface_exists():
    assert list(inspect.signature(L.pauli_block_transfer).parameters) == ["source", "target", "terms", "c", "out", "return_norm2"]
    assert list(inspect.signature(L.lanczos_coefficients).parameters) == ["op", "start", "m"]
    assert list(inspect.signature(L.continued_fraction).parameters) == ["alpha", "beta", "z", "norm2"]
    assert list(inspect.signature(L.spectral_function).parameters) == ["alpha", "beta", "omega", "eta", "e0", "norm2"]
    for cls in (L.PauliMomentumOperator, L.PauliMomentumFullOperator, L.PauliSymmetricOperator):
        assert list(inspect.signature(cls.transfer).parameters) == ["self", "terms", "c", "target", "out", "return_norm2"]
    assert "beta[k] couples alpha[k] and alpha[k + 1]" in L.continued_fraction.__doc__
