// von_neumann_entropy (include/lambda_lanczos_hip/entropy.hpp: cyclic Jacobi on a Hermitian matrix, host only) on
// rho = U diag(p) U^H with a fixed 8 x 8 unitary U = u1 (x) u2 (x) u3 written out below and several spectra p, against
// -sum p ln p.  Tolerance: the eigenvalues of the rho that was formed differ from p, and the Jacobi eigenvalues from those, by at
// most delta = 64 eps ||rho||_F in all (8 x 8 products and a few eps ||rho||_F of the method); with eta(x) = -x ln x and
// |eta(x) - eta(y)| <= eta(|x - y|) for |x - y| <= 1/2 the entropy moves by at most 8 eta(delta).  Also: diag(1, 0) -> 0,
// I / 4 -> ln 4, a matrix that is not normalised, the largest size (64 x 64, maximally mixed -> 6 ln 2; there the products are 64
// long and 64 eigenvalues move: 64 eta(64 * 64 eps ||rho||_F)), and dim 65 refused.
// Built (plain, and with the address and undefined-behaviour sanitizers) and run by tests/test_pauli_rdm_plan_host.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include <lambda_lanczos_hip/entropy.hpp>

typedef std::complex<double> Z;
static int fails = 0;
static double eta(double x) { return x > 0.0 ? -x * std::log(x) : 0.0; }
static void require(bool ok, const char* what, double got, double want, double tol) {
  std::printf("%s: %.17g, exact %.17g, tolerance %.3g: %s\n", what, got, want, tol, ok ? "ok" : "WRONG");
  if (!ok) ++fails;
}

int main() {
  const double eps = 2.220446049250313e-16, r = 0.70710678118654752440;
  const Z I(0.0, 1.0);
  const Z u1[2][2] = {{0.6, 0.8}, {-0.8, 0.6}};
  const Z u2[2][2] = {{0.6, 0.8 * I}, {0.8 * I, 0.6}};
  const Z u3[2][2] = {{r, r}, {r * I, -r * I}};
  Z U[8][8];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) U[i][j] = u1[i >> 2][j >> 2] * u2[(i >> 1) & 1][(j >> 1) & 1] * u3[i & 1][j & 1];
  const double spectra[4][8] = {{0.3, 0.25, 0.2, 0.1, 0.08, 0.04, 0.02, 0.01},
                                {0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125, 0.125},
                                {1.0, 0, 0, 0, 0, 0, 0, 0},
                                {0.5, 0.5, 0, 0, 0, 0, 0, 0}};
  for (int k = 0; k < 4; ++k) {
    std::vector<Z> rho(64);
    double want = 0.0, fro2 = 0.0;
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 8; ++j) {
        Z v = 0.0;
        for (int l = 0; l < 8; ++l) v += U[i][l] * spectra[k][l] * std::conj(U[j][l]);
        rho[(size_t)(i * 8 + j)] = v;
        fro2 += std::norm(v);
      }
    for (int l = 0; l < 8; ++l) want += eta(spectra[k][l]);
    const double delta = 64.0 * eps * std::sqrt(fro2), tol = 8.0 * eta(delta);
    const double got = lambda_lanczos_hip::von_neumann_entropy(rho, 8);
    char what[64];
    std::snprintf(what, sizeof what, "U diag(p%d) U^H", k);
    require(std::fabs(got - want) <= tol, what, got, want, tol);
  }
  {
    const std::vector<Z> pure = {1.0, 0.0, 0.0, 0.0};
    const double got = lambda_lanczos_hip::von_neumann_entropy(pure, 2);
    require(got == 0.0 && !std::signbit(got), "diag(1, 0)", got, 0.0, 0.0);
    std::vector<Z> mixed(16, 0.0), scaled(4, 0.0);
    for (int i = 0; i < 4; ++i) mixed[(size_t)(i * 5)] = 0.25;
    const double tol = 4.0 * eta(64.0 * eps * 0.5);
    require(std::fabs(lambda_lanczos_hip::von_neumann_entropy(mixed, 4) - std::log(4.0)) <= tol, "I / 4",
            lambda_lanczos_hip::von_neumann_entropy(mixed, 4), std::log(4.0), tol);
    scaled[0] = scaled[3] = 3.0;  // not normalised: rho / tr rho counts
    require(std::fabs(lambda_lanczos_hip::von_neumann_entropy(scaled, 2) - std::log(2.0)) <= tol, "3 I", lambda_lanczos_hip::von_neumann_entropy(scaled, 2),
            std::log(2.0), tol);
  }
  {  // 64 x 64: what six sites that each cut a singlet give, (I / 2)^(x6) = I / 64, formed as (U (x) U) (I / 64) (U (x) U)^H
    std::vector<Z> rho(64 * 64);
    double fro2 = 0.0;
    for (int i = 0; i < 64; ++i)
      for (int j = 0; j < 64; ++j) {
        Z v = 0.0;
        for (int l = 0; l < 8; ++l)
          for (int q = 0; q < 8; ++q) v += U[i >> 3][l] * U[i & 7][q] * (1.0 / 64.0) * std::conj(U[j >> 3][l] * U[j & 7][q]);
        rho[(size_t)(i * 64 + j)] = v;
        fro2 += std::norm(v);
      }
    const double delta = 64.0 * 64.0 * eps * std::sqrt(fro2), tol = 64.0 * eta(delta);
    const double got = lambda_lanczos_hip::von_neumann_entropy(rho, 64);
    require(std::fabs(got - 6.0 * std::log(2.0)) <= tol, "dim 64, maximally mixed, rotated", got, 6.0 * std::log(2.0), tol);
  }
  bool refused = false;
  try {
    (void)lambda_lanczos_hip::von_neumann_entropy(std::vector<Z>(65 * 65), 65);
  } catch (const std::invalid_argument&) {
    refused = true;
  }
  require(refused, "dim 65 is refused", refused, 1.0, 0.0);
  std::printf("%d failures\n", fails);
  return fails == 0 ? 0 : 1;
}
