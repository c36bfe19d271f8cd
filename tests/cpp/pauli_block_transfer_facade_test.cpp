// transfer of the momentum-block operators (include/lambda_lanczos_hip/common.hpp) and the continued fraction of
// include/lambda_lanczos_hip/spectral.hpp in the reference's idiom, on a ring of 6 spins: the full-space blocks m = 0 -> m = 2
// (complex double; -0.5 Z_0 + 1.25 Y_0 Z_1, which does not commute with the translation) and the sector blocks (n_down = 3)
// m = 3 -> m = 0 (double; Z_0).  The program prints its results — `phi <case> <k> <re> <im>`, `norm2 <case> <v>`,
// `cf <k> <re> <im>`, `spec <k> <v>` with 17 significant digits — and tests/test_zz_cpp_pauli_block_transfer_facade.py holds them
// against the Python reference (generators.pauli_block_transfer_np, continued_fraction).  Checked here: a std::vector and a
// device pointer give the same bits, norm2 is the sum of the squares, no terms give +0.0, and a symmetric block is refused.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

int main() {
  try {
    bool ok = true;
    typedef std::complex<double> Z;
    const int L = 6;
    std::vector<ll::PauliTerm> heis, tfim;
    for (int j = 0; j < L; ++j) {
      const uint64_t q = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
      heis.push_back({q, 0, 0.25});
      heis.push_back({q, q, 0.25});
      heis.push_back({0, q, 0.2});
      tfim.push_back({0, q, -1.0});
      tfim.push_back({(uint64_t)1 << j, 0, -0.7});
    }
    {  // ---- the full space, complex double, m = 0 -> m = 2
      ll::PauliMomentumFullOperator<Z> S(L, 0, tfim), T(L, 2, tfim);
      const std::vector<ll::PauliTerm> terms = {{0, 1, -0.5}, {1, 3, 1.25}};
      std::vector<Z> c((size_t)S.size());
      for (size_t i = 0; i < c.size(); ++i) c[i] = Z(std::sin(0.37 * (double)(i + 1)) + 0.2, std::cos(1.3 * (double)i) - 0.1);
      double norm2 = -1.0;
      const std::vector<Z> phi = S.transfer(T, terms, c, &norm2);
      ok = ok && (int64_t)phi.size() == T.size();
      for (size_t k = 0; k < phi.size(); ++k) std::printf("phi full %zu %.17g %.17g\n", k, phi[k].real(), phi[k].imag());
      std::printf("norm2 full %.17g\n", norm2);
      double sq = 0;
      for (const Z& v : phi) sq += std::norm(v);
      ok = ok && std::fabs(norm2 - sq) <= 1e-13 * sq && sq > 0;
      // device pointers: the same bits
      void *dc = nullptr, *dphi = nullptr;
      ll::check(ll_malloc(S.context().get(), c.size() * sizeof(Z), &dc));
      ll::check(ll_malloc(S.context().get(), phi.size() * sizeof(Z), &dphi));
      ll::check(ll_memcpy_h2d(S.context().get(), dc, c.data(), c.size() * sizeof(Z)));
      double norm2_dev = -1.0;
      S.transfer(T, terms, (const Z*)dc, (Z*)dphi, &norm2_dev);
      std::vector<Z> from_dev(phi.size());
      ll::check(ll_memcpy_d2h(S.context().get(), from_dev.data(), dphi, phi.size() * sizeof(Z)));
      ll::check(ll_free(S.context().get(), dc));
      ll::check(ll_free(S.context().get(), dphi));
      const bool same = std::memcmp(from_dev.data(), phi.data(), phi.size() * sizeof(Z)) == 0 && norm2_dev == norm2;
      std::printf("c and phi on the device: %s\n", same ? "the same bits" : "DIFFERENT bits");
      ok = ok && same;
      // no terms: +0.0
      const std::vector<Z> none = S.transfer(T, {}, c, &norm2);
      bool zero = norm2 == 0.0 && !std::signbit(norm2);
      for (const Z& v : none) zero = zero && v == Z(0, 0) && !std::signbit(v.real()) && !std::signbit(v.imag());
      std::printf("no terms: %s\n", zero ? "+0.0" : "WRONG");
      ok = ok && zero;
      // a momentum / reflection / spin-inversion block is refused
      bool refused = false;
      try {
        ll::PauliSymmetricOperator<Z> Y(L, 0, tfim, 1, 0);
        (void)Y.transfer(T, terms, std::vector<Z>((size_t)Y.size(), Z(1, 0)));
      } catch (const ll::Error& e) {
        refused = std::strstr(e.what(), "semi-momentum") != nullptr;
        std::printf("a symmetric block is refused: %s\n", e.what());
      }
      ok = ok && refused;
    }
    {  // ---- the sector n_down = 3, double, m = 3 -> m = 0
      ll::PauliMomentumOperator<double> S(L, 3, 3, heis), T(L, 3, 0, heis);
      std::vector<double> c((size_t)S.size());
      for (size_t i = 0; i < c.size(); ++i) c[i] = std::sin(0.61 * (double)(i + 1)) + 0.3;
      double norm2 = -1.0;
      const std::vector<double> phi = S.transfer(T, {{0, 1, 1.0}}, c, &norm2);
      ok = ok && (int64_t)phi.size() == T.size();
      for (size_t k = 0; k < phi.size(); ++k) std::printf("phi sector %zu %.17g %.17g\n", k, phi[k], 0.0);
      std::printf("norm2 sector %.17g\n", norm2);
    }
    {  // ---- spectral.hpp
      std::vector<double> alpha, beta;
      for (int k = 0; k < 5; ++k) {
        alpha.push_back(std::cos((double)k));
        beta.push_back(0.5 + 0.1 * (double)k);
      }
      std::vector<double> omega;
      for (int k = 0; k < 4; ++k) {
        omega.push_back(0.3 * (double)k - 1.0);
        const Z g = ll::continued_fraction(alpha, beta, Z(omega.back(), 0.1), 2.5);
        std::printf("cf %d %.17g %.17g\n", k, g.real(), g.imag());
      }
      const std::vector<double> spec = ll::spectral_function(alpha, beta, omega, 0.1, -0.25, 2.5);
      for (size_t k = 0; k < spec.size(); ++k) std::printf("spec %zu %.17g\n", k, spec[k]);
      std::vector<double> short_beta(beta.begin(), beta.begin() + 4);
      ok = ok && ll::continued_fraction(alpha, short_beta, Z(0.2, 0.1)) == ll::continued_fraction(alpha, beta, Z(0.2, 0.1));
      bool threw = false;
      try {
        (void)ll::continued_fraction({}, {}, Z(0, 1));
      } catch (const std::invalid_argument&) {
        threw = true;
      }
      ok = ok && threw;
    }
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const ll::Error& e) {
    std::printf("%s\n", e.what());
    return std::strstr(e.what(), "no CPU fallback") != nullptr ? 2 : 3;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 3;
  }
}
