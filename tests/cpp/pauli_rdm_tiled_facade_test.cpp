// PauliOperator<T>::reduced_density_matrix_tiled and PauliSectorOperator<T>::reduced_density_matrix_tiled (include/
// lambda_lanczos_hip/common.hpp) in the reference's idiom: one full-space case (complex double, 9 spins, seven sites in no order:
// three macro-tiles; psi as a std::vector and as a device pointer: the same bits) and one sector case (double, 10 spins, 5 down,
// seven sites), every entry against the definition rho[a][a'] = sum_e psi(a, e) conj(psi(a', e)) evaluated here in long double,
// within the bound of a double-accumulated dot product of the two fibres, 2 (n_e + 8) eps sum |psi(a, e)||psi(a', e)|; the exact
// Hermitian mirror, the exact zeros of a sector, the trace, agreement with reduced_density_matrix at four sites, and a refusal.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;
typedef std::complex<double> Z;

static int popc(uint32_t v) { return __builtin_popcount(v); }

// full[s]: the amplitude of state s (0 outside the basis)
template <typename T>
static bool check_rho(const char* what, int L, const std::vector<int>& sites, const std::vector<T>& full, const std::vector<Z>& got,
                      bool sector) {
  const int m = (int)sites.size(), dim = 1 << m;
  uint32_t sub = 0;
  for (int s : sites) sub |= 1u << s;
  bool ok = got.size() == (size_t)dim * dim;
  double worst = 0;
  int shown = 0;
  for (int a = 0; ok && a < dim; ++a) {
    for (int ap = 0; ap < dim; ++ap) {
      uint32_t sa = 0, sap = 0;
      for (int k = 0; k < m; ++k) {
        if ((a >> k) & 1) sa |= 1u << sites[(size_t)k];
        if ((ap >> k) & 1) sap |= 1u << sites[(size_t)k];
      }
      std::complex<long double> sum = 0;
      long double mag = 0;
      int ne = 0;
      for (uint32_t s = 0; s < (1u << L); ++s) {
        if (s & sub) continue;
        ++ne;
        const std::complex<long double> x(full[s | sa]), y(full[s | sap]);
        sum += x * std::conj(y);
        mag += (std::fabs(x.real()) + std::fabs(x.imag())) * (std::fabs(y.real()) + std::fabs(y.imag()));
      }
      const double bound = 2.0 * (ne + 8.0) * 2.220446049250313e-16 * (double)mag + 2.220446049250313e-16 * (double)std::abs(sum) + 1e-300;
      const Z g = got[(size_t)a * dim + ap], h = got[(size_t)ap * dim + a];
      const double err = std::fmax(std::fabs(g.real() - (double)sum.real()), std::fabs(g.imag() - (double)sum.imag()));
      const bool mirrored = std::memcmp(&g, &h, sizeof(double)) == 0 && g.imag() == -h.imag() && !(g.imag() == 0.0 && std::signbit(g.imag()));
      const bool zero_ok = !(sector && popc((uint32_t)a) != popc((uint32_t)ap)) || (g == Z(0.0, 0.0) && !std::signbit(g.real()));
      if (!(err <= bound) || !mirrored || !zero_ok || (a == ap && g.imag() != 0.0)) {
        if (shown++ < 8)
          std::printf("%s: entry (%d, %d) = (%.17g, %.17g), definition (%.17Lg, %.17Lg), bound %.3g, mirrored %d, zero rule %d\n", what,
                      a, ap, g.real(), g.imag(), sum.real(), sum.imag(), bound, (int)mirrored, (int)zero_ok);
        ok = false;
      }
      worst = std::fmax(worst, err / bound);
    }
  }
  std::printf("%s: %d x %d entries, worst error / bound %.3g: %s\n", what, dim, dim, worst, ok ? "ok" : "WRONG");
  return ok;
}

int main() {
  try {
    bool ok = true;
    {  // ---- the full space, complex double
      const int L = 9;
      const size_t n = (size_t)1 << L;
      std::vector<Z> psi(n);
      for (size_t s = 0; s < n; ++s) psi[s] = Z(std::sin(0.37 * (double)(s + 1)) + 0.2, std::cos(1.3 * (double)s) - 0.1);
      const std::vector<int> sites = {8, 1, 3, 0, 5, 6, 2};
      ll::PauliOperator<Z> H(L, {{0, 3, 1.0}});
      int64_t sweeps = -1;
      const std::vector<Z> host = H.reduced_density_matrix_tiled(sites, psi, &sweeps);
      ok = check_rho("full space, psi on the host", L, sites, psi, host, false) && ok;
      double nn = 0, tr = 0;
      for (const Z& v : psi) nn += std::norm(v);
      for (int a = 0; a < 128; ++a) tr += host[(size_t)a * 129].real();
      const bool trace = std::fabs(tr - nn) <= 1e-13 * nn && sweeps == 1;
      std::printf("trace %.15f against ||psi||^2 %.15f, %lld sweep: %s\n", tr, nn, (long long)sweeps, trace ? "ok" : "WRONG");
      ok = ok && trace;
      void* dpsi = nullptr;
      ll::check(ll_malloc(H.context().get(), n * sizeof(Z), &dpsi));
      ll::check(ll_memcpy_h2d(H.context().get(), dpsi, psi.data(), n * sizeof(Z)));
      const std::vector<Z> dev = H.reduced_density_matrix_tiled(sites, (const Z*)dpsi);
      ll::check(ll_free(H.context().get(), dpsi));
      const bool same = dev.size() == host.size() && std::memcmp(dev.data(), host.data(), dev.size() * sizeof(Z)) == 0;
      std::printf("psi on the device: %s\n", same ? "the same bits" : "DIFFERENT bits");
      ok = ok && same;
      // four sites: both entry points against the same definition
      const std::vector<int> four = {7, 2, 4, 0};
      ok = check_rho("four sites, the tiled form", L, four, psi, H.reduced_density_matrix_tiled(four, psi), false) && ok;
      ok = check_rho("four sites, the one-sweep form", L, four, psi, H.reduced_density_matrix(four, psi), false) && ok;
      bool refused = false, three = false;
      try {
        (void)H.reduced_density_matrix_tiled({1, 4, 1, 0}, psi);
      } catch (const ll::Error& e) {
        refused = std::strstr(e.what(), "is repeated") != nullptr;
        std::printf("a repeated site is refused: %s\n", e.what());
      }
      try {
        (void)H.reduced_density_matrix_tiled({1, 4, 0}, psi);
      } catch (const ll::Error& e) {
        three = std::strstr(e.what(), "n_sub = 3") != nullptr;
        std::printf("three sites are refused: %s\n", e.what());
      }
      ok = ok && refused && three;
    }
    {  // ---- one S_z sector, double
      const int L = 10, nd = 5;
      std::vector<uint32_t> basis;
      for (uint32_t s = 0; s < ((uint32_t)1 << L); ++s)
        if (popc(s) == nd) basis.push_back(s);
      std::vector<double> psi(basis.size()), full((size_t)1 << L, 0.0);
      for (size_t i = 0; i < psi.size(); ++i) full[basis[i]] = psi[i] = std::sin(0.61 * (double)(i + 1)) + 0.3;
      std::vector<ll::PauliTerm> heis;
      for (int j = 0; j < L; ++j) {
        const uint64_t m = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
        heis.push_back({m, 0, 0.25});
        heis.push_back({m, m, 0.25});
        heis.push_back({0, m, 0.25});
      }
      ll::PauliSectorOperator<double> H(L, nd, heis);
      int64_t sweeps = -1;
      const std::vector<int> sites = {9, 0, 2, 4, 5, 7, 8};
      const std::vector<Z> got = H.reduced_density_matrix_tiled(sites, psi, &sweeps);
      ok = check_rho("sector (10, 5), psi on the host", L, sites, full, got, true) && sweeps == 1 && ok;
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
