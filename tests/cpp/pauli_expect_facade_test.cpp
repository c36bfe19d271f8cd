// PauliOperator<T>::expectation and PauliSectorOperator<T>::expectation (include/lambda_lanczos_hip/common.hpp) in the reference's
// idiom: one full-space case (complex double, 7 spins; psi as a std::vector and as a device pointer: the same bits) and one
// sector case (double, 8 spins, 4 down), every value against the definition
//   coef * sum_s Re[conj(psi(s ^ x)) i^nY (-1)^popcount(s & z) psi(s)]
// evaluated here in long double, within the bound of a double-accumulated dot product, 2 (n + 8) eps |coef| sum |psi(s ^ x)||psi(s)|;
// the identity returns ||psi||^2, an odd nY on a real type and an odd number of flips in a sector return +0.0 without a sweep.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

static int popc(uint64_t v) { return __builtin_popcountll(v); }

template <typename T>
static void by_definition(const ll::PauliTerm& t, const std::vector<uint32_t>& basis, const std::vector<T>& psi, double& value,
                          double& bound) {
  static const std::complex<long double> iy[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
  const std::complex<long double> ph = iy[popc(t.x_mask & t.z_mask) & 3];
  long double sum = 0, mag = 0;
  for (size_t i = 0; i < basis.size(); ++i) {
    const uint32_t p = basis[i] ^ (uint32_t)t.x_mask;
    const auto it = std::lower_bound(basis.begin(), basis.end(), p);
    if (it == basis.end() || *it != p) continue;
    const std::complex<long double> a(psi[(size_t)(it - basis.begin())]), b(psi[i]);
    const long double sign = (popc(basis[i] & t.z_mask) & 1) ? -1.0L : 1.0L;
    sum += (std::conj(a) * ph * sign * b).real();
    mag += (std::fabs(a.real()) + std::fabs(a.imag())) * (std::fabs(b.real()) + std::fabs(b.imag()));
  }
  value = (double)((long double)t.coef * sum);
  bound = 2.0 * ((double)basis.size() + 8.0) * 2.220446049250313e-16 * std::fabs(t.coef) * (double)mag + 2.220446049250313e-16 * std::fabs(value);
}

template <typename T>
static bool check_all(const char* what, const std::vector<ll::PauliTerm>& obs, const std::vector<uint32_t>& basis,
                      const std::vector<T>& psi, const std::vector<double>& got) {
  bool ok = got.size() == obs.size();
  double worst = 0;
  for (size_t j = 0; ok && j < obs.size(); ++j) {
    double want, bound;
    by_definition(obs[j], basis, psi, want, bound);
    const double err = std::fabs(got[j] - want);
    if (!(err <= bound)) {
      std::printf("%s: observable %zu (x %llx z %llx): %.17g, definition %.17g, bound %.3g\n", what, j, (unsigned long long)obs[j].x_mask,
                  (unsigned long long)obs[j].z_mask, got[j], want, bound);
      ok = false;
    }
    if (bound > 0) worst = std::fmax(worst, err / bound);
  }
  std::printf("%s: %zu observables, worst error / bound %.3g: %s\n", what, obs.size(), worst, ok ? "ok" : "WRONG");
  return ok;
}

int main() {
  try {
    bool ok = true;
    {  // ---- the full space, complex double
      typedef std::complex<double> Z;
      const int L = 7;
      const size_t n = (size_t)1 << L;
      std::vector<uint32_t> basis(n);
      std::vector<Z> psi(n);
      for (size_t s = 0; s < n; ++s) {
        basis[s] = (uint32_t)s;
        psi[s] = Z(std::sin(0.37 * (double)(s + 1)) + 0.2, std::cos(1.3 * (double)s) - 0.1);
      }
      std::vector<ll::PauliTerm> obs = {{0, 0, 1.0}};
      for (int j = 0; j < L; ++j) {
        const uint64_t b = (uint64_t)1 << j, c = (uint64_t)1 << ((j + 1) % L);
        obs.push_back({b, 0, 0.5});        // X_j
        obs.push_back({b, b, -1.25});      // Y_j
        obs.push_back({0, b, 2.0});        // Z_j
        obs.push_back({b | c, b | c, 0.25});  // Y_j Y_j+1
        obs.push_back({b | c, c, 1.0});    // X_j Y_j+1
      }
      obs.push_back({0x7f, 0x2a, -0.75});
      for (int r = 0; r < 40; ++r) obs.push_back({(uint64_t)((r * 37 + 5) & 0x7f), (uint64_t)((r * 91 + 3) & 0x7f), 0.1 * (r - 20)});
      ll::PauliOperator<Z> H(L, {{0, 3, 1.0}});
      int64_t sweeps = -1;
      const std::vector<double> host = H.expectation(obs, psi, &sweeps);
      ok = check_all("full space, psi on the host", obs, basis, psi, host) && ok;
      double nn = 0;
      for (const Z& v : psi) nn += std::norm(v);
      const bool idn = std::fabs(host[0] - nn) <= 1e-13 * nn && sweeps == (int64_t)((obs.size() + 31) / 32);
      std::printf("identity %.15f against ||psi||^2 %.15f, %lld sweeps: %s\n", host[0], nn, (long long)sweeps, idn ? "ok" : "WRONG");
      ok = ok && idn;
      void* dpsi = nullptr;
      ll::check(ll_malloc(H.context().get(), n * sizeof(Z), &dpsi));
      ll::check(ll_memcpy_h2d(H.context().get(), dpsi, psi.data(), n * sizeof(Z)));
      const std::vector<double> dev = H.expectation(obs, (const Z*)dpsi);
      ll::check(ll_free(H.context().get(), dpsi));
      const bool same = dev.size() == host.size() && std::memcmp(dev.data(), host.data(), dev.size() * sizeof(double)) == 0;
      std::printf("psi on the device: %s\n", same ? "the same bits" : "DIFFERENT bits");
      ok = ok && same;
      bool refused = false;
      try {
        (void)H.expectation({{(uint64_t)1 << L, 0, 1.0}}, psi);
      } catch (const ll::Error& e) {
        refused = std::strstr(e.what(), "at or above n_sites") != nullptr;
        std::printf("a mask bit above the chain is refused: %s\n", e.what());
      }
      ok = ok && refused;
    }
    {  // ---- one S_z sector, double
      const int L = 8, nd = 4;
      std::vector<uint32_t> basis;
      for (uint32_t s = 0; s < ((uint32_t)1 << L); ++s)
        if (popc(s) == nd) basis.push_back(s);
      std::vector<double> psi(basis.size());
      for (size_t i = 0; i < psi.size(); ++i) psi[i] = std::sin(0.61 * (double)(i + 1)) + 0.3;
      std::vector<ll::PauliTerm> heis;
      std::vector<ll::PauliTerm> obs = {{0, 0, 1.0}};
      for (int j = 0; j < L; ++j) {
        const uint64_t m = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
        heis.push_back({m, 0, 0.25});
        heis.push_back({m, m, 0.25});
        heis.push_back({0, m, 0.25});
        for (int k = j + 1; k < L; ++k) {
          const uint64_t q = ((uint64_t)1 << j) | ((uint64_t)1 << k);
          obs.push_back({q, 0, 0.25});   // X_j X_k
          obs.push_back({q, q, 0.25});   // Y_j Y_k
          obs.push_back({0, q, 0.25});   // Z_j Z_k
        }
        obs.push_back({0, (uint64_t)1 << j, 1.0});
      }
      obs.push_back({0xf0, 0x0f, 2.0});
      const size_t first_zero = obs.size();
      obs.push_back({1, 0, 1.0});        // one flip leaves the sector
      obs.push_back({3, 1, 1.0});        // one Y on a real type
      ll::PauliSectorOperator<double> H(L, nd, heis);
      int64_t sweeps = -1;
      const std::vector<double> got = H.expectation(obs, psi, &sweeps);
      ok = check_all("sector (8, 4), psi on the host", obs, basis, psi, got) && ok;
      const bool zeros = got[first_zero] == 0.0 && !std::signbit(got[first_zero]) && got[first_zero + 1] == 0.0 &&
                         !std::signbit(got[first_zero + 1]) && sweeps == (int64_t)((first_zero + 31) / 32);
      std::printf("the two identically zero strings: %g %g, %lld sweeps: %s\n", got[first_zero], got[first_zero + 1], (long long)sweeps,
                  zeros ? "ok" : "WRONG");
      ok = ok && zeros;
      int64_t none = -1;
      const std::vector<double> z2 = H.expectation({{1, 0, 1.0}, {2, 2, -3.0}}, psi, &none);
      ok = ok && none == 0 && z2[0] == 0.0 && z2[1] == 0.0;
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
