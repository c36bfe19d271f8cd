// PauliSectorOperator<T> (include/lambda_lanczos_hip/common.hpp) in the reference's idiom: the ground state of the Heisenberg ring
// of 12 spins in the sector of 6 flipped spins against the same run with a host mv_mul lambda over the same sector, one
// Exponentiator step exp(-i H dt) that keeps the norm, and the refusal of an H that does not conserve S_z.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/exponentiator.hpp>
#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

static std::vector<ll::PauliTerm> heisenberg_ring(int L, double J) {
  std::vector<ll::PauliTerm> terms;
  for (int j = 0; j < L; ++j) {
    const uint64_t m = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
    terms.push_back({m, 0, 0.25 * J});  // XX
    terms.push_back({m, m, 0.25 * J});  // YY
    terms.push_back({0, m, 0.25 * J});  // ZZ
  }
  return terms;
}

int main() {
  try {
    bool ok = true;
    const int L = 12, n_down = 6;
    const auto terms = heisenberg_ring(L, 1.0);
    // the sector by its definition: the states with n_down set bits, ascending, and their positions
    std::vector<uint32_t> states;
    std::vector<int32_t> rank((size_t)1 << L, -1);
    for (uint32_t s = 0; s < ((uint32_t)1 << L); ++s)
      if (__builtin_popcount(s) == n_down) {
        rank[s] = (int32_t)states.size();
        states.push_back(s);
      }
    const size_t n = states.size();
    ll::PauliSectorOperator<double> H(L, n_down, terms);
    bool good = (size_t)H.size() == n && n == 924 && H.device_bytes() >= (int64_t)(4 * n);
    // the same Hamiltonian as the user's own mv_mul over the sector, by the definition of the terms
    auto mv_mul = [&](const std::vector<double>& in, std::vector<double>& out) {
      for (size_t i = 0; i < n; ++i) {
        for (const auto& t : terms) {
          const uint32_t src = states[i] ^ (uint32_t)t.x_mask;
          if (rank[src] < 0) continue;
          const int ny = __builtin_popcountll(t.x_mask & t.z_mask);
          const double sign = ((__builtin_popcountll(src & t.z_mask) + ny / 2) & 1) ? -1.0 : 1.0;
          out[i] += sign * t.coef * in[(size_t)rank[src]];
        }
      }
    };
    double e_dev, e_host;
    std::vector<double> v_dev, v_host, start(n);
    for (size_t i = 0; i < n; ++i) start[i] = std::sin(0.37 * (double)(i + 1));
    for (int which = 0; which < 2; ++which) {
      ll::LambdaLanczos<double> engine = which ? ll::LambdaLanczos<double>(mv_mul, n, false, 1) : ll::LambdaLanczos<double>(H, n, false, 1);
      engine.eigenvalue_offset = -H.inf_norm();
      engine.init_vector = [&](std::vector<double>& v) { v = start; };
      engine.run(which ? e_host : e_dev, which ? v_host : v_dev);
    }
    good = good && std::fabs(e_dev - e_host) <= 1e-10 * std::fmax(1.0, std::fabs(e_host - H.inf_norm())) && v_dev.size() == n;
    std::printf("ring L = 12, sector of 6: device %.15f, host mv_mul %.15f, %zu states: %s\n", e_dev, e_host, n, good ? "ok" : "WRONG");
    ok = ok && good;

    typedef std::complex<double> Z;
    auto zterms = terms;
    zterms.push_back({0x3, 0x2, 0.3});   // X0 Y1 - Y0 X1: a complex Hermitian matrix that conserves S_z
    zterms.push_back({0x3, 0x1, -0.3});
    ll::PauliSectorOperator<Z> Hz(L, n_down, zterms);
    ll::Exponentiator<Z> expo(Hz, n);
    std::vector<Z> in(n), out;
    double nin = 0, nout = 0;
    for (size_t i = 0; i < n; ++i) {
      in[i] = Z(std::cos(0.11 * (double)i), std::sin(0.23 * (double)i));
      nin += std::norm(in[i]);
    }
    const size_t itern = expo.run(Z(0.0, -0.05), in, out);
    for (size_t i = 0; i < n; ++i) nout += std::norm(out[i]);
    const bool unit = out.size() == n && std::fabs(std::sqrt(nout / nin) - 1.0) <= 1e-12;
    std::printf("exp(-i H dt): %zu iterations, |out| / |in| - 1 = %.3e: %s\n", itern, std::sqrt(nout / nin) - 1.0, unit ? "ok" : "WRONG");
    ok = ok && unit;

    bool refused = false;
    try {
      auto bad = terms;
      bad.push_back({0x1, 0, -1.5});  // a field along x
      ll::PauliSectorOperator<double> Hb(L, n_down, bad);
    } catch (const ll::Error& e) {
      refused = std::strstr(e.what(), "conserve S_z") != nullptr && std::strstr(e.what(), "0x1") != nullptr;
      std::printf("a field along x is refused: %s\n", e.what());
    }
    ok = ok && refused;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
