// PauliSymmetricOperator<T> (include/lambda_lanczos_hip/common.hpp) in the reference's idiom: on the transverse-field Ising ring
// of 12 spins LambdaLanczos<double> finds the ground energy in the block of momentum 0, parity +1 and spin inversion +1 (122 of
// the 4096 states), and the same run with the full-space PauliOperator<double> gives the same energy — the ground state of the
// ring carries these labels; the block of parity -1 lies above it; the image stays O(D); an empty block and a longitudinal field
// under the spin flip are refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

static std::vector<ll::PauliTerm> tfim(int L, double J, double h) {
  std::vector<ll::PauliTerm> terms;
  for (int j = 0; j < L; ++j) terms.push_back({0, ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L)), -J});  // ZZ
  for (int j = 0; j < L; ++j) terms.push_back({(uint64_t)1 << j, 0, -h});                                    // X
  return terms;
}

template <typename Engine> static double ground(Engine& engine, size_t n, double offset) {
  std::vector<double> start(n), v;
  for (size_t i = 0; i < n; ++i) start[i] = std::sin(0.37 * (double)(i + 1)) + 1.5;
  engine.eigenvalue_offset = offset;
  engine.init_vector = [&](std::vector<double>& x) { x = start; };
  double e = 0;
  engine.run(e, v);
  return e;
}

int main() {
  try {
    bool ok = true;
    const int L = 12;
    const auto terms = tfim(L, 1.0, 0.7);
    ll::PauliSymmetricOperator<double> Hs(L, 0, terms, +1, +1), Hodd(L, 0, terms, -1, +1);
    ll::PauliOperator<double> H(L, terms);
    const size_t n = (size_t)Hs.size(), n_odd = (size_t)Hodd.size(), n_full = (size_t)H.size();
    const double norm = Hs.inf_norm();
    ll::LambdaLanczos<double> in_block(Hs, n, false, 1), in_odd(Hodd, n_odd, false, 1), in_full(H, n_full, false, 1);
    const double e_block = ground(in_block, n, -norm), e_odd = ground(in_odd, n_odd, -norm), e_full = ground(in_full, n_full, -norm);
    const double scale = std::fmax(1.0, std::fabs(e_full - norm));
    const bool good = n == 122 && n_full == 4096 && Hs.device_bytes() <= (int64_t)(8 * n + 192 * 1024) &&
                      std::fabs(norm - (12 * 1.0 + 12 * 0.7)) <= 1e-12 && std::fabs(e_block - e_full) <= 1e-10 * scale &&
                      e_odd > e_full + 0.1;
    std::printf("TFIM ring L = 12, block (0, +, +) (%lld states, %lld device bytes): %.15f, all 4096 states %.15f, block (0, -, +) "
                "(%lld states) %.15f: %s\n",
                (long long)n, (long long)Hs.device_bytes(), e_block, e_full, (long long)n_odd, e_odd, good ? "ok" : "WRONG");
    ok = ok && good;

    bool empty_refused = false, field_refused = false;
    try {
      ll::PauliSymmetricOperator<double> He(4, 0, tfim(4, 1.0, 0.7), -1, 0);
    } catch (const ll::Error& e) {
      empty_refused = std::strstr(e.what(), "is empty") != nullptr;
      std::printf("an empty block is refused: %s\n", e.what());
    }
    try {
      auto with_field = terms;
      for (int j = 0; j < L; ++j) with_field.push_back({0, (uint64_t)1 << j, -0.3});
      ll::PauliSymmetricOperator<double> Hf(L, 0, with_field, 0, +1);
    } catch (const ll::Error& e) {
      field_refused = std::strstr(e.what(), "global spin flip") != nullptr && std::strstr(e.what(), "z_mask") != nullptr;
      std::printf("a longitudinal field is refused under the spin flip: %s\n", e.what());
    }
    ok = ok && empty_refused && field_refused;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
