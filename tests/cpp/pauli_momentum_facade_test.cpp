// PauliMomentumOperator<T> (include/lambda_lanczos_hip/common.hpp) in the reference's idiom: on the Heisenberg ring of 12 spins,
// sector of 6 flipped spins, the ground energy of the block of momentum 0 (double) equals the sector's ground energy
// (PauliSectorOperator: the ground state of a ring of 4 k spins has momentum 0); the blocks of momentum m and L - m (complex
// double) share their lowest eigenvalue (reflection maps one to the other); the block sizes add up to the sector's; an open
// chain is refused.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

static std::vector<ll::PauliTerm> heisenberg(int L, double J, bool ring) {
  std::vector<ll::PauliTerm> terms;
  for (int j = 0; j < (ring ? L : L - 1); ++j) {
    const uint64_t m = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
    terms.push_back({m, 0, 0.25 * J});  // XX
    terms.push_back({m, m, 0.25 * J});  // YY
    terms.push_back({0, m, 0.25 * J});  // ZZ
  }
  return terms;
}

template <typename T, typename Op> static double ground(Op& H) {
  const size_t n = (size_t)H.size();
  std::vector<T> start(n), v;
  for (size_t i = 0; i < n; ++i) start[i] = T(std::sin(0.37 * (double)(i + 1)) + 1.5);
  ll::LambdaLanczos<T> engine(H, n, false, 1);
  engine.eigenvalue_offset = -H.inf_norm();
  engine.init_vector = [&](std::vector<T>& x) { x = start; };
  double e = 0;
  engine.run(e, v);
  return e;
}

int main() {
  try {
    bool ok = true;
    const int L = 12, n_down = 6;
    const auto terms = heisenberg(L, 1.0, true);
    ll::PauliSectorOperator<double> Hs(L, n_down, terms);
    ll::PauliMomentumOperator<double> H0(L, n_down, 0, terms);
    const double e_sec = ground<double>(Hs), e_0 = ground<double>(H0);
    const double scale = std::fmax(1.0, std::fabs(e_sec - Hs.inf_norm()));
    bool good = H0.size() == 80 && H0.device_bytes() >= (int64_t)(4 * Hs.size()) && std::fabs(e_0 - e_sec) <= 1e-10 * scale;
    std::printf("ring L = 12, sector of 6: block m = 0 (%lld states) %.15f, sector (%lld states) %.15f: %s\n", (long long)H0.size(),
                e_0, (long long)Hs.size(), e_sec, good ? "ok" : "WRONG");
    ok = ok && good;

    typedef std::complex<double> Z;
    int64_t total = 0;
    for (int m = 0; m < L; ++m) total += ll::PauliMomentumOperator<Z>(L, n_down, m, terms).size();
    ll::PauliMomentumOperator<Z> H5(L, n_down, 5, terms), H7(L, n_down, 7, terms);
    const double e_5 = ground<Z>(H5), e_7 = ground<Z>(H7);
    good = total == Hs.size() && H5.size() == H7.size() && std::fabs(e_5 - e_7) <= 1e-10 * scale && e_5 > e_0;
    std::printf("blocks m = 5 and 7 (%lld states): %.15f, %.15f; sum of the block sizes %lld: %s\n", (long long)H5.size(), e_5, e_7,
                (long long)total, good ? "ok" : "WRONG");
    ok = ok && good;

    bool refused = false;
    try {
      ll::PauliMomentumOperator<double> Hb(L, n_down, 0, heisenberg(L, 1.0, false));
    } catch (const ll::Error& e) {
      refused = std::strstr(e.what(), "translation") != nullptr && std::strstr(e.what(), "x_mask") != nullptr;
      std::printf("an open chain is refused: %s\n", e.what());
    }
    ok = ok && refused;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
