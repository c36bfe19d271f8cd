// PauliMomentumFullOperator<T> (include/lambda_lanczos_hip/common.hpp) in the reference's idiom: on the transverse-field Ising
// ring of 12 spins — an H that conserves no S_z, which the sector operators refuse — LambdaLanczos<double> finds the ground
// energy of the block of momentum 0 (352 states) with the device operator, and the same run with the user's own mv_mul lambda
// over the block's CSR matrix (built here on the host from the gather form) gives the same energy; the image stays O(D_m); an
// open chain is refused.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

static std::vector<ll::PauliTerm> tfim(int L, double J, double h, bool ring) {
  std::vector<ll::PauliTerm> terms;
  for (int j = 0; j < (ring ? L : L - 1); ++j) terms.push_back({0, ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L)), -J});  // ZZ
  for (int j = 0; j < L; ++j) terms.push_back({(uint64_t)1 << j, 0, -h});                                                     // X
  return terms;
}

// the smallest rotation of s and the orbit length
static void orbit(uint32_t s, int L, uint32_t& rep, int& period) {
  const uint32_t mask = (uint32_t)(((uint64_t)1 << L) - 1);
  rep = s;
  period = L;
  uint32_t t = s;
  for (int j = 1; j < L; ++j) {
    t = ((t << 1) | (t >> (L - 1))) & mask;
    if (t == s && period == L) period = j;
    rep = std::min(rep, t);
  }
}

struct Csr {
  std::vector<int64_t> rp;
  std::vector<int32_t> ci;
  std::vector<double> va;
};

// the block of momentum 0 by the gather form: row a, per term, weight sqrt(R_a / R_b) in the column of the partner's representative
static Csr block_m0(int L, const std::vector<ll::PauliTerm>& terms) {
  std::vector<uint32_t> reps;
  std::vector<int> per;
  for (uint32_t s = 0; s < ((uint32_t)1 << L); ++s) {
    uint32_t r;
    int p;
    orbit(s, L, r, p);
    if (r == s) {
      reps.push_back(s);
      per.push_back(p);
    }
  }
  Csr m;
  m.rp.push_back(0);
  for (size_t i = 0; i < reps.size(); ++i) {
    for (const ll::PauliTerm& t : terms) {
      const uint32_t p = reps[i] ^ (uint32_t)t.x_mask;
      uint32_t b;
      int rb;
      orbit(p, L, b, rb);
      const double sign = (__builtin_popcount(p & (uint32_t)t.z_mask) & 1) ? -1.0 : 1.0;  // no Y in this H
      m.ci.push_back((int32_t)(std::lower_bound(reps.begin(), reps.end(), b) - reps.begin()));
      m.va.push_back(sign * t.coef * std::sqrt((double)per[i] / (double)rb));
    }
    m.rp.push_back((int64_t)m.ci.size());
  }
  return m;
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
    const auto terms = tfim(L, 1.0, 0.7, true);
    ll::PauliMomentumFullOperator<double> H0(L, 0, terms);
    const size_t n = (size_t)H0.size();
    const Csr A = block_m0(L, terms);
    auto mv_mul = [&](const std::vector<double>& in, std::vector<double>& out) {
      for (size_t i = 0; i + 1 < A.rp.size(); ++i)
        for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) out[i] += A.va[(size_t)k] * in[(size_t)A.ci[(size_t)k]];
    };
    const double norm = H0.inf_norm();
    ll::LambdaLanczos<double> on_device(H0, n, false, 1), on_host(mv_mul, n, false, 1);
    const double e_dev = ground(on_device, n, -norm), e_host = ground(on_host, n, -norm);
    const double scale = std::fmax(1.0, std::fabs(e_host - norm));
    const bool good = n == 352 && A.rp.size() == n + 1 && H0.device_bytes() <= (int64_t)(8 * n + 65536) &&
                      std::fabs(norm - (12 * 1.0 + 12 * 0.7)) <= 1e-12 && std::fabs(e_dev - e_host) <= 1e-10 * scale;
    std::printf("TFIM ring L = 12, block m = 0 (%lld states, %lld device bytes): device operator %.15f, mv_mul over the CSR %.15f: %s\n",
                (long long)n, (long long)H0.device_bytes(), e_dev, e_host, good ? "ok" : "WRONG");
    ok = ok && good;

    bool refused = false;
    try {
      ll::PauliMomentumFullOperator<double> Hb(L, 0, tfim(L, 1.0, 0.7, false));
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
