// PauliOperator<T> (include/lambda_lanczos_hip/common.hpp) in the reference's idiom: the Heisenberg ring of 4 spins (ground state
// -2 J), the ring of 12 spins against the same matrix stored as CsrMatrix<double>, and one Exponentiator step exp(-i H dt) that
// keeps the norm.
#include <cmath>
#include <complex>
#include <cstdio>
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

// the same Hamiltonian as a stored matrix, by the definition of the terms
static void expand(int L, const std::vector<ll::PauliTerm>& terms, std::vector<int64_t>& rp, std::vector<int32_t>& ci,
                   std::vector<double>& va) {
  const int64_t n = (int64_t)1 << L;
  rp.assign(1, 0);
  for (int64_t s = 0; s < n; ++s) {
    for (const auto& t : terms) {
      const uint64_t src = (uint64_t)s ^ t.x_mask;
      const int ny = __builtin_popcountll(t.x_mask & t.z_mask);
      const double sign = ((__builtin_popcountll(src & t.z_mask) + ny / 2) & 1) ? -1.0 : 1.0;
      ci.push_back((int32_t)src);
      va.push_back(sign * t.coef);
    }
    rp.push_back((int64_t)ci.size());
  }
}

int main() {
  try {
    bool ok = true;
    {
      const double J = 1.5;
      ll::PauliOperator<double> H(4, heisenberg_ring(4, J));
      ll::LambdaLanczos<double> engine(H, (size_t)16, false, 1);
      engine.eigenvalue_offset = -H.inf_norm();
      double value;
      std::vector<double> vec;
      engine.run(value, vec);
      const bool good = std::fabs(value + 2.0 * J) <= 1e-10 * 2.0 * J && vec.size() == 16;
      std::printf("ring L = 4: E0 %.15f (exact %.15f), %lld device bytes: %s\n", value, -2.0 * J, (long long)H.device_bytes(),
                  good ? "ok" : "WRONG");
      ok = ok && good;
    }
    {
      const int L = 12;
      const size_t n = (size_t)1 << L;
      const auto terms = heisenberg_ring(L, 1.0);
      std::vector<int64_t> rp;
      std::vector<int32_t> ci;
      std::vector<double> va;
      expand(L, terms, rp, ci, va);
      ll::PauliOperator<double> H(L, terms);
      ll::CsrMatrix<double> A(rp, ci, va);
      double e_free, e_csr;
      std::vector<double> v_free, v_csr;
      std::vector<double> start(n);
      for (size_t i = 0; i < n; ++i) start[i] = std::sin(0.37 * (double)(i + 1));
      for (int which = 0; which < 2; ++which) {
        ll::LambdaLanczos<double> engine = which ? ll::LambdaLanczos<double>(A, n, false, 1) : ll::LambdaLanczos<double>(H, n, false, 1);
        engine.eigenvalue_offset = -H.inf_norm();
        engine.init_vector = [&](std::vector<double>& v) { v = start; };
        engine.run(which ? e_csr : e_free, which ? v_csr : v_free);
      }
      const bool good = std::fabs(e_free - e_csr) <= 1e-10 * std::fmax(1.0, std::fabs(e_csr - H.inf_norm()));
      std::printf("ring L = 12: matrix-free %.15f, CsrMatrix %.15f: %s\n", e_free, e_csr, good ? "ok" : "WRONG");
      ok = ok && good;

      typedef std::complex<double> Z;
      auto zterms = terms;
      zterms.push_back({0x3, 0x1, 0.3});  // X1 Y0: a complex Hermitian matrix
      ll::PauliOperator<Z> Hz(L, zterms);
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
    }
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
