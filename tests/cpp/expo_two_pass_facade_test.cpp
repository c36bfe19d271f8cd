// Exponentiator<T>::run_two_pass (include/lambda_lanczos_hip/exponentiator.hpp) in the reference's idiom: the transverse-field
// Ising ring of 10 spins (J = 1, h = 1.5) evolved by a = -0.5i in complex double, and by the real a = -0.3 with max_iteration = 30
// in double, without a stored Krylov basis, against the facade's own run() on the same operator and input:
// max|delta| <= 1e-10 ||input||; the device-buffer overload in place; and full_orthogonalize reaching the caller as an Error.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include <lambda_lanczos_hip/exponentiator.hpp>

namespace ll = lambda_lanczos;

static std::vector<ll::PauliTerm> tfim_ring(int L, double J, double h) {
  std::vector<ll::PauliTerm> terms;
  for (int j = 0; j < L; ++j) {
    const uint64_t m = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
    terms.push_back({0, m, -J});                 // -J Z_j Z_{j+1}
    terms.push_back({(uint64_t)1 << j, 0, -h});  // -h X_j
  }
  return terms;
}

template <typename T> static T start_value(size_t i);
template <> double start_value<double>(size_t i) { return std::sin(0.37 * (double)(i + 1)); }
template <> std::complex<double> start_value<std::complex<double>>(size_t i) {
  return std::complex<double>(std::sin(0.37 * (double)(i + 1)), std::cos(0.53 * (double)(i + 1)));
}

template <typename T> static bool check_type(const char* name, T a, size_t max_iteration) {
  const int L = 10;
  const size_t n = (size_t)1 << L;
  ll::PauliOperator<T> H(L, tfim_ring(L, 1.0, 1.5));
  std::vector<T> input(n), out_ref, out_two, out_dev(n);
  double in_norm = 0.0;
  for (size_t i = 0; i < n; ++i) {
    input[i] = start_value<T>(i);
    in_norm += std::norm(std::complex<double>(input[i]));
  }
  in_norm = std::sqrt(in_norm);
  ll::Exponentiator<T> ex(H, n);
  if (max_iteration > 0) ex.max_iteration = max_iteration;
  const size_t it_ref = ex.run(a, input, out_ref);
  const size_t it_two = ex.run_two_pass(a, input, out_two);
  // the device-buffer overload, in place
  void* d_psi = nullptr;
  ll::check(ll_malloc(H.context().get(), n * sizeof(T), &d_psi));
  ll::check(ll_memcpy_h2d(H.context().get(), d_psi, input.data(), n * sizeof(T)));
  const size_t it_dev = ex.run_two_pass_device(a, static_cast<const T*>(d_psi), static_cast<T*>(d_psi));
  ll::check(ll_memcpy_d2h(H.context().get(), out_dev.data(), d_psi, n * sizeof(T)));
  ll::check(ll_free(H.context().get(), d_psi));
  double worst = 0.0;
  bool same = out_two.size() == n;
  for (size_t i = 0; i < n && same; ++i) {
    worst = std::fmax(worst, std::abs(std::complex<double>(out_two[i]) - std::complex<double>(out_ref[i])));
    same = out_dev[i] == out_two[i];
  }
  bool good = out_two.size() == n && same && it_dev == it_two;
  good = good && worst <= 1e-10 * in_norm;
  good = good && (it_two > it_ref ? it_two - it_ref : it_ref - it_two) <= 1;
  std::printf("%s: %zu / %zu iterations (two-pass / stored basis); max|delta| / |input| %.2e; device buffer in place %s: %s\n", name,
              it_two, it_ref, worst / in_norm, same ? "same values" : "DIFFERENT", good ? "ok" : "WRONG");
  bool refused = false;
  try {
    ll::Exponentiator<T> full(H, n);
    full.full_orthogonalize = true;  // no basis to orthogonalise against: reaches the caller as an Error
    std::vector<T> out;
    full.run_two_pass(a, input, out);
  } catch (const ll::Error&) {
    refused = true;
  }
  std::printf("%s: full_orthogonalize refused: %s\n", name, refused ? "ok" : "WRONG");
  return good && refused;
}

int main() {
  try {
    bool ok = check_type<std::complex<double>>("complex double", std::complex<double>(0.0, -0.5), 0);
    ok = check_type<double>("double", -0.3, 30) && ok;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
