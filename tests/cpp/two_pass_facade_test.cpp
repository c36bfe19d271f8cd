// LambdaLanczos<T>::run_two_pass (include/lambda_lanczos_hip/lambda_lanczos.hpp) in the reference's idiom: the ground state of the
// transverse-field Ising ring of 10 spins (J = 1, h = 1.5) without a stored Krylov basis, in double and complex double, against
// the stored-basis run() on the same operator and start vector (one tracked root, like the two-pass solver); the overload
// without the vector; and invalid parameters reaching the caller as an Error.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

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

template <typename T> static bool check_type(const char* name) {
  const int L = 10;
  const size_t n = (size_t)1 << L;
  ll::PauliOperator<T> H(L, tfim_ring(L, 1.0, 1.5));
  std::vector<T> start(n);
  for (size_t i = 0; i < n; ++i) start[i] = start_value<T>(i);
  ll::LambdaLanczos<T> engine(H, n, false, 1);
  engine.init_vector = [&](std::vector<T>& v) { v = start; };
  engine.eigenvalue_offset = -H.inf_norm();
  engine.num_eigs_per_iteration = 1;  // run() then tracks one root, as run_two_pass does: the same stop rule
  double e_ref, e_two, e_only;
  std::vector<T> v_ref, v_two;
  engine.run(e_ref, v_ref);
  const size_t it_ref = engine.getIterationCounts()[0];
  const size_t it_two = engine.run_two_pass(e_two, v_two);
  const double residual = engine.getLastResidual();
  const ll_run_stats st = engine.getLastStats();
  const size_t it_only = engine.run_two_pass(e_only);
  std::complex<double> ov(0.0, 0.0);
  double nrm = 0.0;
  for (size_t i = 0; i < n && v_two.size() == n; ++i) {
    ov += std::conj(std::complex<double>(v_ref[i])) * std::complex<double>(v_two[i]);
    nrm += std::norm(std::complex<double>(v_two[i]));
  }
  bool good = v_two.size() == n;
  good = good && std::fabs(e_two - e_ref) <= 1e-10 * std::fmax(1.0, std::fabs(e_ref));
  good = good && e_only == e_two && it_only == it_two && engine.getLastStats().workspace_vectors == 3;
  good = good && 1.0 - std::abs(ov) <= 1e-8 && std::fabs(std::sqrt(nrm) - 1.0) <= 4 * 2.3e-16;
  good = good && residual <= 1e-5 * H.inf_norm();
  good = good && st.workspace_vectors == 4 && st.replay_mismatches == 0;
  good = good && (it_two > it_ref ? it_two - it_ref : it_ref - it_two) <= 3;
  std::printf("%s: E0 two-pass %.15f, stored basis %.15f; %zu / %zu iterations; 1 - overlap %.2e; residual %.2e; %lld vectors, %lld "
              "mismatches: %s\n", name, e_two, e_ref, it_two, it_ref, 1.0 - std::abs(ov), residual, (long long)st.workspace_vectors,
              (long long)st.replay_mismatches, good ? "ok" : "WRONG");
  bool refused = false;
  try {
    ll::LambdaLanczos<T> two(H, n, false, 1);
    two.max_iteration = 0;  // an invalid parameter reaches the caller as an Error, like run()'s
    double e;
    two.run_two_pass(e);
  } catch (const ll::Error&) {
    refused = true;
  }
  std::printf("%s: invalid parameters refused: %s\n", name, refused ? "ok" : "WRONG");
  return good && refused;
}

int main() {
  try {
    bool ok = check_type<double>("double");
    ok = check_type<std::complex<double>>("complex double") && ok;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
