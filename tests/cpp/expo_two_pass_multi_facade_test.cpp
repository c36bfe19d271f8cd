// Exponentiator<T>::run_two_pass with SEVERAL times (include/lambda_lanczos_hip/exponentiator.hpp; ll_expo_two_pass_multi) in the
// reference's idiom: the transverse-field Ising ring of 10 spins (J = 1, h = 1.5) in complex double, evolved to three times from
// one Krylov space.  Every output and iteration count must equal, byte for byte, what the single-time run_two_pass gives for that
// time alone; the device-buffer overload (one output in place) gives the same bytes again.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/exponentiator.hpp>

namespace ll = lambda_lanczos;
typedef std::complex<double> Z;

static std::vector<ll::PauliTerm> tfim_ring(int L, double J, double h) {
  std::vector<ll::PauliTerm> terms;
  for (int j = 0; j < L; ++j) {
    const uint64_t m = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
    terms.push_back({0, m, -J});                 // -J Z_j Z_{j+1}
    terms.push_back({(uint64_t)1 << j, 0, -h});  // -h X_j
  }
  return terms;
}

int main() {
  try {
    const int L = 10;
    const size_t n = (size_t)1 << L;
    ll::PauliOperator<Z> H(L, tfim_ring(L, 1.0, 1.5));
    std::vector<Z> input(n);
    for (size_t i = 0; i < n; ++i) input[i] = Z(std::sin(0.37 * (double)(i + 1)), std::cos(0.53 * (double)(i + 1)));
    const std::vector<Z> times = {Z(0.0, -0.5), Z(0.0, -1.5), Z(0.0, -0.1)};
    ll::Exponentiator<Z> ex(H, n);

    std::vector<std::vector<Z>> outs;
    const std::vector<size_t> counts = ex.run_two_pass(times, input, outs);
    bool ok = counts.size() == times.size() && outs.size() == times.size();

    // the device-buffer overload: output 1 in place
    std::vector<void*> d(times.size(), nullptr);
    std::vector<Z*> d_out;
    for (size_t j = 0; j < times.size(); ++j) {
      ll::check(ll_malloc(H.context().get(), n * sizeof(Z), &d[j]));
      d_out.push_back(static_cast<Z*>(d[j]));
    }
    ll::check(ll_memcpy_h2d(H.context().get(), d[1], input.data(), n * sizeof(Z)));
    const std::vector<size_t> counts_dev = ex.run_two_pass_device(times, static_cast<const Z*>(d[1]), d_out.data());

    for (size_t j = 0; j < times.size() && ok; ++j) {
      std::vector<Z> single, from_dev(n);
      const size_t it = ex.run_two_pass(times[j], input, single);
      ll::check(ll_memcpy_d2h(H.context().get(), from_dev.data(), d[j], n * sizeof(Z)));
      const bool same = outs[j].size() == n && std::memcmp(outs[j].data(), single.data(), n * sizeof(Z)) == 0;
      const bool same_dev = std::memcmp(from_dev.data(), single.data(), n * sizeof(Z)) == 0;
      std::printf("a = %+.1fi: %zu iterations (multi) / %zu (device buffers) / %zu (single); host %s, device %s\n", times[j].imag(),
                  counts[j], counts_dev[j], it, same ? "same bytes" : "DIFFERENT", same_dev ? "same bytes" : "DIFFERENT");
      ok = same && same_dev && counts[j] == it && counts_dev[j] == it;
    }
    for (void* p : d) ll::check(ll_free(H.context().get(), p));
    ok = ok && counts[0] != counts[1] && counts[1] != counts[2];  // (the times end at different iterations: accumulators retire early)

    bool refused = false;
    try {
      std::vector<Z> many(LL_EXPO_MULTI_MAX + 1, Z(0.0, -0.1));
      ex.run_two_pass(many, input, outs);
    } catch (const ll::Error&) {
      refused = true;
    }
    std::printf("seventeen times refused: %s\n", refused ? "ok" : "WRONG");
    ok = ok && refused;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
