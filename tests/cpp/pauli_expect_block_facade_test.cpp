// PauliMomentumFullOperator<T>::expectation and PauliSymmetricOperator<T>::expectation (include/lambda_lanczos_hip/common.hpp) in the
// reference's idiom: the momentum block m = 1 of a ring of 8 spins (complex double; c as a std::vector and as a device pointer:
// the same bits), every value against the definition on the full space,
//   coef * sum_s Re[conj(Psi(s ^ x)) i^nY (-1)^popcount(s & z) Psi(s)],   Psi(T^l r) = e^(-2 pi i m l / L) R_r^(-1/2) c_r,
// evaluated here in long double, within (2 (D S + 8) + 32) eps |coef| sum |Psi(s ^ x)||Psi(s)| for the S <= L strings of the
// group average and the D coefficients; the identity returns ||c||^2; under spin inversion Z_0 is answered +0.0 without a sweep;
// a mask bit above the ring is refused.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

static int popc(uint64_t v) { return __builtin_popcountll(v); }

int main() {
  try {
    bool ok = true;
    typedef std::complex<double> Z;
    typedef std::complex<long double> ZL;
    const int L = 8, m = 1;
    const uint32_t full = (1u << L) - 1;
    const long double pi = 3.141592653589793238462643383279502884L;
    auto rotl = [&](uint32_t v) { return ((v << 1) | (v >> (L - 1))) & full; };
    // the block's basis: the smallest member of every orbit whose length R satisfies m R = 0 (mod L), ascending
    std::vector<uint32_t> reps;
    std::vector<uint32_t> rep_of(full + 1);
    std::vector<int> shift_of(full + 1), period_of(full + 1);
    for (uint32_t s = 0; s <= full; ++s) {
      uint32_t cur = s, best = s;
      int first = 0, period = L;
      for (int j = 1; j < L; ++j) {
        cur = rotl(cur);
        if (cur == s && period == L) period = j;
        if (cur < best) best = cur, first = j;
      }
      rep_of[s] = best;                                  // T^first s = best: s = T^(period - first) best
      shift_of[s] = (period - first) % period;           // (the first minimiser comes before the orbit repeats)
      period_of[s] = period;
      if (best == s && (m * period) % L == 0) reps.push_back(s);
    }
    const size_t D = reps.size();
    std::vector<Z> c(D);
    for (size_t i = 0; i < D; ++i) c[i] = Z(std::sin(0.37 * (double)(i + 1)) + 0.2, std::cos(1.3 * (double)i) - 0.1);
    std::vector<ZL> psi(full + 1, ZL(0, 0));
    for (uint32_t s = 0; s <= full; ++s) {
      if ((m * period_of[s]) % L != 0) continue;
      const size_t i = (size_t)(std::lower_bound(reps.begin(), reps.end(), rep_of[s]) - reps.begin());
      const long double a = -2.0L * pi * (long double)(m * shift_of[s]) / (long double)L;
      psi[s] = ZL(std::cos(a), std::sin(a)) / std::sqrt((long double)period_of[s]) * ZL(c[i]);
    }
    std::vector<ll::PauliTerm> obs = {{0, 0, 1.0}};
    for (int r = 1; r <= L / 2; ++r) {
      const uint64_t q = 1u | ((uint64_t)1 << r);
      obs.push_back({0, q, 1.0});              // Z_0 Z_r
      obs.push_back({q, 0, 0.25});             // X_0 X_r
      obs.push_back({q, q, -0.75});            // Y_0 Y_r
      obs.push_back({q, (uint64_t)1 << r, 1.5});  // X_0 Y_r
    }
    obs.push_back({1, 0, 0.5});
    obs.push_back({1, 1, -1.25});
    obs.push_back({0, 1, 2.0});
    obs.push_back({5, 2, -2.0});               // X_0 Z_1 X_2
    for (int r = 0; r < 24; ++r) obs.push_back({(uint64_t)((r * 37 + 5) & full), (uint64_t)((r * 91 + 3) & full), 0.1 * (r - 10)});

    std::vector<ll::PauliTerm> ring;
    for (int j = 0; j < L; ++j) {
      ring.push_back({0, ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L)), -1.0});
      ring.push_back({(uint64_t)1 << j, 0, -0.7});
    }
    ll::PauliMomentumFullOperator<Z> H(L, m, ring);
    ok = ok && (size_t)H.size() == D;
    int64_t sweeps = -1;
    const std::vector<double> host = H.expectation(obs, c, &sweeps);
    static const ZL iy[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
    double worst = 0;
    for (size_t j = 0; j < obs.size() && host.size() == obs.size(); ++j) {
      const ll::PauliTerm& t = obs[j];
      const ZL ph = iy[popc(t.x_mask & t.z_mask) & 3];
      long double sum = 0, mag = 0;
      for (uint32_t s = 0; s <= full; ++s) {
        const ZL a = psi[s ^ (uint32_t)t.x_mask], b = psi[s];
        const long double sign = (popc(s & t.z_mask) & 1) ? -1.0L : 1.0L;
        sum += (std::conj(a) * ph * sign * b).real();
        mag += (std::fabs(a.real()) + std::fabs(a.imag())) * (std::fabs(b.real()) + std::fabs(b.imag()));
      }
      const double want = (double)((long double)t.coef * sum);
      const double bound = (2.0 * ((double)D * L + 8.0) + 32.0) * 2.220446049250313e-16 * std::fabs(t.coef) * (double)mag +
                           2.220446049250313e-16 * std::fabs(want);
      const double err = std::fabs(host[j] - want);
      if (!(err <= bound)) {
        std::printf("observable %zu (x %llx z %llx): %.17g, definition %.17g, bound %.3g\n", j, (unsigned long long)t.x_mask,
                    (unsigned long long)t.z_mask, host[j], want, bound);
        ok = false;
      }
      if (bound > 0) worst = std::fmax(worst, err / bound);
    }
    std::printf("momentum block (8, m = 1), D = %zu, %zu observables, worst error / bound %.3g\n", D, obs.size(), worst);
    double nn = 0;
    for (const Z& v : c) nn += std::norm(v);
    const bool idn = host.size() == obs.size() && std::fabs(host[0] - nn) <= 1e-13 * nn && sweeps == (int64_t)((obs.size() + 31) / 32);
    std::printf("identity %.15f against ||c||^2 %.15f, %lld sweeps: %s\n", host.empty() ? 0.0 : host[0], nn, (long long)sweeps, idn ? "ok" : "WRONG");
    ok = ok && idn;
    void* dc = nullptr;
    ll::check(ll_malloc(H.context().get(), D * sizeof(Z), &dc));
    ll::check(ll_memcpy_h2d(H.context().get(), dc, c.data(), D * sizeof(Z)));
    const std::vector<double> dev = H.expectation(obs, (const Z*)dc);
    ll::check(ll_free(H.context().get(), dc));
    const bool same = dev.size() == host.size() && std::memcmp(dev.data(), host.data(), dev.size() * sizeof(double)) == 0;
    std::printf("c on the device: %s\n", same ? "the same bits" : "DIFFERENT bits");
    ok = ok && same;
    bool refused = false;
    try {
      (void)H.expectation({{(uint64_t)1 << L, 0, 1.0}}, c);
    } catch (const ll::Error& e) {
      refused = std::strstr(e.what(), "at or above n_sites") != nullptr;
      std::printf("a mask bit above the ring is refused: %s\n", e.what());
    }
    ok = ok && refused;
    {  // under spin inversion every image of Z_0 cancels: +0.0, no sweep; X_0 needs one
      ll::PauliSymmetricOperator<double> S(L, 0, ring, 1, 1);
      std::vector<double> cs((size_t)S.size());
      for (size_t i = 0; i < cs.size(); ++i) cs[i] = std::sin(0.61 * (double)(i + 1)) + 0.3;
      int64_t none = -1, one = -1;
      const std::vector<double> z0 = S.expectation({{0, 1, 1.0}, {0, 7, -3.0}}, cs, &none);
      const std::vector<double> x0 = S.expectation({{1, 0, 1.0}, {0, 1, 1.0}}, cs, &one);
      const bool zeros = none == 0 && z0[0] == 0.0 && !std::signbit(z0[0]) && z0[1] == 0.0 && !std::signbit(z0[1]) && one == 1 &&
                         x0[0] != 0.0 && x0[1] == 0.0;
      std::printf("spin inversion: <Z_0> = %g without a sweep, <X_0> = %.15f in %lld: %s\n", z0[0], x0[0], (long long)one, zeros ? "ok" : "WRONG");
      ok = ok && zeros;
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
