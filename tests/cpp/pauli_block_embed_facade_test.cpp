// expand, project and reduced_density_matrix of the block operators (include/lambda_lanczos_hip/common.hpp) in the reference's
// idiom, on a ring of 12 spins: the momentum block (n_down = 6, m = 4; complex double) into its S_z sector and into the full
// space, and the symmetric block (m = 0, parity +1, inversion +1; double) into the full space.  The embedding is formed here from
// its definition — the state T^l r carries e^(-2 pi i m l / L) / sqrt(R) c_r; under G = {T^j P^rho Z^zeta} the state g r carries
// 1 / sqrt(R) c_r for the trivial character — so that
//   expand          the real character is the product c_r * (1 / sqrt(R)) bit for bit; complex phases within 16 eps |val c|,
//   project         of a vector that is not in the block: B^H psi from the definition within (2 (|G| + 8) + 8) eps sum |val psi|,
//   the round trip  project(expand(c)) = c within the two bounds,
//   the entropy     von_neumann_entropy(block.reduced_density_matrix(sites, c, target)) is that of the target's own
//                   reduced_density_matrix on the expanded state (the same kernel on the same bits), its trace ||c||^2,
// with a std::vector and a device pointer giving the same bits, and a sector target refused for a full-space block.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

int main() {
  try {
    bool ok = true;
    typedef std::complex<double> Z;
    const double eps = 2.220446049250313e-16;
    const int L = 12;
    const uint32_t full = (1u << L) - 1;
    auto rotl = [&](uint32_t v) { return ((v << 1) | (v >> (L - 1))) & full; };
    auto rev = [&](uint32_t v) {
      uint32_t r = 0;
      for (int i = 0; i < L; ++i)
        if ((v >> i) & 1u) r |= 1u << (L - 1 - i);
      return r;
    };
    std::vector<ll::PauliTerm> heis, tfim;
    for (int j = 0; j < L; ++j) {
      const uint64_t q = ((uint64_t)1 << j) | ((uint64_t)1 << ((j + 1) % L));
      heis.push_back({q, 0, 0.25});
      heis.push_back({q, q, 0.25});
      heis.push_back({0, q, 0.2});
      tfim.push_back({0, q, -1.0});
      tfim.push_back({(uint64_t)1 << j, 0, -0.7});
    }

    {  // ---- the momentum block (12, 6, m = 4) into the sector and into the full space
      const int nd = 6, m = 4;
      std::vector<uint32_t> states;
      for (uint32_t s = 0; s <= full; ++s)
        if (__builtin_popcount(s) == nd) states.push_back(s);
      std::vector<uint32_t> reps;
      std::vector<int> rep_i(full + 1, -1), shift_of(full + 1, 0), period_of(full + 1, 0);
      for (uint32_t s : states) {
        uint32_t cur = s, best = s;
        int first = 0, period = L;
        for (int j = 1; j < L; ++j) {
          cur = rotl(cur);
          if (cur == s && period == L) period = j;
          if (cur < best) best = cur, first = j;
        }
        period_of[s] = period;
        shift_of[s] = (period - first) % period;
        if ((m * period) % L != 0) continue;
        if (best == s) reps.push_back(s);
        rep_i[s] = (int)best;  // the representative for now; its number below
      }
      for (uint32_t s : states)
        if (rep_i[s] >= 0) rep_i[s] = (int)(std::lower_bound(reps.begin(), reps.end(), (uint32_t)rep_i[s]) - reps.begin());
      const size_t D = reps.size(), N = states.size();
      ll::PauliMomentumOperator<Z> H(L, nd, m, heis);
      ll::PauliSectorOperator<Z> S(L, nd, heis);
      ll::PauliOperator<Z> F(L, heis);
      ok = ok && (size_t)H.size() == D && (size_t)S.size() == N;
      std::vector<Z> c(D);
      for (size_t i = 0; i < D; ++i) c[i] = Z(std::sin(0.37 * (double)(i + 1)) + 0.2, std::cos(1.3 * (double)i) - 0.1);
      std::vector<Z> val(N, Z(0, 0));
      for (size_t t = 0; t < N; ++t) {
        const uint32_t s = states[t];
        if (rep_i[s] < 0) continue;
        const double a = -2.0 * M_PI * (double)((m * shift_of[s]) % L) / (double)L;
        val[t] = Z(std::cos(a), std::sin(a)) / std::sqrt((double)period_of[s]);
      }
      const std::vector<Z> psi = H.expand(S, c);
      double worst = 0;
      bool exp_ok = psi.size() == N;
      for (size_t t = 0; t < N && exp_ok; ++t) {
        const uint32_t s = states[t];
        if (rep_i[s] < 0) {
          exp_ok = exp_ok && psi[t] == Z(0, 0) && !std::signbit(psi[t].real()) && !std::signbit(psi[t].imag());
          continue;
        }
        const Z want = val[t] * c[(size_t)rep_i[s]];
        const double bound = 17.0 * eps * std::abs(want);  // 16 eps |val c| and the storage rounding
        const double err = std::abs(psi[t] - want);
        exp_ok = exp_ok && err <= bound;
        worst = std::fmax(worst, err / bound);
      }
      std::printf("momentum block (12, 6, m = 4), D = %zu into the sector of %zu states: expand worst error / bound %.3g: %s\n", D, N,
                  worst, exp_ok ? "ok" : "WRONG");
      ok = ok && exp_ok;
      // into the full space: the same values at the states' own indices, +0.0 outside the sector
      const std::vector<Z> big = H.expand(F, c);
      bool big_ok = big.size() == (size_t)full + 1;
      size_t t = 0;
      for (uint32_t s = 0; s <= full && big_ok; ++s) {
        if (t < N && states[t] == s) big_ok = std::memcmp(&big[s], &psi[t++], sizeof(Z)) == 0;
        else big_ok = big[s] == Z(0, 0) && !std::signbit(big[s].real()) && !std::signbit(big[s].imag());
      }
      std::printf("into the full space: %s\n", big_ok ? "the sector's bits, +0.0 outside" : "WRONG");
      ok = ok && big_ok;
      // project a vector that is not in the block
      std::vector<Z> rnd(N);
      for (size_t i = 0; i < N; ++i) rnd[i] = Z(std::cos(0.77 * (double)i) + 0.1, std::sin(0.21 * (double)(i + 3)));
      std::vector<Z> want(D, Z(0, 0));
      std::vector<double> mag(D, 0.0);
      for (size_t i = 0; i < N; ++i) {
        const int a = rep_i[states[i]];
        if (a < 0) continue;
        want[(size_t)a] += std::conj(val[i]) * rnd[i];
        mag[(size_t)a] += std::abs(val[i]) * std::abs(rnd[i]);
      }
      const std::vector<Z> got = H.project(S, rnd);
      bool prj_ok = got.size() == D;
      worst = 0;
      for (size_t a = 0; a < D && prj_ok; ++a) {
        const double bound = (2.0 * (L + 8) + 8.0) * eps * mag[a] + eps * std::abs(want[a]);
        prj_ok = prj_ok && std::abs(got[a] - want[a]) <= bound;
        worst = std::fmax(worst, std::abs(got[a] - want[a]) / bound);
      }
      std::printf("project of a vector outside the block: worst error / bound %.3g: %s\n", worst, prj_ok ? "ok" : "WRONG");
      ok = ok && prj_ok;
      const std::vector<Z> back = H.project(S, psi);
      bool rt_ok = back.size() == D;
      for (size_t a = 0; a < D && rt_ok; ++a) rt_ok = std::abs(back[a] - c[a]) <= (2.0 * (L + 8) + 8.0 + 18.0) * eps * std::abs(c[a]);
      std::printf("round trip project(expand(c)) = c: %s\n", rt_ok ? "ok" : "WRONG");
      ok = ok && rt_ok;
      // device pointers: the same bits
      void *dc = nullptr, *dpsi = nullptr;
      ll::check(ll_malloc(H.context().get(), D * sizeof(Z), &dc));
      ll::check(ll_malloc(H.context().get(), N * sizeof(Z), &dpsi));
      ll::check(ll_memcpy_h2d(H.context().get(), dc, c.data(), D * sizeof(Z)));
      H.expand(S, (const Z*)dc, (Z*)dpsi);
      std::vector<Z> from_dev(N);
      ll::check(ll_memcpy_d2h(H.context().get(), from_dev.data(), dpsi, N * sizeof(Z)));
      const bool same = std::memcmp(from_dev.data(), psi.data(), N * sizeof(Z)) == 0;
      std::printf("c and psi on the device: %s\n", same ? "the same bits" : "DIFFERENT bits");
      ok = ok && same;
      // the entropy: the block's call against the target's own on the expanded state
      double nn = 0;
      for (const Z& v : c) nn += std::norm(v);
      const std::vector<int> sites = {0, 1, 2, 3, 4, 5};
      const std::vector<Z> rho_b = H.reduced_density_matrix(sites, c, S), rho_t = S.reduced_density_matrix(sites, (const Z*)dpsi);
      const std::vector<Z> rho_d = H.reduced_density_matrix(sites, (const Z*)dc, S);
      ll::check(ll_free(H.context().get(), dc));
      ll::check(ll_free(H.context().get(), dpsi));
      double tr = 0;
      for (int a = 0; a < 64; ++a) tr += rho_b[(size_t)a * 65].real();
      const double sb = ll::von_neumann_entropy(rho_b, 64), st = ll::von_neumann_entropy(rho_t, 64);
      const bool ent = rho_b.size() == 4096 && std::memcmp(rho_b.data(), rho_t.data(), 4096 * sizeof(Z)) == 0 &&
                       std::memcmp(rho_b.data(), rho_d.data(), 4096 * sizeof(Z)) == 0 && sb == st && sb > 0.0 &&
                       sb <= 6.0 * std::log(2.0) && std::fabs(tr - nn) <= 1e-12 * nn;
      std::printf("entropy of six sites of the block state %.15f (trace %.15f, ||c||^2 %.15f): %s\n", sb, tr, nn, ent ? "ok" : "WRONG");
      ok = ok && ent;
    }

    {  // ---- the symmetric block (12, m = 0, parity +1, inversion +1) into the full space: the trivial character
      const int G = 4 * L;
      std::vector<uint32_t> rep_of(full + 1);
      std::vector<int> orbit_of(full + 1);
      for (uint32_t s = 0; s <= full; ++s) {
        uint32_t best = s;
        int stab = 0;
        for (int rho = 0; rho < 2; ++rho)
          for (int zeta = 0; zeta < 2; ++zeta) {
            uint32_t cur = rho ? rev(s) : s;
            if (zeta) cur ^= full;
            for (int j = 0; j < L; ++j) {
              if (cur < best) best = cur;
              if (cur == s) ++stab;
              cur = rotl(cur);
            }
          }
        rep_of[s] = best;
        orbit_of[s] = G / stab;
      }
      std::vector<uint32_t> reps;
      for (uint32_t s = 0; s <= full; ++s)
        if (rep_of[s] == s) reps.push_back(s);  // the trivial character admits every orbit
      const size_t D = reps.size(), N = (size_t)full + 1;
      ll::PauliSymmetricOperator<double> H(L, 0, tfim, 1, 1);
      ll::PauliOperator<double> F(L, tfim);
      ok = ok && (size_t)H.size() == D;
      std::vector<double> c(D);
      for (size_t i = 0; i < D; ++i) c[i] = std::sin(0.61 * (double)(i + 1)) + 0.3;
      const std::vector<double> psi = H.expand(F, c);
      bool exp_ok = psi.size() == N;
      for (uint32_t s = 0; s <= full && exp_ok; ++s) {
        const size_t a = (size_t)(std::lower_bound(reps.begin(), reps.end(), rep_of[s]) - reps.begin());
        exp_ok = psi[s] == c[a] * (1.0 / std::sqrt((double)orbit_of[s]));
      }
      std::printf("symmetric block (12, 0, +, +), D = %zu: expand is c * (1 / sqrt(R)) bit for bit: %s\n", D, exp_ok ? "ok" : "WRONG");
      ok = ok && exp_ok;
      std::vector<double> ints(N);
      for (size_t i = 0; i < N; ++i) ints[i] = (double)((int)((i * 2654435761u) % 15u) - 7);
      const std::vector<double> got = H.project(F, ints);
      std::vector<double> S(D, 0.0);
      for (uint32_t s = 0; s <= full; ++s) {
        const size_t a = (size_t)(std::lower_bound(reps.begin(), reps.end(), rep_of[s]) - reps.begin());
        S[a] += (double)(G / orbit_of[s]) * ints[s];  // every state of the orbit is reached |G| / R times: an exact integer
      }
      bool prj_ok = got.size() == D;
      for (size_t a = 0; a < D && prj_ok; ++a) prj_ok = got[a] == S[a] * (std::sqrt((double)orbit_of[reps[a]]) / (double)G);
      std::printf("project of an integer vector is S * (sqrt(R) / |G|) bit for bit: %s\n", prj_ok ? "ok" : "WRONG");
      ok = ok && prj_ok;
      const std::vector<double> back = H.project(F, psi);
      bool rt_ok = back.size() == D;
      for (size_t a = 0; a < D && rt_ok; ++a) rt_ok = std::fabs(back[a] - c[a]) <= (2.0 * (G + 8) + 8.0 + 18.0) * eps * std::fabs(c[a]);
      std::printf("round trip: %s\n", rt_ok ? "ok" : "WRONG");
      ok = ok && rt_ok;
      const double s3 = ll::von_neumann_entropy(H.reduced_density_matrix({0, 1, 2}, c, F), 8);
      const double s3t = ll::von_neumann_entropy(F.reduced_density_matrix({0, 1, 2}, psi), 8);
      std::printf("entropy of three sites %.15f, of the expanded state %.15f\n", s3, s3t);
      ok = ok && s3 == s3t && s3 > 0.0 && s3 <= 3.0 * std::log(2.0);
      bool refused = false;
      try {
        ll::PauliSectorOperator<double> S6(L, 6, heis);
        (void)H.expand(S6, c);
      } catch (const ll::Error& e) {
        refused = std::strstr(e.what(), "a full-space block does not fit an S_z-sector target") != nullptr;
        std::printf("a sector target is refused for a full-space block: %s\n", e.what());
      }
      ok = ok && refused;
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
