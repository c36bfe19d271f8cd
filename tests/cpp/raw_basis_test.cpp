// The host algebra of the raw-basis forms (lambda-lanczos_amd/csrc/raw_basis.hpp, scalar_types.hpp) on a construction where the
// orthonormal u_l are the unit vectors of R^m / C^m: a vector is its own coefficient list, so no tolerance hides in an
// orthogonalisation.  Built (plain, and with the address and undefined-behaviour sanitizers) and run by tests/test_raw_basis_host.py.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

#include "raw_basis.hpp"

using namespace ll;
typedef std::complex<double> Z;
typedef std::vector<Z> Vec;

static std::mt19937_64 rng(20260607);
static double uni(double lo, double hi) { return lo + (hi - lo) * ((double)(rng() >> 11) * 0x1p-53); }
static long long checks = 0, fails = 0;
#define REQUIRE(cond, ...)                          \
  do {                                              \
    ++checks;                                       \
    if (!(cond) && fails++ < 20) {                  \
      std::printf("FAIL line %d: ", __LINE__);      \
      std::printf(__VA_ARGS__);                     \
      std::printf("\n");                            \
    }                                               \
  } while (0)

template <typename T> constexpr bool is_cplx = scalar_traits<T>::is_complex;
template <typename T> Z draw(double mag) {  // |z| <= mag; real for a real T
  if (is_cplx<T>) return Z(uni(-mag, mag), uni(-mag, mag)) * std::sqrt(0.5);
  return Z(uni(-mag, mag), 0.0);
}
template <typename T> Z draw_modulus(double mag) {  // |z| == mag
  const int k = (int)(rng() & 3);
  if (is_cplx<T> && (k & 2)) return Z(0.0, (k & 1) ? mag : -mag);
  return Z((k & 1) ? mag : -mag, 0.0);
}
static double max_abs_diff(const Vec& a, const Vec& b) {
  double e = 0.0;
  for (size_t i = 0; i < a.size(); ++i) e = std::max(e, std::abs(a[i] - b[i]));
  return e;
}
static Z coef(int R, const double* g, int64_t j) { return R == 2 ? Z(g[2 * j], g[2 * j + 1]) : Z(g[j], 0.0); }
static void put(int R, double* g, int64_t j, Z v) {
  if (R == 2) g[2 * j] = v.real(), g[2 * j + 1] = v.imag();
  else g[j] = v.real();
}

// ---------------------------------------------------------------- conversions, all four storage types
template <typename T> void test_conversions() {
  typedef typename scalar_traits<T>::real Real;
  for (int i = 0; i < 2000; ++i) {
    const Z v(std::ldexp(uni(-1, 1), (int)(rng() % 60) - 30), std::ldexp(uni(-1, 1), (int)(rng() % 60) - 30));
    T t, t2;
    from_z(v, &t);
    Real re, im = 0;
    if constexpr (is_cplx<T>) re = t.re, im = t.im;
    else re = t;
    REQUIRE(re == (Real)v.real(), "real part is not the cast of %a", v.real());
    if (is_cplx<T>) REQUIRE(im == (Real)v.imag(), "imaginary part is not the cast of %a", v.imag());
    const Z back = to_z(t);
    REQUIRE(back.real() == (double)re && back.imag() == (double)im, "to_z does not widen (%a, %a)", (double)re, (double)im);
    from_z(back, &t2);
    REQUIRE(std::memcmp(&t, &t2, sizeof(T)) == 0, "T -> Z -> T changes bits");
  }
}

// ---------------------------------------------------------------- block form
// a_j = rho_j u_j + sum_{l<j} C_j[l] u_l for j >= k0 (rho_j in [0.5, 2], |C| <= cmag, or == cmag), a_j = u_j in front of k0
template <typename T> struct Record {
  BlockRows br;
  std::vector<Vec> a;
};
template <typename T> Record<T> make_record(int64_t m, int64_t k0, double cmag, bool exact_modulus) {
  Record<T> rec;
  BlockRows& br = rec.br;
  br.R = scalar_traits<T>::reals;
  br.k0 = k0;
  br.end = m;
  if (m > k0) {
    br.rows.resize(block_row_at(br.R, m) - block_row_at(br.R, k0) + 1);
    br.rho.resize((size_t)(m - k0));
  }
  rec.a.assign((size_t)m, Vec((size_t)m, Z(0.0, 0.0)));
  for (int64_t j = 0; j < m; ++j) {
    if (j < k0) {
      rec.a[j][j] = 1.0;
      continue;
    }
    rec.a[j][j] = br.rho[(size_t)(j - k0)] = uni(0.5, 2.0);
    double* row = br.rows.data() + (block_row_at(br.R, j) - block_row_at(br.R, k0));
    for (int64_t l = 0; l < j; ++l) put(br.R, row, l, rec.a[j][l] = exact_modulus ? draw_modulus<T>(cmag) : draw<T>(cmag));
  }
  return rec;
}
static Vec combine(const std::vector<Vec>& a, const Vec& c) {  // sum_j c_j a_j
  Vec x(c.size(), Z(0.0, 0.0));
  for (size_t j = 0; j < c.size(); ++j)
    for (size_t i = 0; i < c.size(); ++i) x[i] += c[j] * a[j][i];
  return x;
}
// sum_j c'_j a_j = sum_j q_j u_j to 1e-13 with |C| <= 1e-9, |q| <= 1: the formula is first order in C, the neglected terms are
// <= m^2 |C|^2 / rho^2 = m^2 4e-18 ~ 1e-14 at m = 48, rounding a few m eps ~ 2e-14.  Teeth: with |C| = 1e-5 (and |q| = 1) neither the
// untouched q nor q / rho (a transform that ignores C) comes within 1e-6 of that bound.
template <typename T> void test_block_transform(int64_t m, int64_t k0, int64_t nw) {
  for (const bool teeth : {false, true}) {
    const Record<T> rec = make_record<T>(m, k0, teeth ? 1e-5 : 1e-9, teeth);
    std::vector<T> q((size_t)(nw * m));
    for (auto& v : q) from_z(teeth ? draw_modulus<T>(1.0) : draw<T>(1.0), &v);
    std::vector<T> c = q;
    block_coeff_over_raw(rec.br, m, nw, c.data());
    for (int64_t w = 0; w < nw; ++w) {
      Vec q0((size_t)m), cw((size_t)m), by_rho((size_t)m);
      for (int64_t j = 0; j < m; ++j) {
        q0[j] = to_z(q[w * m + j]);
        cw[j] = to_z(c[w * m + j]);
        by_rho[j] = j >= k0 ? q0[j] / rec.br.rho[(size_t)(j - k0)] : q0[j];
      }
      const double err = max_abs_diff(combine(rec.a, cw), q0);
      if (!teeth) REQUIRE(err <= 1e-13, "block transform m %d k0 %d nw %d: error %.3e", (int)m, (int)k0, (int)nw, err);
      if (!teeth && k0 == m) REQUIRE(std::memcmp(c.data(), q.data(), q.size() * sizeof(T)) == 0, "an empty record changed q");
      if (teeth && k0 < m) {
        const double untouched = max_abs_diff(combine(rec.a, q0), q0);
        REQUIRE(untouched > 1e-13 + 1e-6, "teeth m %d k0 %d: the untransformed q is within %.3e", (int)m, (int)k0, untouched);
        if (m >= 2) {
          const double rho_only = max_abs_diff(combine(rec.a, by_rho), q0);
          REQUIRE(rho_only > 1e-13 + 1e-6, "teeth m %d k0 %d: q / rho is within %.3e", (int)m, (int)k0, rho_only);
        }
      }
    }
  }
}
// The rows scaled for the flush, then the descending in-place update as the device performs it: a_j -= sum_{l<j} row_j[l] a_l over the
// vectors as they are at that moment (raw below j), times 1 / rho_j.  The completed vectors are the u_j to 1e-13 (same reasoning as
// above); the rows behind `last`, and the entries against the complete vectors in front of k0, keep their bits.
template <typename T> void test_flush(int64_t m, int64_t k0, int64_t last) {
  const Record<T> rec = make_record<T>(m, k0, 1e-9, false);
  BlockRows br = rec.br;
  block_rows_over_raw(br, last);
  const int R = br.R;
  for (int64_t j = k0; j < m; ++j) {
    const size_t at = block_row_at(R, j) - block_row_at(R, k0);
    const size_t same_to = j > last ? (size_t)R * j : (size_t)R * std::min(k0, j);
    REQUIRE(std::memcmp(br.rows.data() + at, rec.br.rows.data() + at, same_to * sizeof(double)) == 0,
            "flush m %d k0 %d last %d: row %d changed where it must not", (int)m, (int)k0, (int)last, (int)j);
  }
  std::vector<Vec> v = rec.a;
  for (int64_t j = last; j >= k0; --j) {
    for (int64_t l = 0; l < j; ++l)
      for (int64_t i = 0; i < m; ++i) v[j][i] -= coef(R, br.row(j), l) * v[l][i];
    const double inv = 1.0 / br.rho[(size_t)(j - k0)];
    for (int64_t i = 0; i < m; ++i) v[j][i] *= inv;
  }
  for (int64_t j = 0; j < m; ++j) {
    Vec want = rec.a[j];  // untouched ...
    if (j >= k0 && j <= last) want.assign((size_t)m, Z(0.0, 0.0)), want[j] = 1.0;  // ... or completed: u_j
    const double err = max_abs_diff(v[j], want);
    REQUIRE(err <= 1e-13, "flush m %d k0 %d last %d: vector %d off by %.3e", (int)m, (int)k0, (int)last, (int)j, err);
  }
}

// ---------------------------------------------------------------- pair tail (exact algebra)
// S = [L locked vectors, u_0 .. u_{Pt-1}] = e_0 .. e_{K-1}, u_P = e_K, u_{P+1} = e_{K+1};
// r1 = rho1 u_P + S g1, r2 = rho2 u_{P+1} + S g2 + gam u_P
template <typename T> void test_pair_tail(int64_t L, int64_t Pt, int nvec, int64_t nw) {
  const int R = scalar_traits<T>::reals;
  const int64_t K = L + Pt, m = Pt + nvec, dim = K + 2;
  std::vector<double> g1h((size_t)(R * K + 1)), g2h((size_t)(R * (K + 1) + 1));
  const double rho1 = uni(0.5, 2.0), rho2 = uni(0.5, 2.0);
  Vec r1((size_t)dim, Z(0.0, 0.0)), r2((size_t)dim, Z(0.0, 0.0));
  for (int64_t j = 0; j < K; ++j) put(R, g1h.data(), j, r1[j] = draw<T>(0.3));
  for (int64_t j = 0; j <= K; ++j) put(R, g2h.data(), j, r2[j] = draw<T>(0.3));  // (entry K: gam)
  r1[K] = rho1;
  r2[K + 1] = rho2;
  std::vector<T> s((size_t)(nw * m));
  for (auto& v : s) from_z(draw<T>(1.0), &v);
  const std::vector<T> c = pair_coeff_over_raw<T>(R, g1h, g2h, rho1, rho2, L, Pt, nvec, m, nw, s);
  REQUIRE((int64_t)c.size() == nw * (K + nvec), "pair tail: %zu coefficients", c.size());
  if ((int64_t)c.size() != nw * (K + nvec)) return;
  for (int64_t w = 0; w < nw; ++w) {
    const T* cw = c.data() + w * (K + nvec);
    Vec got((size_t)dim, Z(0.0, 0.0)), want((size_t)dim, Z(0.0, 0.0));
    for (int64_t j = 0; j < K; ++j) got[j] = to_z(cw[j]);
    for (int64_t i = 0; i < dim; ++i) {
      if (nvec >= 1) got[i] += to_z(cw[K]) * r1[i];
      if (nvec == 2) got[i] += to_z(cw[K + 1]) * r2[i];
    }
    for (int64_t k = 0; k < m; ++k) want[L + k] = to_z(s[w * m + k]);
    const double err = max_abs_diff(got, want), bound = 64.0 * (double)(K + 2) * DBL_EPSILON;
    REQUIRE(err <= bound, "pair tail L %d Pt %d nvec %d nw %d: error %.3e > %.3e", (int)L, (int)Pt, nvec, (int)nw, err, bound);
    if (nvec == 0) {
      const T zero{};
      for (int64_t j = 0; j < L; ++j) REQUIRE(std::memcmp(cw + j, &zero, sizeof(T)) == 0, "pair tail: a locked column is not 0");
      REQUIRE(Pt == 0 || std::memcmp(cw + L, s.data() + w * m, (size_t)Pt * sizeof(T)) == 0, "pair tail: nvec 0 changed bits");
    }
  }
}

template <typename T> void test_type() {
  for (const int64_t m : {1, 2, 3, 7, 48})
    for (const int64_t k0 : std::set<int64_t>{0, std::min<int64_t>(1, m), m - 1, m}) {
      for (const int64_t nw : {1, 3}) test_block_transform<T>(m, k0, nw);
      for (const int64_t last : std::set<int64_t>{m - 1, std::min(m - 1, k0 + (m - 1 - k0) / 2), k0 - 1}) test_flush<T>(m, k0, last);
    }
  for (const int64_t L : {0, 2})
    for (const int64_t Pt : {0, 1, 5})
      for (const int nvec : {0, 1, 2})
        for (const int64_t nw : {1, 3}) test_pair_tail<T>(L, Pt, nvec, nw);
}

int main() {
  test_conversions<double>();
  test_conversions<zc>();
  test_conversions<float>();
  test_conversions<cf>();
  test_type<double>();
  test_type<zc>();
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
