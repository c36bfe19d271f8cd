// lambda-lanczos_amd/csrc/raw_basis.hpp on the records that blocks of EIGHT leave (LoopState::enqueue_block_f64): raw vectors from
// k0 = 2 on, in blocks of 4, 4, 4, 4, 8, 8, 8, and a stop, a flush or a hand-over at every position of the last block of eight.  What
// the loop fetches for a stop at `count` vectors is rows k0 .. count - 1 and nothing behind (LoopState::fetch_block_rows): the
// record here is allocated to exactly that size, so under the address sanitizer a read of a row behind the stop is an error.
// Construction as in raw_basis_test.cpp: the orthonormal u_l are unit vectors, a vector is its own coefficient list.
// Built (plain and sanitized) and run by tests/test_raw_basis_block8_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "raw_basis.hpp"

using namespace ll;
typedef std::complex<double> Z;
typedef std::vector<Z> Vec;

static std::mt19937_64 rng(20261021);
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

static Z coef(int R, const double* g, int64_t j) { return R == 2 ? Z(g[2 * j], g[2 * j + 1]) : Z(g[j], 0.0); }

// a_j = rho_j u_j + sum_{l<j} C_j[l] u_l for k0 <= j < count (rho_j in [0.5, 2], |C| <= 1e-9: what the gate admits), a_j = u_j in front
template <typename T> void stop_at(int64_t k0, int64_t count) {
  constexpr int R = scalar_traits<T>::reals;
  BlockRows br;
  br.R = R;
  br.k0 = k0;
  br.end = count;
  br.rows.resize(block_row_at(R, count) - block_row_at(R, k0) + 1);
  br.rho.resize((size_t)(count - k0));
  std::vector<Vec> a((size_t)count, Vec((size_t)count, Z(0.0, 0.0)));
  for (int64_t j = 0; j < count; ++j) {
    if (j < k0) {
      a[j][j] = 1.0;
      continue;
    }
    a[j][j] = br.rho[(size_t)(j - k0)] = uni(0.5, 2.0);
    double* row = br.rows.data() + (block_row_at(R, j) - block_row_at(R, k0));
    for (int64_t l = 0; l < j; ++l) {
      const Z c(uni(-1e-9, 1e-9), R == 2 ? uni(-1e-9, 1e-9) : 0.0);
      a[j][l] = c;
      row[(size_t)R * l] = c.real();
      if (R == 2) row[2 * l + 1] = c.imag();
    }
  }
  // the Ritz GEMV's coefficients over the raw vectors: sum_j c'_j a_j = sum_j q_j u_j, first order in C (error <= count^2 |C|^2 / rho^2
  // ~ 1e-14 at 42 vectors, plus rounding)
  std::vector<T> q((size_t)count), c;
  for (auto& v : q) from_z(Z(uni(-1, 1), R == 2 ? uni(-1, 1) : 0.0), &v);
  c = q;
  block_coeff_over_raw(br, count, 1, c.data());
  double err = 0.0;
  for (int64_t i = 0; i < count; ++i) {
    Z x(0.0, 0.0);
    for (int64_t j = 0; j < count; ++j) x += to_z(c[j]) * a[j][i];
    err = std::max(err, std::abs(x - to_z(q[i])));
  }
  REQUIRE(err <= 1e-13, "stop at %d (k0 %d): transformed coefficients off by %.3e", (int)count, (int)k0, err);
  // the in-place flush of a_k0 .. a_{count-1}, descending, as the device performs it
  BlockRows fl = br;
  block_rows_over_raw(fl, count - 1);
  std::vector<Vec> v = a;
  for (int64_t j = count - 1; j >= k0; --j) {
    for (int64_t l = 0; l < j; ++l)
      for (int64_t i = 0; i < count; ++i) v[j][i] -= coef(R, fl.row(j), l) * v[l][i];
    for (int64_t i = 0; i < count; ++i) v[j][i] *= 1.0 / fl.rho[(size_t)(j - k0)];
  }
  err = 0.0;
  for (int64_t j = 0; j < count; ++j)
    for (int64_t i = 0; i < count; ++i) err = std::max(err, std::abs(v[j][i] - (i == j ? Z(1.0, 0.0) : Z(0.0, 0.0))));
  REQUIRE(err <= 1e-13, "flush to %d (k0 %d): completed vectors off by %.3e", (int)(count - 1), (int)k0, err);
}

int main() {
  // vectors 0, 1 complete; blocks of four end at 6, 10, 14, 18; blocks of eight at 26, 34, 42: a stop at every row of the last one,
  // and the same with the form entered late (k0 = 19: re-entry after a repair)
  for (const int64_t k0 : {2, 19})
    for (int64_t count = 35; count <= 42; ++count) {
      stop_at<double>(k0, count);
      stop_at<zc>(k0, count);
    }
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
