// Host algebra of the raw-basis forms (LoopState, lanczos_loop.hpp): coefficients over orthonormal u_j rewritten as coefficients over the RAW
// vectors the device holds.  Pure functions on host arrays, standard headers only (tests/cpp/raw_basis_test.cpp).  R = scalar_traits<T>::reals.
#pragma once

#include "scalar_types.hpp"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ll {

// Block form: row j of the packed triangle holds C_j[l] = <u_l, a_j>, l < j, and starts here
inline size_t block_row_at(int R, int64_t j) { return (size_t)R * (size_t)j * (size_t)(j > 0 ? j - 1 : 0) / 2; }
struct BlockRows {  // the record of the raw vectors a_k0 .. a_{end-1} on the host
  int R = 1;
  int64_t k0 = 0, end = 0;
  std::vector<double> rows;  // rows k0 .. end - 1 of the packed triangle
  std::vector<double> rho;   // rho_k0 .. rho_{end-1}
  const double* row(int64_t j) const { return rows.data() + (block_row_at(R, j) - block_row_at(R, k0)); }
};
// C_j[l] / rho_l in place, rows k0 .. last: the coefficients of block_flush's multi-axpys over the raw a_l (rho_l = 1 in front of k0)
inline void block_rows_over_raw(BlockRows& br, int64_t last) {
  for (int64_t j = br.k0; j <= last; ++j) {
    double* row = br.rows.data() + (block_row_at(br.R, j) - block_row_at(br.R, br.k0));
    for (int64_t l = br.k0; l < j; ++l)
      for (int q = 0; q < br.R; ++q) row[(size_t)br.R * l + q] /= br.rho[(size_t)(l - br.k0)];
  }
}
// coeff (nw rows of m) in place: sum_j q_j u_j = sum_j c'_j a_j with c'_j = (q_j - sum_{k>j} C_k[j] q_k / rho_k) / rho_j, first order in C
template <typename T> void block_coeff_over_raw(const BlockRows& br, int64_t m, int64_t nw, T* coeff) {
  typedef std::complex<double> Z;
  const int64_t end = std::min<int64_t>(br.end, m);
  std::vector<Z> cs((size_t)m);
  for (int64_t w = 0; w < nw; ++w) {
    T* q = coeff + (size_t)w * m;
    for (int64_t j = 0; j < m; ++j) cs[(size_t)j] = to_z(q[j]);
    for (int64_t kk = br.k0; kk < end; ++kk) {
      const Z f = to_z(q[kk]) / br.rho[(size_t)(kk - br.k0)];
      const double* row = br.row(kk);
      for (int64_t l = 0; l < kk; ++l) cs[(size_t)l] -= (br.R == 2 ? Z(row[2 * l], row[2 * l + 1]) : Z(row[l], 0.0)) * f;
    }
    for (int64_t j = 0; j < m; ++j) from_z(j >= br.k0 && j < end ? cs[(size_t)j] / br.rho[(size_t)(j - br.k0)] : cs[(size_t)j], q + j);
  }
}

// Pair form, end of a pass: S = [L locked vectors, u_0 .. u_{Pt-1}] is complete and nvec raw vectors are pending,
//   u_P = (r1 - S g1) / rho1,  u_{P+1} = (r2 - S g2 - gam u_P) / rho2   (g2h: g2, then gam)
// so sum_k s_k u_k (coeff: nw rows of m) is a combination of [S, r1, r2]: returns its nw rows of L + Pt + nvec coefficients.
template <typename T>
std::vector<T> pair_coeff_over_raw(int R, const std::vector<double>& g1h, const std::vector<double>& g2h, double rho1, double rho2,
                                   int64_t L, int64_t Pt, int nvec, int64_t m, int64_t nw, const std::vector<T>& coeff) {
  typedef std::complex<double> Z;
  auto gz = [&](const std::vector<double>& g, int64_t j) { return R == 2 ? Z(g[(size_t)2 * j], g[(size_t)2 * j + 1]) : Z(g[(size_t)j], 0.0); };
  const int64_t K = L + Pt, mm = K + nvec;
  std::vector<T> c2((size_t)nw * mm);
  std::vector<Z> cs((size_t)K);
  for (int64_t w = 0; w < nw; ++w) {
    const T* sw = coeff.data() + (size_t)w * m;
    for (int64_t j = 0; j < K; ++j) cs[(size_t)j] = j < L ? Z(0.0, 0.0) : to_z(sw[j - L]);
    Z on_r1(0.0, 0.0), on_r2(0.0, 0.0);
    if (nvec >= 1) {
      Z a = to_z(sw[Pt]);                                                // coefficient of u_P
      if (nvec == 2) {
        on_r2 = to_z(sw[Pt + 1]) / rho2;                                 // ... of u_{P+1}
        for (int64_t j = 0; j < K; ++j) cs[(size_t)j] -= on_r2 * gz(g2h, j);
        a -= on_r2 * gz(g2h, K);                                         // gam = <u_P, r2>
      }
      on_r1 = a / rho1;
      for (int64_t j = 0; j < K; ++j) cs[(size_t)j] -= on_r1 * gz(g1h, j);
    }
    T* out = c2.data() + (size_t)w * mm;
    for (int64_t j = 0; j < K; ++j) from_z(cs[(size_t)j], out + j);
    if (nvec >= 1) from_z(on_r1, out + K);
    if (nvec == 2) from_z(on_r2, out + K + 1);
  }
  return c2;
}
}  // namespace ll
