// The von Neumann entropy of a small density matrix, on the host: what a caller computes from the reduced density matrix that
// PauliOperator<T>::reduced_density_matrix returns.  Standard headers only, no device.
//
//   von_neumann_entropy(rho, dim) = -sum_i lambda_i ln lambda_i,   lambda = the eigenvalues of rho / tr rho,
// rho a Hermitian dim x dim matrix, row-major, dim <= 64; eigenvalues <= 0 contribute 0.  The eigenvalues come from the cyclic
// Jacobi method on the Hermitian matrix (complex rotations; sweeps until the off-diagonal part is below eps ||rho||_F), whose
// eigenvalue errors are a few eps ||rho||_F.  Only the upper triangle is read.
#pragma once

#include <cmath>
#include <complex>
#include <stdexcept>
#include <vector>

namespace lambda_lanczos_hip {

// the eigenvalues of the Hermitian matrix a (dim x dim, row-major; the upper triangle is read), in no particular order
inline std::vector<double> hermitian_eigenvalues_jacobi(const std::vector<std::complex<double>>& a_in, int dim) {
  typedef std::complex<double> Z;
  if (dim < 1 || dim > 64 || a_in.size() != (size_t)dim * (size_t)dim)
    throw std::invalid_argument("hermitian_eigenvalues_jacobi: a dim x dim matrix with 1 <= dim <= 64");
  const size_t n = (size_t)dim;
  std::vector<Z> a(a_in);
  double norm2 = 0.0;
  for (size_t p = 0; p < n; ++p) {
    a[p * n + p] = Z(a[p * n + p].real(), 0.0);
    norm2 += a[p * n + p].real() * a[p * n + p].real();
    for (size_t q = p + 1; q < n; ++q) {
      a[q * n + p] = std::conj(a[p * n + q]);
      norm2 += 2.0 * std::norm(a[p * n + q]);
    }
  }
  const double stop = 1.1102230246251565e-16 * std::sqrt(norm2);
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off2 = 0.0;
    for (size_t p = 0; p < n; ++p)
      for (size_t q = p + 1; q < n; ++q) off2 += 2.0 * std::norm(a[p * n + q]);
    if (std::sqrt(off2) <= stop) break;
    for (size_t p = 0; p < n; ++p) {
      for (size_t q = p + 1; q < n; ++q) {
        const double g = std::abs(a[p * n + q]);
        if (g == 0.0) continue;
        // a_pq = g e^{i phi}: the rotation J with columns (c, -s e^{-i phi}) and (s e^{i phi}, c) annihilates it
        const Z phase = a[p * n + q] / g;
        const double app = a[p * n + p].real(), aqq = a[q * n + q].real();
        const double theta = (aqq - app) / (2.0 * g);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (size_t k = 0; k < n; ++k) {  // columns p and q: A <- A J
          const Z akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - s * std::conj(phase) * akq;
          a[k * n + q] = s * phase * akp + c * akq;
        }
        for (size_t k = 0; k < n; ++k) {  // rows p and q: A <- J^H A
          const Z apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - s * phase * aqk;
          a[q * n + k] = s * std::conj(phase) * apk + c * aqk;
        }
        a[p * n + q] = a[q * n + p] = Z(0.0, 0.0);
        a[p * n + p] = Z(a[p * n + p].real(), 0.0);
        a[q * n + q] = Z(a[q * n + q].real(), 0.0);
      }
    }
  }
  std::vector<double> lam(n);
  for (size_t p = 0; p < n; ++p) lam[p] = a[p * n + p].real();
  return lam;
}

inline double von_neumann_entropy(const std::vector<std::complex<double>>& rho, int dim) {
  const std::vector<double> lam = hermitian_eigenvalues_jacobi(rho, dim);
  double trace = 0.0;
  for (double v : lam) trace += v;
  if (!(trace > 0.0)) throw std::invalid_argument("von_neumann_entropy: the trace of rho is not positive");
  double s = 0.0;
  for (double v : lam) {
    const double x = v / trace;
    if (x > 0.0) s -= x * std::log(x);
  }
  return s + 0.0;
}

}  // namespace lambda_lanczos_hip
