// Spectral functions from the coefficients of a Lanczos run, on the host: what a caller computes from the (alpha, beta) that
// LambdaLanczos<T>::run_two_pass (ll_lanczos_two_pass_* with eps = 0 and max_iteration = M) returns for the start vector
// phi = O psi of PauliMomentumOperator<T>::transfer.  Standard headers only, no device.
//
//   continued_fraction(alpha, beta, z, norm2) = norm2 / (z - alpha[0] - beta[0]^2 / (z - alpha[1] - beta[1]^2 / (... - alpha[m - 1])))
//                                             = norm2 e_1^T (z - T)^-1 e_1,    T the m x m tridiagonal,
// evaluated bottom-up, m divisions.  Indexing as ll_lanczos_two_pass_* writes it: m = alpha.size(), beta[k] couples alpha[k] and
// alpha[k + 1]; only beta[0 .. m - 2] enter, so beta may hold m - 1 entries or m (the last one of a run is the norm of the
// residual that ended it, not an element of T, and is not read).
//   spectral_function(alpha, beta, omega, eta, e0, norm2) = -Im G(omega + e0 + i eta) / pi: Lorentz-broadened by eta > 0, on a
// real frequency omega measured from e0 (the ground-state energy); it integrates to norm2 over omega.
#pragma once

#include <complex>
#include <stdexcept>
#include <vector>

namespace lambda_lanczos_hip {

inline std::complex<double> continued_fraction(const std::vector<double>& alpha, const std::vector<double>& beta, std::complex<double> z,
                                               double norm2 = 1.0) {
  const size_t m = alpha.size();
  if (m < 1 || beta.size() + 1 < m) throw std::invalid_argument("continued_fraction: at least one alpha and alpha.size() - 1 betas");
  std::complex<double> d = z - alpha[m - 1];
  for (size_t k = m - 1; k-- > 0;) d = z - alpha[k] - (beta[k] * beta[k]) / d;
  return norm2 / d;
}

inline double spectral_function(const std::vector<double>& alpha, const std::vector<double>& beta, double omega, double eta,
                                double e0 = 0.0, double norm2 = 1.0) {
  return -continued_fraction(alpha, beta, std::complex<double>(omega + e0, eta), norm2).imag() / 3.14159265358979323846;
}
inline std::vector<double> spectral_function(const std::vector<double>& alpha, const std::vector<double>& beta,
                                             const std::vector<double>& omega, double eta, double e0 = 0.0, double norm2 = 1.0) {
  std::vector<double> out(omega.size());
  for (size_t i = 0; i < omega.size(); ++i) out[i] = spectral_function(alpha, beta, omega[i], eta, e0, norm2);
  return out;
}

}  // namespace lambda_lanczos_hip
