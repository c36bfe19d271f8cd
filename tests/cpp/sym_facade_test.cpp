// SymmetricCsrMatrix<T> (include/lambda_lanczos_hip/common.hpp): the 5-point Laplacian 40x40 given as its upper triangle,
// one eigen-solve through the facade against the analytic smallest eigenvalue; the operator must keep the one-triangle image.
#include <cmath>
#include <cstdio>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

int main() {
  try {
    const int64_t N = 40, n = N * N;
    std::vector<int64_t> rp{0};
    std::vector<int32_t> ci;
    std::vector<double> va;
    for (int64_t r = 0; r < n; ++r) {  // row r: the diagonal, then its right and lower neighbours (col >= row)
      const int64_t x = r % N, y = r / N;
      const int64_t nb[3] = {r, x + 1 < N ? r + 1 : -1, y + 1 < N ? r + N : -1};
      for (int t = 0; t < 3; ++t)
        if (nb[t] >= 0) {
          ci.push_back((int32_t)nb[t]);
          va.push_back(t == 0 ? 4.0 : -1.0);
        }
      rp.push_back((int64_t)ci.size());
    }
    ll::SymmetricCsrMatrix<double> A(rp, ci, va, ll::Triangle::Upper);
    ll::LambdaLanczos<double> engine(A, (size_t)n, false, 1);
    engine.eigenvalue_offset = -8.0;
    double value;
    std::vector<double> vec;
    engine.run(value, vec);
    const double want = 4.0 - 4.0 * std::cos(M_PI / (N + 1));
    const bool ok = A.selected_spmv() == LL_SPMV_SYM && std::fabs(value - want) <= 8.0 * engine.eps * 10 && vec.size() == (size_t)n;
    std::printf("kernel %d, lambda_min %.15f (analytic %.15f), %lld device bytes: %s\n", A.selected_spmv(), value, want,
                (long long)A.device_bytes(), ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
