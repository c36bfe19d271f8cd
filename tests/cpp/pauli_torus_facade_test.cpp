// PauliTorusOperator<T> (include/lambda_lanczos_hip/common.hpp) in the reference's idiom: on the 4 x 4 Heisenberg torus
// LambdaLanczos<double> finds the ground energy -11.228483208428853 in the block (mx, my) = (0, 0) of the sector n_down = 8 (822 of
// the 12 870 states), and the same run with PauliSectorOperator<double> gives the same energy — the ground state of the torus is
// translation invariant; the block (2, 2) lies above it; the staggered correlation <Z_0 Z_r> changes sign with the sublattice;
// the image stays O(D); an open cylinder and a real type at a complex momentum are refused.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include <lambda_lanczos_hip/lambda_lanczos.hpp>

namespace ll = lambda_lanczos;

// three strings of J / 4 per bond; y_periodic = false leaves the bonds (x, Ly - 1) - (x, 0) out: an open cylinder
static std::vector<ll::PauliTerm> heisenberg_torus(int lx, int ly, bool y_periodic) {
  std::vector<ll::PauliTerm> terms;
  auto bond = [&](int a, int b) {
    const uint64_t m = ((uint64_t)1 << a) | ((uint64_t)1 << b);
    terms.push_back({m, 0, 0.25});
    terms.push_back({m, m, 0.25});
    terms.push_back({0, m, 0.25});
  };
  for (int y = 0; y < ly; ++y)
    for (int x = 0; x < lx; ++x) {
      bond(x + lx * y, (x + 1) % lx + lx * y);
      if (y_periodic || y + 1 < ly) bond(x + lx * y, x + lx * ((y + 1) % ly));
    }
  return terms;
}

template <typename Engine> static double ground(Engine& engine, size_t n, double offset, std::vector<double>& v) {
  std::vector<double> start(n);
  for (size_t i = 0; i < n; ++i) start[i] = std::sin(0.37 * (double)(i + 1)) + 1.5;
  engine.eigenvalue_offset = offset;
  engine.init_vector = [&](std::vector<double>& x) { x = start; };
  double e = 0;
  engine.run(e, v);
  return e;
}

int main() {
  try {
    bool ok = true;
    const double e_exact = -11.228483208428853;
    const auto terms = heisenberg_torus(4, 4, true);
    ll::PauliTorusOperator<double> Hb(4, 4, 0, 0, terms, 8), Hpi(4, 4, 2, 2, terms, 8);
    ll::PauliSectorOperator<double> Hs(16, 8, terms);
    const size_t n = (size_t)Hb.size(), n_pi = (size_t)Hpi.size(), n_sector = (size_t)Hs.size();
    const double norm = Hb.inf_norm();
    ll::LambdaLanczos<double> in_block(Hb, n, false, 1), in_pi(Hpi, n_pi, false, 1), in_sector(Hs, n_sector, false, 1);
    std::vector<double> v, v_pi, v_sector;
    const double e_block = ground(in_block, n, -norm, v), e_pi = ground(in_pi, n_pi, -norm, v_pi),
                 e_sector = ground(in_sector, n_sector, -norm, v_sector);
    const double scale = std::fmax(1.0, std::fabs(e_exact - norm));
    const bool good = n == 822 && n_pi == 816 && n_sector == 12870 && Hb.device_bytes() <= (int64_t)(8 * n + 192 * 1024) &&
                      std::fabs(norm - 96 * 0.25) <= 1e-12 && std::fabs(e_block - e_exact) <= 1e-10 * scale &&
                      std::fabs(e_block - e_sector) <= 1e-10 * scale && e_pi > e_exact + 0.1;
    std::printf("Heisenberg torus 4 x 4, block (0, 0) at n_down = 8 (%lld states, %lld device bytes): %.15f, the sector's %lld states "
                "%.15f, block (2, 2) (%lld states) %.15f: %s\n",
                (long long)n, (long long)Hb.device_bytes(), e_block, (long long)n_sector, e_sector, (long long)n_pi, e_pi,
                good ? "ok" : "WRONG");
    ok = ok && good;

    // <Z_0 Z_r> on the block's ground state: negative on the other sublattice, positive on the own one
    const std::vector<ll::PauliTerm> zz = {{0, 1 | (1 << 1), 1.0}, {0, 1 | (1 << 5), 1.0}, {0, 1 | (1 << 10), 1.0}, {0, 0, 1.0}};
    const std::vector<double> c = Hb.expectation(zz, v);
    const bool staggered = c[0] < -0.1 * c[3] && c[1] > 0.05 * c[3] && c[2] > 0.05 * c[3] && std::fabs(c[3] - 1.0) <= 1e-10;
    std::printf("<Z_0 Z_(1,0)> = %.6f, <Z_0 Z_(1,1)> = %.6f, <Z_0 Z_(2,2)> = %.6f, <1> = %.12f: %s\n", c[0], c[1], c[2], c[3],
                staggered ? "ok" : "WRONG");
    ok = ok && staggered;

    ll::PauliTorusOperator<std::complex<double>> Hz(4, 4, 1, 0, terms, 8);   // a complex block: every type takes it
    ok = ok && Hz.size() == 800;

    bool cylinder_refused = false, real_refused = false;
    try {
      ll::PauliTorusOperator<double> Hc(4, 4, 0, 0, heisenberg_torus(4, 4, false), 8);
    } catch (const ll::Error& e) {
      cylinder_refused = std::strstr(e.what(), "does not commute with T_y") != nullptr && std::strstr(e.what(), "z_mask") != nullptr;
      std::printf("an open cylinder is refused: %s\n", e.what());
    }
    try {
      ll::PauliTorusOperator<double> Hr(4, 4, 1, 0, terms, 8);
    } catch (const ll::Error& e) {
      real_refused = std::strstr(e.what(), "real storage type") != nullptr;
      std::printf("a real type at mx = 1 is refused: %s\n", e.what());
    }
    ok = ok && cylinder_refused && real_refused;
    std::printf("%s\n", ok ? "PASSED" : "FAILED");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::printf("EXCEPTION: %s\n", e.what());
    return 2;
  }
}
