// The host-side arithmetic of the torus group (lambda-lanczos_amd/csrc/pauli_torus_plan.hpp) by brute force on every shape of up
// to 12 sites, and on 4 x 4 and 5 x 4 against recorded dimensions:
//   the translations   T_x and T_y move site (x, y) to (x + 1 mod Lx, y) and (x, y + 1 mod Ly), bit by bit; they commute, T_x^Lx =
//                      T_y^Ly = 1, and stay inside the n bits on 30 sites
//   the codes          inverse_code names the inverse element; phase_num is additive (a character) and, with Ly = 1 or Lx = 1,
//                      the ring's (m j) mod L
//   admission          pauli_torus_admit against an independent walk over the whole orbit: the smallest member, the stabiliser's
//                      size, the character on the stabiliser — including representatives that a ring's rule (m R = 0 mod n) would
//                      admit although the character excludes them
//   the slices         concatenated in ascending top bits they are the basis, ascending, for the full space and every sector;
//                      the dimensions of a shape sum to 2^n (to C(n, n_down)) over the blocks; recorded dimensions are met
// Built (plain, and with the address and undefined-behaviour sanitizers) and run by tests/test_pauli_torus_plan_host.py.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "pauli_torus_plan.hpp"

using namespace ll;

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

// independent of the header: site by site
static uint32_t shift_sites(uint32_t v, int lx, int ly, int dx, int dy) {
  uint32_t r = 0;
  for (int y = 0; y < ly; ++y)
    for (int x = 0; x < lx; ++x)
      if ((v >> (x + lx * y)) & 1u) r |= (uint32_t)1 << ((x + dx) % lx + lx * ((y + dy) % ly));
  return r;
}

static void test_translations(int lx, int ly) {
  const PauliTorus g(lx, ly);
  const int n = lx * ly;
  const uint32_t full = (uint32_t)(((uint64_t)1 << n) - 1);
  bool moves = true, commute = true, closed = true;
  for (uint32_t v = 0; v <= full; ++v) {
    moves = moves && g.tx(v) == shift_sites(v, lx, ly, 1, 0) && g.ty(v) == shift_sites(v, lx, ly, 0, 1);
    commute = commute && g.tx(g.ty(v)) == g.ty(g.tx(v));
    closed = closed && g.move(v, lx - 1, 0) == shift_sites(v, lx, ly, lx - 1, 0) && g.tx(g.move(v, lx - 1, 0)) == v &&
             g.ty(g.move(v, 0, ly - 1)) == v;
    if (v == full) break;
  }
  REQUIRE(moves, "%d x %d: T_x, T_y against the site-by-site shift", lx, ly);
  REQUIRE(commute, "%d x %d: T_x T_y = T_y T_x", lx, ly);
  REQUIRE(closed, "%d x %d: T_x^Lx = T_y^Ly = 1", lx, ly);
  bool inverse = true, additive = true, ring = true;
  for (int c = 0; c < n; ++c) {
    const int ic = g.inverse_code(c);
    inverse = inverse && ic >= 0 && ic < n && g.move(g.move(5u & full, c % lx, c / lx), ic % lx, ic / lx) == (5u & full) &&
              g.move(g.move(full >> 1, c % lx, c / lx), ic % lx, ic / lx) == (full >> 1);
    for (int mx = 0; mx < lx; ++mx)
      for (int my = 0; my < ly; ++my) {
        for (int d = 0; d < n; ++d) {
          const int cd = g.code((c % lx + d % lx) % lx, (c / lx + d / lx) % ly);
          additive = additive && g.phase_num(mx, my, cd) == (g.phase_num(mx, my, c) + g.phase_num(mx, my, d)) % n;
        }
        if (ly == 1) ring = ring && g.phase_num(mx, 0, c) == (mx * c) % n;
        if (lx == 1) ring = ring && g.phase_num(0, my, c) == (my * c) % n;
      }
  }
  REQUIRE(inverse, "%d x %d: inverse_code", lx, ly);
  REQUIRE(additive, "%d x %d: phase_num is a character", lx, ly);
  REQUIRE(ring, "%d x %d: with one extent 1 the ring's numerators", lx, ly);
}

static long long binom(int n, int k) {
  long long r = 1;
  for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
  return r;
}

// the whole basis of a block through the slices, as creation joins them
static std::vector<uint32_t> basis(const PauliTorus& g, int n_down, int mx, int my, int top_bits, std::vector<uint8_t>& len) {
  const int n = g.sites();
  top_bits = std::min(top_bits, n);
  std::vector<uint32_t> reps;
  for (uint32_t q = 0; q < ((uint32_t)1 << top_bits); ++q) pauli_torus_slice(g, n_down, mx, my, q, n - top_bits, reps, len);
  return reps;
}

static void test_admission(int lx, int ly) {
  const PauliTorus g(lx, ly);
  const int n = lx * ly;
  const uint32_t full = (uint32_t)(((uint64_t)1 << n) - 1);
  long long excluded_beyond_ring_rule = 0;
  for (int mx = 0; mx < lx; ++mx)
    for (int my = 0; my < ly; ++my) {
      bool same = true;
      std::vector<uint32_t> want;
      std::vector<uint8_t> want_len;
      for (uint32_t r = 0; r <= full; ++r) {
        // independent: every image, the smallest, the stabiliser, the character on it
        uint32_t least = r;
        int stab = 0;
        bool chi_one = true;
        for (int b = 0; b < ly; ++b)
          for (int a = 0; a < lx; ++a) {
            const uint32_t im = shift_sites(r, lx, ly, a, b);
            least = std::min(least, im);
            if (im == r) {
              ++stab;
              // e^(-2 pi i (mx a / lx + my b / ly)) = 1 iff mx a ly + my b lx = 0 mod n
              if ((mx * a * ly + my * b * lx) % n != 0) chi_one = false;
            }
          }
        const int expect = (least == r && chi_one) ? stab : 0;
        same = same && pauli_torus_admit(g, mx, my, r) == expect && (expect == 0 || n % expect == 0);
        // the ring's rule taken per direction, m R = 0, passes an orbit of R = n / stab states that the character excludes
        if (least == r && !chi_one && (mx * (n / stab)) % lx == 0 && (my * (n / stab)) % ly == 0) ++excluded_beyond_ring_rule;
        if (expect) {
          want.push_back(r);
          want_len.push_back((uint8_t)(n / stab));
        }
        if (r == full) break;
      }
      REQUIRE(same, "%d x %d (%d, %d): pauli_torus_admit against the walk over the orbit", lx, ly, mx, my);
      for (int top_bits : {0, 3, 10}) {
        std::vector<uint8_t> len;
        const std::vector<uint32_t> got = basis(g, -1, mx, my, top_bits, len);
        REQUIRE(got == want && len == want_len, "%d x %d (%d, %d): the slices of %d top bits join to the basis", lx, ly, mx, my, top_bits);
      }
      for (int nd = 0; nd <= n; ++nd) {
        std::vector<uint32_t> sect;
        std::vector<uint8_t> sect_len, len;
        for (size_t i = 0; i < want.size(); ++i)
          if (__builtin_popcount(want[i]) == nd) {
            sect.push_back(want[i]);
            sect_len.push_back(want_len[i]);
          }
        const std::vector<uint32_t> got = basis(g, nd, mx, my, 4, len);
        REQUIRE(got == sect && len == sect_len, "%d x %d (%d, %d) n_down %d: the sector's slices", lx, ly, mx, my, nd);
      }
    }
  if (lx == 4 && ly == 2) REQUIRE(excluded_beyond_ring_rule > 0, "4 x 2: no representative that only the character excludes");
}

static void test_sums(int lx, int ly, int n_down, long long d00, long long others_min, long long others_max) {
  const PauliTorus g(lx, ly);
  const int n = lx * ly;
  long long total = 0, lo = -1, hi = -1;
  for (int mx = 0; mx < lx; ++mx)
    for (int my = 0; my < ly; ++my) {
      std::vector<uint8_t> len;
      const std::vector<uint32_t> reps = basis(g, n_down, mx, my, 10, len);
      bool ascending = true;
      for (size_t i = 1; i < reps.size(); ++i) ascending = ascending && reps[i - 1] < reps[i];
      REQUIRE(ascending && len.size() == reps.size(), "%d x %d (%d, %d): ascending", lx, ly, mx, my);
      const long long d = (long long)reps.size();
      total += d;
      if (mx == 0 && my == 0) REQUIRE(d == d00, "%d x %d n_down %d: D(0, 0) = %lld, recorded %lld", lx, ly, n_down, d, d00);
      else {
        lo = lo < 0 ? d : std::min(lo, d);
        hi = std::max(hi, d);
      }
    }
  REQUIRE(total == (n_down < 0 ? (1ll << n) : binom(n, n_down)), "%d x %d n_down %d: the blocks sum to %lld", lx, ly, n_down, total);
  REQUIRE(lo == others_min && hi == others_max, "%d x %d n_down %d: the other blocks span %lld .. %lld, recorded %lld .. %lld", lx, ly,
          n_down, lo, hi, others_min, others_max);
}

int main() {
  for (int lx = 1; lx <= 12; ++lx)
    for (int ly = 1; lx * ly <= 12; ++ly) {
      test_translations(lx, ly);
      if (lx * ly <= 10 || (lx == 4 && ly == 3) || (lx == 3 && ly == 4)) test_admission(lx, ly);
    }
  test_sums(2, 2, -1, 7, 3, 3);
  test_sums(3, 3, -1, 64, 56, 56);
  test_sums(3, 4, -1, 352, 335, 348);
  test_sums(4, 2, 4, 12, 8, 10);
  test_sums(4, 3, 6, 80, 75, 80);
  test_sums(4, 4, 8, 822, 800, 816);
  test_sums(4, 4, -1, 4156, 4080, 4140);
  {  // 5 x 4 at n_down = 10: three recorded blocks
    const PauliTorus g(5, 4);
    std::vector<uint8_t> len;
    REQUIRE(basis(g, 10, 0, 0, 10, len).size() == 9252, "5 x 4 n_down 10 (0, 0)");
    REQUIRE(basis(g, 10, 0, 2, 10, len).size() == 9252, "5 x 4 n_down 10 (0, 2)");
    REQUIRE(basis(g, 10, 1, 2, 10, len).size() == 9250, "5 x 4 n_down 10 (1, 2)");
  }
  {  // thirty sites: the top bits survive both translations
    const PauliTorus g(6, 5);
    const uint32_t v = ((uint32_t)1 << 29) | 1u;
    REQUIRE(g.tx(v) == (((uint32_t)1 << 24) | 2u) && g.ty(v) == (((uint32_t)1 << 5) | 64u) && (g.site_mask() >> 30) == 0,
            "6 x 5: T_x, T_y on the top site");
    REQUIRE(pauli_torus_admit(g, 0, 0, 1u) == 1 && pauli_torus_admit(g, 3, 2, 1u) == 1 && pauli_torus_admit(g, 0, 0, 2u) == 0,
            "6 x 5: one flipped spin");
    REQUIRE(pauli_torus_admit(g, 0, 0, g.site_mask()) == 30 && pauli_torus_admit(g, 1, 0, g.site_mask()) == 0, "6 x 5: all spins flipped");
  }
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
