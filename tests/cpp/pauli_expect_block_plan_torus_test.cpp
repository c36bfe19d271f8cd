// The torus group of the planning of ll_pauli_expect_block (lambda-lanczos_amd/csrc/pauli_expect_block_plan.hpp with
// PauliBlockGroup::lx > 0), by brute force over ALL strings on the shapes of 4 to 6 sites and sampled strings on 4 x 3 and 4 x 4:
//   the image rules   T_x and T_y act on states as permutations without signs; h P h^-1 |s> evaluated from the definition
//                     P|s> = i^nY (-1)^popcount(s & z) |s ^ x> equals P'|s> with both masks of P' moved by h
//   the orbit         strings ascending by (x, z), none with multiplicity 0, nothing cancels, the multiplicities sum to |G| = Lx Ly
//                     and equal an independent count over the group; closed under T_x and T_y with one multiplicity
//   the tables        as a ring's: groups by ascending x mask, tc = (multiplicity / |G|) i^nY; members of one orbit get identical
//                     tables whatever their coefficients; the zero rules are the ring's without the flip
//   the ring          with Ly = 1 (and with Lx = 1) the plan is the shift group's of a ring of as many sites, table for table.
// The ring groups stay covered by pauli_expect_block_plan_test.cpp.  Built (plain, and with the address and undefined-behaviour
// sanitizers) and run by tests/test_pauli_torus_plan_host.py.
#include <cstdio>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "pauli_expect_block_plan.hpp"

using namespace ll;

struct Term {
  uint64_t x_mask, z_mask;
  double coef;
};

static std::mt19937_64 rng(20261021);
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

static int popc(uint64_t v) { return __builtin_popcountll(v); }

// independent of the headers: site by site
static uint32_t shift_sites(uint32_t v, int lx, int ly, int dx, int dy) {
  uint32_t r = 0;
  for (int y = 0; y < ly; ++y)
    for (int x = 0; x < lx; ++x)
      if ((v >> (x + lx * y)) & 1u) r |= (uint32_t)1 << ((x + dx) % lx + lx * ((y + dy) % ly));
  return r;
}
static void apply_string(uint32_t x, uint32_t z, uint32_t s, uint32_t* out, int* ph) {
  *out = s ^ x;
  *ph = (popc(x & z) + 2 * (popc(s & z) & 1)) & 3;
}

static PauliBlockGroup torus(int lx, int ly) {
  PauliBlockGroup g;
  g.n_sites = lx * ly;
  g.lx = lx;
  g.ly = ly;
  return g;
}

// h P h^-1 = P' for the two generators, on every state
static void test_image_rules(int lx, int ly) {
  const int n = lx * ly;
  const uint32_t full = (1u << n) - 1;
  const PauliTorus t(lx, ly);
  for (uint32_t x = 0; x <= full; ++x)
    for (uint32_t z = 0; z <= full; ++z)
      for (int gen = 0; gen < 2; ++gen) {
        const uint32_t ix = gen == 0 ? t.tx(x) : t.ty(x), iz = gen == 0 ? t.tx(z) : t.ty(z);
        bool ok = true;
        for (uint32_t s = 0; s <= full && ok; ++s) {
          const uint32_t pre = gen == 0 ? shift_sites(s, lx, ly, lx - 1, 0) : shift_sites(s, lx, ly, 0, ly - 1);  // h^-1 s
          uint32_t mid, rhs;
          int ph, ph2;
          apply_string(x, z, pre, &mid, &ph);
          const uint32_t lhs = gen == 0 ? shift_sites(mid, lx, ly, 1, 0) : shift_sites(mid, lx, ly, 0, 1);
          apply_string(ix, iz, s, &rhs, &ph2);
          ok = lhs == rhs && ph == ph2;
        }
        REQUIRE(ok, "%d x %d x=%x z=%x generator %d: the image rule", lx, ly, x, z, gen);
      }
}

typedef std::map<std::pair<uint32_t, uint32_t>, int> Count;

static void test_string(int lx, int ly, uint32_t x, uint32_t z) {
  const PauliBlockGroup g = torus(lx, ly);
  const int G = lx * ly;
#define CASE "%d x %d x=%x z=%x"
#define CASE_ARGS lx, ly, x, z
  const std::vector<PauliBlockString> orb = pauli_block_orbit(g, x, z);
  Count want, got;
  for (int b = 0; b < ly; ++b)
    for (int a = 0; a < lx; ++a) want[{shift_sites(x, lx, ly, a, b), shift_sites(z, lx, ly, a, b)}] += 1;
  long long total = 0;
  for (size_t i = 0; i < orb.size(); ++i) {
    got[{orb[i].x, orb[i].z}] = orb[i].mult;
    total += orb[i].mult;
    REQUIRE(orb[i].mult > 0, CASE ": a multiplicity that is not positive", CASE_ARGS);
    if (i) REQUIRE(orb[i - 1].x < orb[i].x || (orb[i - 1].x == orb[i].x && orb[i - 1].z < orb[i].z), CASE ": order", CASE_ARGS);
  }
  REQUIRE(g.size() == G && total == G && got == want, CASE ": multiplicities against the count over the group", CASE_ARGS);
  bool closed = true;
  for (const PauliBlockString& q : orb) {
    auto has = [&](uint32_t ax, uint32_t az) { return got.count({ax, az}) && got[{ax, az}] == q.mult; };
    closed = closed && has(shift_sites(q.x, lx, ly, 1, 0), shift_sites(q.z, lx, ly, 1, 0)) &&
             has(shift_sites(q.x, lx, ly, 0, 1), shift_sites(q.z, lx, ly, 0, 1));
  }
  REQUIRE(closed, CASE ": the orbit is closed under T_x and T_y with one multiplicity", CASE_ARGS);
  const int ny = popc(x & z);
  for (int cplx = 0; cplx < 2; ++cplx)
    for (int sector = 0; sector < 2; ++sector) {
      const Term t{x, z, 1.5};
      const PauliExpectBlockPlan p = pauli_expect_block_plan(g, cplx != 0, sector != 0, 1, &t, 32);
      const bool zero = (!cplx && (ny & 1)) || (sector && (popc(x) & 1));
      REQUIRE((p.nslots() == 0) == zero && (p.slot[0] < 0) == zero, CASE ": the zero rules (cplx %d sector %d)", CASE_ARGS, cplx, sector);
      if (p.nslots() != 1) continue;
      const PauliExpectBlockSlot& s = p.slots[0];
      bool tables = s.nstrings() == (int64_t)orb.size() && (int64_t)s.gptr.size() == s.ngroups() + 1 && s.gptr.front() == 0 &&
                    s.gptr.back() == (int32_t)orb.size() && s.tc.size() == orb.size() * (cplx ? 2 : 1);
      size_t k = 0;
      for (int64_t gi = 0; gi < s.ngroups() && tables; ++gi) {
        tables = (gi == 0 || s.gx[(size_t)gi - 1] < s.gx[(size_t)gi]) && s.gptr[(size_t)gi] == (int32_t)k;
        for (; tables && (int32_t)k < s.gptr[(size_t)gi + 1]; ++k) {
          const double w = (double)orb[k].mult / (double)G, c = (ny & 3) >= 2 ? -w : w;
          tables = orb[k].x == s.gx[(size_t)gi] && orb[k].z == s.tz[k];
          if (cplx) tables = tables && s.tc[2 * k] == ((ny & 1) ? 0.0 : c) && s.tc[2 * k + 1] == ((ny & 1) ? c : 0.0);
          else tables = tables && s.tc[k] == c;
        }
      }
      REQUIRE(tables && k == orb.size(), CASE ": the tables (cplx %d)", CASE_ARGS, cplx);
      bool identical = true;
      for (const PauliBlockString& q : orb) {
        const Term u{q.x, q.z, -0.25};
        const PauliExpectBlockPlan pu = pauli_expect_block_plan(g, cplx != 0, sector != 0, 1, &u, 32);
        identical = identical && pu.nslots() == 1 && pu.slots[0].gx == s.gx && pu.slots[0].gptr == s.gptr && pu.slots[0].tz == s.tz &&
                    pu.slots[0].tc == s.tc && pu.slots[0].coef == -0.25;
      }
      REQUIRE(identical, CASE ": members of one orbit give identical tables (cplx %d sector %d)", CASE_ARGS, cplx, sector);
    }
#undef CASE
#undef CASE_ARGS
}

// Ly = 1 and Lx = 1: the ring's shift group
static void test_ring(int L) {
  PauliBlockGroup ring;
  ring.n_sites = L;
  const uint32_t full = (1u << L) - 1;
  bool same = true;
  for (uint32_t x = 0; x <= full; ++x)
    for (uint32_t z = 0; z <= full; ++z) {
      const Term t{x, z, 2.0};
      const PauliExpectBlockPlan want = pauli_expect_block_plan(ring, true, false, 1, &t, 32);
      for (int flat = 0; flat < 2; ++flat) {
        const PauliExpectBlockPlan got = pauli_expect_block_plan(flat ? torus(L, 1) : torus(1, L), true, false, 1, &t, 32);
        same = same && got.nslots() == want.nslots() &&
               (got.nslots() == 0 || (got.slots[0].gx == want.slots[0].gx && got.slots[0].gptr == want.slots[0].gptr &&
                                      got.slots[0].tz == want.slots[0].tz && got.slots[0].tc == want.slots[0].tc));
      }
    }
  REQUIRE(same, "L=%d: the torus of one row (one column) plans as the ring", L);
}

int main() {
  for (int lx = 1; lx <= 4; ++lx)
    for (int ly = 1; lx * ly <= 4; ++ly) test_image_rules(lx, ly);
  test_image_rules(3, 2);
  test_image_rules(2, 3);
  const int shapes[][2] = {{2, 2}, {4, 1}, {1, 4}, {5, 1}, {3, 2}, {2, 3}, {6, 1}, {1, 6}};
  for (const auto& sh : shapes) {
    const uint32_t full = (1u << (sh[0] * sh[1])) - 1;
    for (uint32_t x = 0; x <= full; ++x)
      for (uint32_t z = 0; z <= full; ++z) test_string(sh[0], sh[1], x, z);
  }
  const int large[][2] = {{4, 3}, {3, 4}, {4, 4}, {6, 5}};
  for (const auto& sh : large) {
    const uint32_t full = (uint32_t)(((uint64_t)1 << (sh[0] * sh[1])) - 1);
    for (int k = 0; k < 300; ++k) test_string(sh[0], sh[1], (uint32_t)rng() & full, (uint32_t)rng() & full);
    test_string(sh[0], sh[1], 0u, 1u | (1u << (sh[0] + 1)));                     // Z_(0,0) Z_(1,1)
    test_string(sh[0], sh[1], 0x5u & full, 0u);                                  // X X two sites apart
    test_string(sh[0], sh[1], 0u, full);                                         // invariant: one image |G| times
  }
  for (int L = 1; L <= 6; ++L) test_ring(L);
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
