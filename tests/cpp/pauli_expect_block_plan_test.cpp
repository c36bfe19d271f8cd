// The host-side planning of ll_pauli_expect_block (lambda-lanczos_amd/csrc/pauli_expect_block_plan.hpp) by brute force over ALL
// strings on 4 to 6 sites and all four group choices (shift; + reflection; + flip; + both):
//   the image rules   T, the reflection and the flip act on states as permutations; h P h^-1 |s> evaluated from the definition
//                     P|s> = i^nY (-1)^popcount(s & z) |s ^ x> equals sign * P'|s> with P' and sign what the header says
//   the orbit         closed under the generators in use, multiplicities equal along it, strings ascending by (x, z), none with
//                     multiplicity 0, the multiplicities sum to |G| (or every string cancelled: the flip and popcount(z) odd), and
//                     every multiplicity equals an independent count over the |G| elements
//   the tables        groups by ascending x mask, z masks ascending inside, gptr consistent, tc = (multiplicity / |G|) i^nY folded as
//                     the operators' tables fold it; members of one orbit get identical tables whatever their coefficients
//   the zero rules    exactly: cancelled / real storage and nY odd / a sector and popcount(x) odd
//   the batches       slots in the caller's order, the back-map a bijection on the live observables, ceil(slots / B) batches that
//                     tile the slots.
// Built (plain, and with the address and undefined-behaviour sanitizers) and run by tests/test_pauli_expect_block_plan_host.py.
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

static std::mt19937_64 rng(20261020);
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

// independent of the header: bit by bit
static uint32_t rot1(uint32_t v, int L) {
  uint32_t r = 0;
  for (int i = 0; i < L; ++i)
    if ((v >> i) & 1u) r |= 1u << ((i + 1) % L);
  return r;
}
static uint32_t mirror(uint32_t v, int L) {
  uint32_t r = 0;
  for (int i = 0; i < L; ++i)
    if ((v >> i) & 1u) r |= 1u << (L - 1 - i);
  return r;
}
// P|s> = i^ph |s'>: the definition
static void apply_string(uint32_t x, uint32_t z, uint32_t s, uint32_t* out, int* ph) {
  *out = s ^ x;
  *ph = (popc(x & z) + 2 * (popc(s & z) & 1)) & 3;
}

// h P h^-1 = sign P' for the three generators, on every state
static void test_image_rules(int L) {
  const uint32_t full = (1u << L) - 1;
  for (uint32_t x = 0; x <= full; ++x)
    for (uint32_t z = 0; z <= full; ++z)
      for (int gen = 0; gen < 3; ++gen) {
        const uint32_t ix = gen == 0 ? pauli_block_rotl(x, 1, L) : gen == 1 ? pauli_block_reverse(x, L) : x;
        const uint32_t iz = gen == 0 ? pauli_block_rotl(z, 1, L) : gen == 1 ? pauli_block_reverse(z, L) : z;
        const int sign_ph = (gen == 2 && (popc(z) & 1)) ? 2 : 0;
        bool ok = true;
        for (uint32_t s = 0; s <= full && ok; ++s) {
          // h^-1 s
          uint32_t pre = s;
          if (gen == 0)
            for (int k = 0; k < L - 1; ++k) pre = rot1(pre, L);  // T^-1 = T^(L - 1)
          else if (gen == 1) pre = mirror(s, L);
          else pre = s ^ full;
          uint32_t mid;
          int ph;
          apply_string(x, z, pre, &mid, &ph);
          const uint32_t lhs = gen == 0 ? rot1(mid, L) : gen == 1 ? mirror(mid, L) : (mid ^ full);
          uint32_t rhs;
          int ph2;
          apply_string(ix, iz, s, &rhs, &ph2);
          ok = lhs == rhs && ph == ((ph2 + sign_ph) & 3);
        }
        REQUIRE(ok, "L=%d x=%x z=%x generator %d: the image rule", L, x, z, gen);
      }
}

typedef std::map<std::pair<uint32_t, uint32_t>, int> Count;
// the signed count of every image over the |G| elements, by repeated application of the generators
static Count count_images(int L, bool refl, bool flip, uint32_t x, uint32_t z) {
  Count c;
  for (int rho = 0; rho < (refl ? 2 : 1); ++rho)
    for (int zeta = 0; zeta < (flip ? 2 : 1); ++zeta) {
      uint32_t cx = rho ? mirror(x, L) : x, cz = rho ? mirror(z, L) : z;
      const int sg = (zeta && (popc(z) & 1)) ? -1 : 1;
      for (int j = 0; j < L; ++j) {
        c[{cx, cz}] += sg;
        cx = rot1(cx, L);
        cz = rot1(cz, L);
      }
    }
  return c;
}

static void test_orbits_and_tables(int L, bool refl, bool flip) {
  const uint32_t full = (1u << L) - 1;
  PauliBlockGroup g;
  g.n_sites = L;
  g.reflection = refl;
  g.flip = flip;
  const int G = L * (refl ? 2 : 1) * (flip ? 2 : 1);
  REQUIRE(g.size() == G, "L=%d: |G|", L);
#define CASE "L=%d refl=%d flip=%d x=%x z=%x"
#define CASE_ARGS L, (int)refl, (int)flip, x, z
  for (uint32_t x = 0; x <= full; ++x)
    for (uint32_t z = 0; z <= full; ++z) {
      const std::vector<PauliBlockString> orb = pauli_block_orbit(g, x, z);
      const Count want = count_images(L, refl, flip, x, z);
      Count got;
      long long total = 0;
      for (size_t i = 0; i < orb.size(); ++i) {
        got[{orb[i].x, orb[i].z}] = orb[i].mult;
        total += orb[i].mult;
        REQUIRE(orb[i].mult != 0, CASE ": a cancelled string stayed", CASE_ARGS);
        if (i) REQUIRE(orb[i - 1].x < orb[i].x || (orb[i - 1].x == orb[i].x && orb[i - 1].z < orb[i].z), CASE ": order", CASE_ARGS);
      }
      REQUIRE(got.size() == orb.size(), CASE ": a string twice", CASE_ARGS);
      const bool cancelled = flip && (popc(z) & 1);
      REQUIRE(orb.empty() == cancelled, CASE ": cancellation", CASE_ARGS);
      REQUIRE(total == (cancelled ? 0 : G), CASE ": multiplicities sum to %lld, |G| = %d", CASE_ARGS, total, G);
      bool same = true, closed = true;
      for (const auto& kv : want) same = same && (kv.second == 0 ? got.count(kv.first) == 0 : (got.count(kv.first) && got[kv.first] == kv.second));
      for (const auto& kv : got) same = same && want.count(kv.first) != 0;
      REQUIRE(same, CASE ": multiplicities against the count over the group", CASE_ARGS);
      for (const PauliBlockString& q : orb) {
        auto has = [&](uint32_t ax, uint32_t az) { return got.count({ax, az}) && got[{ax, az}] == q.mult; };
        closed = closed && has(rot1(q.x, L), rot1(q.z, L)) && (!refl || has(mirror(q.x, L), mirror(q.z, L)));
      }
      REQUIRE(closed, CASE ": the orbit is closed under the generators with one multiplicity", CASE_ARGS);

      for (int cplx = 0; cplx < 2; ++cplx)
        for (int sector = 0; sector < 2; ++sector) {
          const Term t{x, z, 1.5};
          const PauliExpectBlockPlan p = pauli_expect_block_plan(g, cplx != 0, sector != 0, 1, &t, 32);
          const int ny = popc(x & z);
          const bool zero = cancelled || (!cplx && (ny & 1)) || (sector && (popc(x) & 1));
          REQUIRE((p.nslots() == 0) == zero && (p.slot[0] < 0) == zero && p.nbatches() == (zero ? 0 : 1), CASE ": the zero rules (cplx %d sector %d)",
                  CASE_ARGS, cplx, sector);
          if (p.nslots() != 1) continue;
          const PauliExpectBlockSlot& s = p.slots[0];
          REQUIRE(s.obs == 0 && s.coef == 1.5 && s.nstrings() == (int64_t)orb.size() && (int64_t)s.gptr.size() == s.ngroups() + 1 &&
                      s.gptr.front() == 0 && s.gptr.back() == (int32_t)orb.size() && s.tc.size() == orb.size() * (cplx ? 2 : 1),
                  CASE ": table sizes", CASE_ARGS);
          bool tables = true;
          size_t k = 0;
          for (int64_t gi = 0; gi < s.ngroups() && tables; ++gi) {
            tables = tables && (gi == 0 || s.gx[(size_t)gi - 1] < s.gx[(size_t)gi]) && s.gptr[(size_t)gi] < s.gptr[(size_t)gi + 1] &&
                     s.gptr[(size_t)gi] == (int32_t)k;
            for (; (int32_t)k < s.gptr[(size_t)gi + 1] && tables; ++k) {
              const double w = (double)orb[k].mult / (double)G, c = (ny & 3) >= 2 ? -w : w;
              tables = orb[k].x == s.gx[(size_t)gi] && orb[k].z == s.tz[k];
              if (cplx) tables = tables && s.tc[2 * k] == ((ny & 1) ? 0.0 : c) && s.tc[2 * k + 1] == ((ny & 1) ? c : 0.0);
              else tables = tables && s.tc[k] == c;
            }
          }
          REQUIRE(tables && k == orb.size(), CASE ": the tables (cplx %d)", CASE_ARGS, cplx);
          // every member of the orbit, with another coefficient: the same tables
          bool identical = true;
          for (const PauliBlockString& q : orb) {
            const Term u{q.x, q.z, -0.25};
            const PauliExpectBlockPlan pu = pauli_expect_block_plan(g, cplx != 0, sector != 0, 1, &u, 32);
            identical = identical && pu.nslots() == 1 && pu.slots[0].gx == s.gx && pu.slots[0].gptr == s.gptr && pu.slots[0].tz == s.tz &&
                        pu.slots[0].tc == s.tc && pu.slots[0].coef == -0.25;
          }
          REQUIRE(identical, CASE ": members of one orbit give identical tables (cplx %d sector %d)", CASE_ARGS, cplx, sector);
        }
    }
#undef CASE
#undef CASE_ARGS
}

static void test_batches(int L, bool refl, bool flip, bool cplx, bool sector, int64_t n_obs, int B) {
  const uint32_t full = (1u << L) - 1;
  PauliBlockGroup g;
  g.n_sites = L;
  g.reflection = refl;
  g.flip = flip;
  std::vector<Term> obs((size_t)n_obs);
  for (Term& t : obs) {
    t.x_mask = (uint32_t)rng() & full;
    t.z_mask = (uint32_t)rng() & full;
    t.coef = (rng() % 7 == 0) ? 0.0 : (double)(int64_t)(rng() % 2001) - 1000.0;
  }
  const PauliExpectBlockPlan p = pauli_expect_block_plan(g, cplx, sector, n_obs, obs.data(), B);
#define CASE "L=%d refl=%d flip=%d cplx=%d sector=%d n_obs=%lld B=%d"
#define CASE_ARGS L, (int)refl, (int)flip, (int)cplx, (int)sector, (long long)n_obs, B
  REQUIRE(p.batch == B && p.n_obs == n_obs && (int64_t)p.slot.size() == n_obs, CASE ": header", CASE_ARGS);
  int64_t live = 0;
  for (int64_t j = 0; j < n_obs; ++j) {
    const Term& t = obs[(size_t)j];
    const bool zero = (flip && (popc(t.z_mask) & 1)) || (!cplx && (popc(t.x_mask & t.z_mask) & 1)) || (sector && (popc(t.x_mask) & 1));
    REQUIRE(p.slot[(size_t)j] == (zero ? -1 : live), CASE ": observable %lld has slot %lld", CASE_ARGS, (long long)j, (long long)p.slot[(size_t)j]);
    if (!zero) {
      if (live < p.nslots())
        REQUIRE(p.slots[(size_t)live].obs == j && p.slots[(size_t)live].coef == t.coef, CASE ": slot %lld maps back", CASE_ARGS, (long long)live);
      ++live;
    }
  }
  REQUIRE(p.nslots() == live, CASE ": %lld slots for %lld live observables", CASE_ARGS, (long long)p.nslots(), (long long)live);
  REQUIRE(p.nbatches() == (live + B - 1) / B, CASE ": %lld batches", CASE_ARGS, (long long)p.nbatches());
  int64_t covered = 0;
  for (int64_t b = 0; b < p.nbatches(); ++b) {
    REQUIRE(p.batch_begin(b) == covered && p.batch_count(b) >= 1 && p.batch_count(b) <= B, CASE ": batch %lld", CASE_ARGS, (long long)b);
    covered += p.batch_count(b);
  }
  REQUIRE(covered == live, CASE ": the batches cover %lld of %lld slots", CASE_ARGS, (long long)covered, (long long)live);
#undef CASE
#undef CASE_ARGS
}

int main() {
  for (int L = 1; L <= 6; ++L) test_image_rules(L);
  for (int L = 4; L <= 6; ++L)
    for (int refl = 0; refl < 2; ++refl)
      for (int flip = 0; flip < 2; ++flip) test_orbits_and_tables(L, refl != 0, flip != 0);
  for (int L : {1, 2, 3}) test_orbits_and_tables(L, true, true);  // the shortest rings: every rotation count stays in range
  for (int L = 1; L <= 6; ++L)
    for (int sym = 0; sym < 4; ++sym)
      for (int cs = 0; cs < 4; ++cs)
        for (int B : {1, 3, 32})
          for (int64_t n_obs : {0, 1, 7, 33, 100}) test_batches(L, (sym & 1) != 0, (sym & 2) != 0, (cs & 1) != 0, (cs & 2) != 0, n_obs, B);
  {  // thirty sites: the masks' top bits survive the rotation and the reflection
    PauliBlockGroup g;
    g.n_sites = 30;
    g.reflection = g.flip = true;
    const std::vector<PauliBlockString> orb = pauli_block_orbit(g, 1u << 29, 1u);
    long long total = 0;
    bool inside = true;
    for (const PauliBlockString& q : orb) {
      total += q.mult;
      inside = inside && (q.x >> 30) == 0 && (q.z >> 30) == 0 && popc(q.x) == 1 && popc(q.z) == 1;
    }
    REQUIRE(orb.empty(), "30 sites, popcount(z) odd under the flip: cancelled");
    g.flip = false;
    const std::vector<PauliBlockString> o2 = pauli_block_orbit(g, 1u << 29, 1u);
    total = 0;
    for (const PauliBlockString& q : o2) {
      total += q.mult;
      inside = inside && (q.x >> 30) == 0 && (q.z >> 30) == 0 && popc(q.x) == 1 && popc(q.z) == 1;
    }
    REQUIRE(inside && total == 60 && o2.size() == 60, "30 sites: X_29 Z_0 has 60 distinct images");
    const PauliExpectBlockPlan p = pauli_expect_block_plan<Term>(g, true, false, 0, nullptr, 32);
    REQUIRE(p.nslots() == 0 && p.nbatches() == 0, "empty plan");
  }
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
