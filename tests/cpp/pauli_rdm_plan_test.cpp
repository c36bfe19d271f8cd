// The host-side planning of ll_pauli_rdm (lambda-lanczos_amd/csrc/pauli_rdm_plan.hpp) against properties that follow from what
// the kernels READ and from the definition rho[a][a'] = sum_e psi(a, e) conj psi(a', e), by brute force over site lists of every
// m at up to 12 sites and several tile sizes:
//   - every state index is produced exactly once by (super-tile, tile, offset), and the LDS index of (amplitude a, row r) holds
//     the state whose subsystem bits are a — every row of a super-tile is one environment configuration, met once;
//   - every entry a <= a' is owned by exactly one thread per row slice, slices cover the rows once, and the partial index is a
//     bijection onto [0, partials);
//   - deposit and extract are inverse to each other, insert_zeros and remove_bits too;
//   - the tile and the batch fit the LDS budget; the site checks name the first offender;
//   - in a sector, (a, e) with popcount(a) = n_down - popcount(e) enumerates the sector's states exactly once.
// Built (plain, and with the address and undefined-behaviour sanitizers) and run by tests/test_pauli_rdm_plan_host.py.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "pauli_rdm_plan.hpp"

using namespace ll;

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

static std::vector<int32_t> random_sites(int n_sites, int m) {
  std::vector<int32_t> all((size_t)n_sites);
  for (int s = 0; s < n_sites; ++s) all[(size_t)s] = s;
  std::shuffle(all.begin(), all.end(), rng);
  all.resize((size_t)m);
  return all;
}

static void check_full(int n_sites, const std::vector<int32_t>& sites, int t) {
  const int m = (int)sites.size();
  const PauliRdmGeom g = pauli_rdm_geom(n_sites, m, sites.data(), t);
  REQUIRE(g.h + g.n_lo == m && g.h == pauli_rdm_high_sites(m, sites.data(), t), "n=%d m=%d t=%d: h + n_lo", n_sites, m, t);
  REQUIRE(g.t + g.h <= n_sites, "n=%d m=%d t=%d: the super-tile is longer than the vector", n_sites, m, t);
  const int64_t nsuper = pauli_rdm_super_tiles(g), nrows = pauli_rdm_rows_per_super_tile(g);
  const uint32_t total = 1u << (g.t + g.h);
  std::vector<int> seen((size_t)1 << n_sites, 0);
  std::vector<int> env_seen((size_t)1 << (n_sites - m), 0);
  for (int64_t u = 0; u < nsuper; ++u) {
    // what the loading loop copies: LDS index idx <- the state of (tile idx >> t, offset)
    for (uint32_t idx = 0; idx < total; ++idx) {
      const uint64_t s = pauli_rdm_state_of(g, (uint32_t)u, idx);
      REQUIRE(s < ((uint64_t)1 << n_sites), "n=%d t=%d: state %llu past the vector", n_sites, t, (unsigned long long)s);
      if (s < seen.size()) ++seen[(size_t)s];
    }
    // what the row loop reads: amplitude a of row r
    std::vector<int> lds_seen(total, 0);
    for (int64_t r = 0; r < nrows; ++r) {
      uint32_t env = ~0u;
      for (uint32_t a = 0; a < (1u << m); ++a) {
        const uint32_t idx = pauli_rdm_lds_index(g, a, (uint32_t)r);
        REQUIRE(idx < total, "n=%d t=%d: LDS index %u of %u", n_sites, t, idx, total);
        if (idx >= total) continue;
        ++lds_seen[idx];
        const uint32_t s = (uint32_t)pauli_rdm_state_of(g, (uint32_t)u, idx);
        REQUIRE(pauli_rdm_extract(s, g.site_bit, m) == a, "n=%d t=%d: row %lld amplitude %u holds another a", n_sites, t, (long long)r, a);
        const uint32_t e = pauli_rdm_remove_bits(s, g.all_bit, m);
        REQUIRE(env == ~0u || env == e, "n=%d t=%d: row %lld mixes environment configurations", n_sites, t, (long long)r);
        env = e;
        REQUIRE(pauli_rdm_state(g, a, e) == s, "n=%d t=%d: deposit(a, e) != state", n_sites, t);
      }
      if (env < env_seen.size()) ++env_seen[env];
    }
    REQUIRE(std::all_of(lds_seen.begin(), lds_seen.end(), [](int c) { return c == 1; }), "n=%d t=%d: an LDS element is not read exactly once", n_sites, t);
  }
  REQUIRE(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }), "n=%d m=%d t=%d: a state is not loaded exactly once", n_sites, m, t);
  REQUIRE(std::all_of(env_seen.begin(), env_seen.end(), [](int c) { return c == 1; }), "n=%d m=%d t=%d: a row is not met exactly once", n_sites, m, t);
}

static void check_ownership(int m) {
  const int R = pauli_rdm_block_edge(m), nb = pauli_rdm_blocks_per_side(m), NB = pauli_rdm_blocks(m), S = pauli_rdm_slices(m);
  const int dim = 1 << m;
  REQUIRE(S >= 1 && NB * S <= kPauliRdmThreads, "m=%d: %d blocks x %d slices", m, NB, S);
  REQUIRE(m > 3 || NB * (S + 1) > kPauliRdmThreads, "m=%d: lanes left idle that a further slice would fill", m);
  std::vector<int> owners((size_t)S * dim * dim, 0);
  for (int tid = 0; tid < kPauliRdmThreads; ++tid) {
    const int blk = tid % NB, slice = tid / NB;
    if (slice >= S) continue;
    const PauliRdmBlock b = pauli_rdm_block_of(nb, blk);
    REQUIRE(0 <= b.bi && b.bi <= b.bj && b.bj < nb, "m=%d: block %d -> (%d, %d)", m, blk, b.bi, b.bj);
    REQUIRE(pauli_rdm_block_number(nb, b.bi, b.bj) == blk, "m=%d: block_number is not the inverse of block_of at %d", m, blk);
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < R; ++j) ++owners[((size_t)slice * dim + (size_t)(b.bi * R + i)) * dim + (size_t)(b.bj * R + j)];
  }
  for (int s = 0; s < S; ++s)
    for (int a = 0; a < dim; ++a)
      for (int ap = a; ap < dim; ++ap)
        REQUIRE(owners[((size_t)s * dim + a) * dim + ap] == 1, "m=%d: entry (%d, %d) has %d owners in slice %d", m, a, ap,
                owners[((size_t)s * dim + a) * dim + ap], s);
  // rows slice, slice + S, ...: every row in exactly one slice
  for (int nrows : {1, 2, 7, 64, 100}) {
    std::vector<int> hit((size_t)nrows, 0);
    for (int s = 0; s < S; ++s)
      for (int r = s; r < nrows; r += S) ++hit[(size_t)r];
    REQUIRE(std::all_of(hit.begin(), hit.end(), [](int c) { return c == 1; }), "m=%d: a row of %d is not in exactly one slice", m, nrows);
  }
  for (bool cplx : {false, true}) {
    const int P = pauli_rdm_partials(m, cplx), nc = cplx ? 2 : 1;
    std::vector<int> used((size_t)P, 0);
    for (int a = 0; a < dim; ++a)
      for (int ap = a; ap < dim; ++ap) {
        const int i = pauli_rdm_partial_index(m, cplx, a, ap);
        REQUIRE(i >= 0 && i + nc <= P, "m=%d: partial index %d of %d", m, i, P);
        for (int c = 0; c < nc && i >= 0 && i + nc <= P; ++c) ++used[(size_t)(i + c)];
      }
    REQUIRE(std::all_of(used.begin(), used.end(), [](int c) { return c <= 1; }), "m=%d: two entries share a partial", m);
  }
}

static void check_sector(int n_sites, int n_down, const std::vector<int32_t>& sites) {
  const int m = (int)sites.size();
  const PauliRdmGeom g = pauli_rdm_geom(n_sites, m, sites.data(), 0);
  std::vector<int> seen((size_t)1 << n_sites, 0);
  for (uint32_t e = 0; e < (1u << (n_sites - m)); ++e) {
    const int p = pauli_rdm_sector_popcount(n_down, e);
    for (uint32_t a = 0; a < (1u << m); ++a) {
      if (__builtin_popcount(a) != p) continue;
      REQUIRE(!pauli_rdm_sector_row_is_zero(n_sites, m, n_down, a), "(%d, %d): a row that is met counts as zero", n_sites, n_down);
      ++seen[pauli_rdm_state(g, a, e)];
    }
  }
  std::vector<int> row_met((size_t)1 << m, 0);
  for (uint32_t s = 0; s < (1u << n_sites); ++s) {
    REQUIRE(seen[s] == (__builtin_popcount(s) == n_down ? 1 : 0), "(%d, %d): state %u met %d times", n_sites, n_down, s, seen[s]);
    if (seen[s]) row_met[pauli_rdm_extract(s, g.site_bit, m)] = 1;
  }
  for (uint32_t a = 0; a < (1u << m); ++a)
    REQUIRE(pauli_rdm_sector_row_is_zero(n_sites, m, n_down, a) == !row_met[a], "(%d, %d): the zero rule of row %u", n_sites, n_down, a);
}

int main() {
  // the bit helpers
  for (int trial = 0; trial < 2000; ++trial) {
    const int n_sites = 1 + (int)(rng() % 30), m = 1 + (int)(rng() % (uint64_t)std::min(6, n_sites));
    const std::vector<int32_t> sites = random_sites(n_sites, m);
    const PauliRdmGeom g = pauli_rdm_geom(n_sites, m, sites.data(), (int)(rng() % (uint64_t)(n_sites + 1)));
    const uint32_t a = (uint32_t)(rng() & ((1u << m) - 1u));
    const uint32_t e = (uint32_t)(rng() & (((uint64_t)1 << (n_sites - m)) - 1u));
    REQUIRE(pauli_rdm_extract(pauli_rdm_deposit(a, g.site_bit, m), g.site_bit, m) == a, "extract(deposit(a)) != a");
    REQUIRE(pauli_rdm_extract(pauli_rdm_deposit(a, g.lds_bit, m), g.lds_bit, m) == a, "the LDS bits of a collide");
    const uint32_t s = pauli_rdm_state(g, a, e);
    REQUIRE((s & g.env_mask) == pauli_rdm_insert_zeros(e, g.all_bit, m) && (s & ~g.env_mask) == pauli_rdm_deposit(a, g.site_bit, m), "state(a, e) mixes its parts");
    REQUIRE(pauli_rdm_remove_bits(s, g.all_bit, m) == e && pauli_rdm_extract(s, g.site_bit, m) == a, "state(a, e) does not come apart");
    REQUIRE(__builtin_popcount(g.env_mask) == n_sites - m, "the environment mask");
  }
  // the site checks
  {
    int which = 0;
    const int32_t ok[3] = {4, 0, 2}, far[3] = {0, 5, 1}, neg[2] = {1, -1}, twice[4] = {3, 1, 2, 1}, seven[7] = {0, 1, 2, 3, 4, 5, 6};
    REQUIRE(pauli_rdm_check_sites(5, 3, ok, &which) == kRdmSitesOk, "a valid list is refused");
    REQUIRE(pauli_rdm_check_sites(5, 3, far, &which) == kRdmSiteOutOfRange && which == 1, "site 5 of 5");
    REQUIRE(pauli_rdm_check_sites(5, 2, neg, &which) == kRdmSiteOutOfRange && which == 1, "a negative site");
    REQUIRE(pauli_rdm_check_sites(5, 4, twice, &which) == kRdmSiteRepeated && which == 3, "a repeated site");
    REQUIRE(pauli_rdm_check_sites(9, 7, seven, &which) == kRdmBadCount, "seven sites");
    REQUIRE(pauli_rdm_check_sites(9, 0, seven, &which) == kRdmBadCount, "no site");
    REQUIRE(pauli_rdm_check_sites(2, 3, ok, &which) == kRdmBadCount, "more sites than the chain has");
  }
  for (int m = 1; m <= kPauliRdmMaxSites; ++m) check_ownership(m);
  // the geometry: every m at up to 12 sites, several tiles (0, a middle one, n_sites, and what the budget gives)
  for (int n_sites = 1; n_sites <= 12; ++n_sites) {
    for (int m = 1; m <= std::min(6, n_sites); ++m) {
      for (int trial = 0; trial < 3; ++trial) {
        std::vector<int32_t> sites = random_sites(n_sites, m);
        if (trial == 1) for (int k = 0; k < m; ++k) sites[(size_t)k] = k;                  // the lowest sites
        if (trial == 2) for (int k = 0; k < m; ++k) sites[(size_t)k] = n_sites - 1 - k;    // the highest, descending
        for (int forced : {-1, 0, 3, 6, 9, 12}) {
          for (int elem : {4, 16}) {
            const int64_t budget = forced < 0 ? 1024 : 32768;   // a small default budget: the lowering loop runs
            const int t = pauli_rdm_tile_bits(n_sites, m, sites.data(), elem, forced, budget);
            const int h = pauli_rdm_high_sites(m, sites.data(), t);
            REQUIRE(t >= 0 && t <= n_sites, "tile bits %d at %d sites", t, n_sites);
            REQUIRE(((int64_t)elem << (t + h)) <= budget || t == 0, "n=%d m=%d: the super-tile 2^(%d + %d) x %d exceeds %lld", n_sites, m, t, h, elem, (long long)budget);
            REQUIRE(forced < 0 || t <= forced, "a forced tile grew");
            if (elem == 16) check_full(n_sites, sites, t);
          }
        }
        for (int forced : {-1, 0, 4, 7}) {
          const int b = pauli_rdm_block_bits(n_sites, m, 16, forced, 32768);
          REQUIRE(b >= 0 && b <= n_sites - m && ((int64_t)16 << (b + m)) <= 32768, "n=%d m=%d: block bits %d", n_sites, m, b);
          REQUIRE(forced < 0 || b <= forced, "a forced batch grew");
        }
        for (int n_down : {0, 1, n_sites / 2, n_sites}) check_sector(n_sites, n_down, sites);
      }
    }
  }
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
