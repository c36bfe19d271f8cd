// Host-side planning of ll_pauli_rdm (kernels: pauli_rdm.hip): the reduced density matrix rho_A = Tr_env |psi><psi| of m <= 6
// sites.  Plain integers in, plain structs out — standard headers only, so the arithmetic builds with a host compiler and is
// checked on the CPU, property by property, in tests/cpp/pauli_rdm_plan_test.cpp.  The few functions the kernels call too carry
// LL_RDM_HD (empty for a host compiler): one definition of where an amplitude lies.
//
// Bit k of the subsystem index a is site sites[k]; e numbers the configurations of the other sites (its bits fill the
// environment mask in ascending order).  state = deposit(a) | deposit_env(e), and rho[a][a'] = sum_e psi(a, e) conj psi(a', e).
//
// Full space.  A tile is 2^t consecutive states.  The subsystem sites split at t: the n_lo sites below it permute a tile, the h
// sites at or above it select one of the 2^h tiles of a SUPER-TILE — tiles that differ in those bits of the tile number only.
// A workgroup holds a super-tile in LDS as [tile j][offset]: 2^(t + h) elements; tile j of super-tile u is tile number
// insert_zeros(u, hi_bit) | deposit(j, hi_bit).  The super-tile holds 2^(t - n_lo) ROWS (environment configurations: the offset
// bits that are not subsystem sites); amplitude a of row r lies at LDS index lds_offset(a) | insert_zeros(r, lo_bit).
//
// Ownership.  rho is cut into R x R blocks (R = block_edge(m)); the nb (nb + 1) / 2 blocks of the upper triangle are numbered
// row by row.  Thread tid owns block tid % NB for the row slice tid / NB: rows slice, slice + S, ... with S = 256 / NB slices;
// threads at or above NB S own nothing.  Every entry a <= a' has exactly one owner per slice.
//
// Sector (n_down set bits): the configuration e admits only the a with popcount(a) = n_down - popcount(e).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define LL_RDM_HD __host__ __device__
#else
#define LL_RDM_HD
#endif

namespace ll {

constexpr int kPauliRdmMaxSites = 6;  // m at most: 64 x 64 entries, at most 16 (complex) per lane
constexpr int kPauliRdmThreads = 256; // the workgroup the thread-to-entry map is made for

enum PauliRdmSiteError { kRdmSitesOk = 0, kRdmBadCount, kRdmSiteOutOfRange, kRdmSiteRepeated };
// the site list of the caller; *which: the index k of the first offending sites[k]
inline PauliRdmSiteError pauli_rdm_check_sites(int n_sites, int n_sub, const int32_t* sites, int* which) {
  *which = -1;
  if (n_sub < 1 || n_sub > kPauliRdmMaxSites || n_sub > n_sites) return kRdmBadCount;
  for (int k = 0; k < n_sub; ++k)
    if (sites[k] < 0 || sites[k] >= n_sites) return *which = k, kRdmSiteOutOfRange;
  for (int k = 1; k < n_sub; ++k)
    for (int j = 0; j < k; ++j)
      if (sites[j] == sites[k]) return *which = k, kRdmSiteRepeated;
  return kRdmSitesOk;
}

// v with a zero bit inserted at each of the positions bits[0] < bits[1] < ... (positions in the RESULT)
LL_RDM_HD inline uint32_t pauli_rdm_insert_zeros(uint32_t v, const uint8_t* bits, int count) {
  for (int k = 0; k < count; ++k) {
    const uint32_t below = (1u << bits[k]) - 1u;
    v = ((v & ~below) << 1) | (v & below);
  }
  return v;
}
// the inverse: the bits of v at those positions removed (whatever they hold)
inline uint32_t pauli_rdm_remove_bits(uint32_t v, const uint8_t* bits, int count) {
  for (int k = count - 1; k >= 0; --k) {
    const uint32_t below = (1u << bits[k]) - 1u;
    v = ((v >> 1) & ~below) | (v & below);
  }
  return v;
}

// ---- the thread-to-entry map
LL_RDM_HD constexpr int pauli_rdm_block_edge(int m) { return m <= 2 ? 1 : (m == 3 ? 2 : 4); }
LL_RDM_HD constexpr int pauli_rdm_blocks_per_side(int m) { return (1 << m) / pauli_rdm_block_edge(m); }
LL_RDM_HD constexpr int pauli_rdm_blocks(int m) { return pauli_rdm_blocks_per_side(m) * (pauli_rdm_blocks_per_side(m) + 1) / 2; }
LL_RDM_HD constexpr int pauli_rdm_slices(int m) { return kPauliRdmThreads / pauli_rdm_blocks(m); }
// doubles of one workgroup's partials: [block][i][j][re, im]
LL_RDM_HD constexpr int pauli_rdm_partials(int m, bool complex_storage) {
  return pauli_rdm_blocks(m) * pauli_rdm_block_edge(m) * pauli_rdm_block_edge(m) * (complex_storage ? 2 : 1);
}
struct PauliRdmBlock {
  int bi, bj;  // block row <= block column
};
// block number -> (bi, bj), row by row over the upper triangle of nb x nb blocks
LL_RDM_HD inline PauliRdmBlock pauli_rdm_block_of(int nb, int blk) {
  int bi = 0;
  while (blk >= nb - bi) {
    blk -= nb - bi;
    ++bi;
  }
  return PauliRdmBlock{bi, bi + blk};
}
LL_RDM_HD constexpr int pauli_rdm_block_number(int nb, int bi, int bj) { return bi * nb - bi * (bi - 1) / 2 + (bj - bi); }
// where entry (a <= a') lies in a workgroup's partials (the real part; the imaginary part follows it for complex storage)
inline int pauli_rdm_partial_index(int m, bool complex_storage, int a, int ap) {
  const int R = pauli_rdm_block_edge(m), nb = pauli_rdm_blocks_per_side(m);
  const int blk = pauli_rdm_block_number(nb, a / R, ap / R);
  return ((blk * R + a % R) * R + ap % R) * (complex_storage ? 2 : 1);
}

// ---- the geometry a kernel receives
struct PauliRdmGeom {
  int32_t n_sites, m;
  int32_t t, h, n_lo;      // full space: tile bits, subsystem sites at or above / below the tile
  uint8_t lo_bit[kPauliRdmMaxSites];   // the sites below t, ascending
  uint8_t hi_bit[kPauliRdmMaxSites];   // the sites at or above t, ascending, minus t: bits of the tile number
  uint8_t all_bit[kPauliRdmMaxSites];  // all sites, ascending (the environment mask's holes)
  uint32_t lds_bit[kPauliRdmMaxSites]; // bit k of a -> its bit of the LDS index [tile j][offset]
  uint32_t site_bit[kPauliRdmMaxSites];// bit k of a -> 1 << sites[k]
  uint32_t env_mask;                   // the sites outside the subsystem
};

// the deposit of a: bit k of a to site sites[k] (site_bit) or to the LDS index (lds_bit)
LL_RDM_HD inline uint32_t pauli_rdm_deposit(uint32_t a, const uint32_t* bit_of, int m) {
  uint32_t v = 0;
  for (int k = 0; k < m; ++k)
    if ((a >> k) & 1u) v |= bit_of[k];
  return v;
}
inline uint32_t pauli_rdm_extract(uint32_t state, const uint32_t* bit_of, int m) {
  uint32_t a = 0;
  for (int k = 0; k < m; ++k)
    if (state & bit_of[k]) a |= 1u << k;
  return a;
}

// sites must have passed pauli_rdm_check_sites; 0 <= t <= n_sites
inline PauliRdmGeom pauli_rdm_geom(int n_sites, int m, const int32_t* sites, int t) {
  PauliRdmGeom g{};
  g.n_sites = n_sites;
  g.m = m;
  g.t = t;
  uint32_t sub = 0;
  for (int k = 0; k < m; ++k) sub |= g.site_bit[k] = 1u << sites[k];
  g.env_mask = (n_sites >= 32 ? ~0u : ((1u << n_sites) - 1u)) & ~sub;
  int n_all = 0;
  for (int s = 0; s < n_sites; ++s) {
    if (!((sub >> s) & 1u)) continue;
    g.all_bit[n_all++] = (uint8_t)s;
    if (s < t) g.lo_bit[g.n_lo++] = (uint8_t)s;
    else g.hi_bit[g.h++] = (uint8_t)(s - t);
  }
  for (int k = 0; k < m; ++k) {
    if (sites[k] < t) {
      g.lds_bit[k] = 1u << sites[k];
    } else {
      int rank = 0;
      for (int j = 0; j < g.h; ++j)
        if (g.hi_bit[j] + t < sites[k]) ++rank;
      g.lds_bit[k] = 1u << (t + rank);
    }
  }
  return g;
}
inline int pauli_rdm_high_sites(int m, const int32_t* sites, int t) {
  int h = 0;
  for (int k = 0; k < m; ++k) h += sites[k] >= t;
  return h;
}
// The tile: forced (>= 0: the key pauli_rdm_tile_bits) or n_sites, lowered until the super-tile 2^(t + h(t)) elem_bytes fits
// budget bytes of LDS (t = 0 always fits: 64 elements at most).
inline int pauli_rdm_tile_bits(int n_sites, int m, const int32_t* sites, int elem_bytes, int forced, int64_t budget) {
  int t = forced >= 0 && forced < n_sites ? forced : n_sites;
  while (t > 0 && ((int64_t)elem_bytes << (t + pauli_rdm_high_sites(m, sites, t))) > budget) --t;
  return t;
}
inline int64_t pauli_rdm_super_tiles(const PauliRdmGeom& g) { return (int64_t)1 << (g.n_sites - g.t - g.h); }
inline int64_t pauli_rdm_rows_per_super_tile(const PauliRdmGeom& g) { return (int64_t)1 << (g.t - g.n_lo); }
// the tile number of tile j (its bit k is hi_bit[k]) of super-tile u
LL_RDM_HD inline uint32_t pauli_rdm_tile_number(const PauliRdmGeom& g, uint32_t u, uint32_t j) {
  uint32_t tile = pauli_rdm_insert_zeros(u, g.hi_bit, g.h);
  for (int k = 0; k < g.h; ++k)
    if ((j >> k) & 1u) tile |= 1u << g.hi_bit[k];
  return tile;
}
// the LDS index of amplitude a of row r of a super-tile
LL_RDM_HD inline uint32_t pauli_rdm_lds_index(const PauliRdmGeom& g, uint32_t a, uint32_t r) {
  return pauli_rdm_deposit(a, g.lds_bit, g.m) | pauli_rdm_insert_zeros(r, g.lo_bit, g.n_lo);
}
// the state that LDS index idx of super-tile u holds
inline uint64_t pauli_rdm_state_of(const PauliRdmGeom& g, uint32_t u, uint32_t idx) {
  return ((uint64_t)pauli_rdm_tile_number(g, u, idx >> g.t) << g.t) | (idx & ((1u << g.t) - 1u));
}

// ---- one S_z sector
// the popcount of a that the environment configuration e admits: negative or above m — none
LL_RDM_HD inline int pauli_rdm_sector_popcount(int n_down, uint32_t e) { return n_down - __builtin_popcount(e); }
// a row a of rho that no environment configuration admits: n_down - popcount(a) outside [0, n_sites - m]
inline bool pauli_rdm_sector_row_is_zero(int n_sites, int m, int n_down, uint32_t a) {
  const int rest = n_down - __builtin_popcount(a);
  return rest < 0 || rest > n_sites - m;
}
// environment configurations per LDS batch, 2^b rows of 2^m elements: forced (>= 0: the key pauli_rdm_block_bits) or all of
// them, lowered until the batch fits budget bytes of LDS
inline int pauli_rdm_block_bits(int n_sites, int m, int elem_bytes, int forced, int64_t budget) {
  int b = forced >= 0 && forced < n_sites - m ? forced : n_sites - m;
  while (b > 0 && ((int64_t)elem_bytes << (b + m)) > budget) --b;
  return b;
}
// the state of (a, e): e fills the environment mask in ascending order
LL_RDM_HD inline uint32_t pauli_rdm_state(const PauliRdmGeom& g, uint32_t a, uint32_t e) {
  return pauli_rdm_deposit(a, g.site_bit, g.m) | pauli_rdm_insert_zeros(e, g.all_bit, g.m);
}

}  // namespace ll
