// Host-side planning of ll_pauli_rdm_tiled (kernels: pauli_rdm_tiled.hip): the reduced density matrix of 4 to 13 sites as the
// Hermitian rank-K update rho = F F^H, F the 2^m x 2^(n - m) matrix of fibres psi(a, e), on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64).  Plain integers in, plain structs out — standard headers only, so the arithmetic builds with a host
// compiler and is checked on the CPU, property by property, in tests/cpp/pauli_rdm_tiled_plan_test.cpp.  What the kernels call
// too carries LL_RDM_HD (pauli_rdm_plan.hpp): one definition of where an amplitude lies and of which lane holds which entry.
//
// Internal row order.  The subsystem sites are sorted ascending; bit k of the INTERNAL index is the k-th lowest site.  The
// rb = min(m, 6) lowest sites are the ROW BITS of a block of 64 rows (2^rb of them hold data; the others are zero padding at
// m = 4, 5), the bb = m - rb sites above them the BLOCK BITS: internal index = block << 6 | row for m >= 6.  The caller's index
// (bit k = sites[k], any order) maps to the internal one by a bit deposit (int_bit); the finishing kernel applies it per index.
//
// Macro-tiles.  rho is cut into nb x nb blocks of EDGE x EDGE, nb = 2^bb; the nb (nb + 1) / 2 of the upper triangle are numbered
// row by row (pauli_rdm_block_of).  One workgroup of 4 waves forms one macro-tile for one slice of K; wave w owns the quadrant
// (w >> 1, w & 1) of 32 x 32 = 2 x 2 MFMA tiles of 16 x 16.  On a diagonal macro-tile the quadrant (1, 0) lies below the diagonal
// and is not formed.
//
// K loop.  e numbers the 2^(n - m) environment configurations (its bits fill the environment mask in ascending order).  A K-step
// stages KC consecutive e of the row block and of the column block: the states of one panel are
//   base(block, step) | deposit(counter, row-site mask | the positions of the low kb bits of e),   kb = min(log2 KC, n - m),
// ascending in the counter, so that consecutive lanes read consecutive addresses wherever the set is contiguous; the (row, k) of
// a state — its LDS place — is the extract of the two masks.  Where 2^(n - m) < KC the columns k >= 2^kb stay zero.
//
// Split-K.  The nk = max(1, 2^(n - m) / KC) K-steps are dealt to ksplit slices (a power of two) of consecutive steps; every
// (macro-tile, slice) writes its 64 x 64 partial; the finishing kernel folds the slices in slice order.
#pragma once

#include <cstdint>

#include "pauli_rdm_plan.hpp"

namespace ll {

constexpr int kPauliRdmTiledMinSites = 4;   // 2^m is a multiple of the 16-row MFMA tile
// Above 13 sites the 4^m entries (1 GiB at 13) and their eigen-decomposition limit the workflow, not this kernel
constexpr int kPauliRdmTiledMaxSites = 13;
constexpr int kPauliRdmTiledEdge = 64;       // the macro-tile this file's kernels are instantiated for
constexpr int kPauliRdmTiledRowBits = 6;
constexpr int kPauliRdmTiledMinKc = 4, kPauliRdmTiledMaxKc = 16, kPauliRdmTiledDefaultKc = 16;
constexpr int kPauliRdmTiledLdsStride = 80;  // doubles per k of a panel plane: 64 rows + 16, so that k and k + 1 differ by 32 banks
constexpr int kPauliRdmTiledFillFactor = 2;  // tiles x ksplit reaches this multiple of the CU count when K allows
constexpr int64_t kPauliRdmTiledSplitBytes = (int64_t)64 << 20;  // the partials of a call with ksplit > 1 stay within this

// the site list of the caller, as pauli_rdm_check_sites with this entry point's range of n_sub
inline PauliRdmSiteError pauli_rdm_tiled_check_sites(int n_sites, int n_sub, const int32_t* sites, int* which) {
  *which = -1;
  if (n_sub < kPauliRdmTiledMinSites || n_sub > kPauliRdmTiledMaxSites || n_sub > n_sites) return kRdmBadCount;
  for (int k = 0; k < n_sub; ++k)
    if (sites[k] < 0 || sites[k] >= n_sites) return *which = k, kRdmSiteOutOfRange;
  for (int k = 1; k < n_sub; ++k)
    for (int j = 0; j < k; ++j)
      if (sites[j] == sites[k]) return *which = k, kRdmSiteRepeated;
  return kRdmSitesOk;
}

// ---- the lane maps of v_mfma_f64_16x16x4_f64: D (16 x 16) = A (16 x 4) B (4 x 16) + C, one double of A and of B and four of
// C / D per lane.  B[k][j] is fed F_col[j][k]: the column panel is read by the same map as the row panel.
LL_RDM_HD constexpr int pauli_mfma_f64_ab_row(int lane) { return lane & 15; }  // A: the row i; B: the column j
LL_RDM_HD constexpr int pauli_mfma_f64_ab_k(int lane) { return lane >> 4; }
LL_RDM_HD constexpr int pauli_mfma_f64_cd_col(int lane) { return lane & 15; }
LL_RDM_HD constexpr int pauli_mfma_f64_cd_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }

// ---- which wave forms what of a macro-tile
LL_RDM_HD constexpr int pauli_rdm_tiled_wave_row0(int wave) { return 32 * (wave >> 1); }
LL_RDM_HD constexpr int pauli_rdm_tiled_wave_col0(int wave) { return 32 * (wave & 1); }
LL_RDM_HD constexpr bool pauli_rdm_tiled_wave_live(bool diagonal, int wave) { return !(diagonal && wave == 2); }
// (row, column) inside the macro-tile of register reg of lane `lane` of the wave's MFMA tile (ti, tj)
LL_RDM_HD constexpr int pauli_rdm_tiled_entry_row(int wave, int ti, int lane, int reg) {
  return pauli_rdm_tiled_wave_row0(wave) + 16 * ti + pauli_mfma_f64_cd_row(lane, reg);
}
LL_RDM_HD constexpr int pauli_rdm_tiled_entry_col(int wave, int tj, int lane) {
  return pauli_rdm_tiled_wave_col0(wave) + 16 * tj + pauli_mfma_f64_cd_col(lane);
}

// ---- bit deposit and extract through a mask: bit j of v <-> the j-th lowest set bit of mask
LL_RDM_HD inline uint32_t pauli_rdm_tiled_pdep(uint32_t v, uint32_t mask) {
  uint32_t out = 0;
  for (uint32_t bit = 1; mask != 0; bit <<= 1) {
    const uint32_t low = mask & (0u - mask);
    if (v & bit) out |= low;
    mask ^= low;
  }
  return out;
}
LL_RDM_HD inline uint32_t pauli_rdm_tiled_pext(uint32_t v, uint32_t mask) {
  uint32_t out = 0;
  for (uint32_t bit = 1; mask != 0; bit <<= 1) {
    const uint32_t low = mask & (0u - mask);
    if (v & low) out |= bit;
    mask ^= low;
  }
  return out;
}

// ---- the geometry a kernel receives
struct PauliRdmTiledGeom {
  int32_t n_sites, m;
  int32_t rb, bb;        // row bits min(m, 6), block bits m - rb
  int32_t kc_log, kb;    // log2 KC; the environment bits a K-step really walks, min(kc_log, n_sites - m)
  uint8_t all_bit[kPauliRdmTiledMaxSites];    // the sites, ascending: internal bit k (the environment mask's holes)
  uint32_t int_bit[kPauliRdmTiledMaxSites];   // bit k of the CALLER's index -> its bit of the internal index
  uint32_t row_mask, block_mask;              // the row sites, the block sites (as bits of a state)
  uint32_t env_low_mask;                      // where the low kb bits of e lie in a state
};

// sites must have passed pauli_rdm_tiled_check_sites; kc a power of two in [kPauliRdmTiledMinKc, kPauliRdmTiledMaxKc]
inline PauliRdmTiledGeom pauli_rdm_tiled_geom(int n_sites, int m, const int32_t* sites, int kc) {
  PauliRdmTiledGeom g{};
  g.n_sites = n_sites;
  g.m = m;
  g.rb = m < kPauliRdmTiledRowBits ? m : kPauliRdmTiledRowBits;
  g.bb = m - g.rb;
  for (g.kc_log = 0; (1 << (g.kc_log + 1)) <= kc;) ++g.kc_log;
  g.kb = g.kc_log < n_sites - m ? g.kc_log : n_sites - m;
  uint32_t sub = 0;
  for (int k = 0; k < m; ++k) sub |= 1u << sites[k];
  int rank = 0;
  for (int s = 0; s < n_sites; ++s) {
    if (!((sub >> s) & 1u)) continue;
    g.all_bit[rank] = (uint8_t)s;
    (rank < g.rb ? g.row_mask : g.block_mask) |= 1u << s;
    ++rank;
  }
  for (int k = 0; k < m; ++k) {
    int r = 0;
    for (int j = 0; j < m; ++j) r += sites[j] < sites[k];
    g.int_bit[k] = 1u << r;
  }
  g.env_low_mask = pauli_rdm_insert_zeros((1u << g.kb) - 1u, g.all_bit, m);
  return g;
}

// KC: forced (> 0: the key pauli_rdm_tiled_kc, lowered to a power of two inside the range the kernels are built for) or the default
inline int pauli_rdm_tiled_kc(int forced) {
  if (forced <= 0) return kPauliRdmTiledDefaultKc;
  int kc = kPauliRdmTiledMinKc;
  while (2 * kc <= forced && 2 * kc <= kPauliRdmTiledMaxKc) kc *= 2;
  return kc;
}
inline int64_t pauli_rdm_tiled_blocks_per_side(const PauliRdmTiledGeom& g) { return (int64_t)1 << g.bb; }
inline int64_t pauli_rdm_tiled_tiles(const PauliRdmTiledGeom& g) {
  const int64_t nb = pauli_rdm_tiled_blocks_per_side(g);
  return nb * (nb + 1) / 2;
}
inline int64_t pauli_rdm_tiled_ksteps(const PauliRdmTiledGeom& g) { return (int64_t)1 << (g.n_sites - g.m - g.kb); }
// doubles of one (macro-tile, slice): [part][row][column]
LL_RDM_HD constexpr int pauli_rdm_tiled_tile_doubles(bool complex_storage) {
  return kPauliRdmTiledEdge * kPauliRdmTiledEdge * (complex_storage ? 2 : 1);
}
// ksplit: forced (> 0: the key pauli_rdm_tiled_ksplit, lowered to a power of two that divides the K-steps) or the smallest power
// of two with tiles x ksplit >= kPauliRdmTiledFillFactor x cus, while the K-steps allow and the partials stay within
// kPauliRdmTiledSplitBytes (ksplit = 1 always stands: then the partials are the upper triangle of rho itself)
inline int64_t pauli_rdm_tiled_ksplit(const PauliRdmTiledGeom& g, bool complex_storage, int forced, int cus) {
  const int64_t nk = pauli_rdm_tiled_ksteps(g), tiles = pauli_rdm_tiled_tiles(g);
  const int64_t tile_bytes = (int64_t)sizeof(double) * pauli_rdm_tiled_tile_doubles(complex_storage);
  int64_t ks = 1;
  if (forced > 0) {
    while (2 * ks <= forced && 2 * ks <= nk) ks *= 2;
    return ks;
  }
  while (tiles * ks < (int64_t)kPauliRdmTiledFillFactor * cus && 2 * ks <= nk && tiles * 2 * ks * tile_bytes <= kPauliRdmTiledSplitBytes)
    ks *= 2;
  return ks;
}
// where the partial of (slice, tile, part, row, column) lies
LL_RDM_HD inline int64_t pauli_rdm_tiled_partial_index(int64_t tiles, bool complex_storage, int64_t slice, int64_t tile, int part,
                                                       int row, int col) {
  return ((slice * tiles + tile) * (complex_storage ? 2 : 1) + part) * (kPauliRdmTiledEdge * kPauliRdmTiledEdge) +
         row * kPauliRdmTiledEdge + col;
}

// ---- a panel: block `blk` of the rows, K-step `step`
// the state all elements of the panel share: the block's bits and the K-step's high environment bits
LL_RDM_HD inline uint32_t pauli_rdm_tiled_panel_base(const PauliRdmTiledGeom& g, uint32_t blk, uint32_t step) {
  return pauli_rdm_tiled_pdep(blk, g.block_mask) | pauli_rdm_insert_zeros(step << g.kb, g.all_bit, g.m);
}
LL_RDM_HD inline uint32_t pauli_rdm_tiled_panel_elems(const PauliRdmTiledGeom& g) { return 1u << (g.rb + g.kb); }
// element `counter` < panel_elems of a panel: what to OR into the base, ascending in the counter
LL_RDM_HD inline uint32_t pauli_rdm_tiled_panel_offset(const PauliRdmTiledGeom& g, uint32_t counter) {
  return pauli_rdm_tiled_pdep(counter, g.row_mask | g.env_low_mask);
}
LL_RDM_HD inline uint32_t pauli_rdm_tiled_offset_row(const PauliRdmTiledGeom& g, uint32_t offset) {
  return pauli_rdm_tiled_pext(offset, g.row_mask);
}
LL_RDM_HD inline uint32_t pauli_rdm_tiled_offset_k(const PauliRdmTiledGeom& g, uint32_t offset) {
  return pauli_rdm_tiled_pext(offset, g.env_low_mask);
}
// the LDS place of (row, k) in a panel plane: the 16 consecutive rows of an MFMA operand at k and at k + 1 fall into the two
// halves of the 64 banks
LL_RDM_HD constexpr uint32_t pauli_rdm_tiled_lds_index(uint32_t row, uint32_t k) { return k * kPauliRdmTiledLdsStride + row; }

// ---- internal <-> caller order
LL_RDM_HD inline uint32_t pauli_rdm_tiled_internal(const PauliRdmTiledGeom& g, uint32_t a) { return pauli_rdm_deposit(a, g.int_bit, g.m); }
inline uint32_t pauli_rdm_tiled_caller(const PauliRdmTiledGeom& g, uint32_t internal) { return pauli_rdm_extract(internal, g.int_bit, g.m); }
// the state of internal index ia and environment configuration e
inline uint32_t pauli_rdm_tiled_state(const PauliRdmTiledGeom& g, uint32_t ia, uint32_t e) {
  return pauli_rdm_tiled_pdep(ia, g.row_mask | g.block_mask) | pauli_rdm_insert_zeros(e, g.all_bit, g.m);
}

// ---- one S_z sector: a state is admitted iff it has n_down set bits, popcount(a) + popcount(e) = n_down
LL_RDM_HD inline bool pauli_rdm_tiled_admits(int n_down, uint32_t state) { return __builtin_popcount(state) == n_down; }
// a macro-tile whose two blocks share no popcount holds zeros by rule only and is not launched: the rows of block I have
// popcount(I) + [0, row_bits], so the ranges of I and J are disjoint iff the popcounts of I and J differ by more than row_bits
LL_RDM_HD inline bool pauli_rdm_tiled_tile_live(uint32_t bi, uint32_t bj, int row_bits) {
  const int d = __builtin_popcount(bi) - __builtin_popcount(bj);
  return (d < 0 ? -d : d) <= row_bits;
}
// a row a (either order: the popcount is the same) that no environment configuration completes
LL_RDM_HD inline bool pauli_rdm_tiled_row_is_zero(int n_sites, int m, int n_down, uint32_t a) {
  const int rest = n_down - __builtin_popcount(a);
  return rest < 0 || rest > n_sites - m;
}

}  // namespace ll
