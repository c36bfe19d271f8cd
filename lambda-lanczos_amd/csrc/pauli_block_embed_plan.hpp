// Host-side planning of ll_pauli_block_expand / ll_pauli_block_project (kernels: pauli_block_embed.hip): which block operator goes
// with which target operator, the two factor tables and the launch geometry.  Plain integers in, plain values out — standard
// headers only, so the rules build with a host compiler and are checked on the CPU in tests/cpp/pauli_block_embed_plan_test.cpp.
//
// B is the isometry of a ring's symmetry block: the row of the state t = g b (b a representative of the block with an orbit of R
// states, g an element of the block's group G) holds chi(g) / sqrt(R) in the column of b; the row of a state whose orbit the block
// excludes is empty.  expand: Psi = B c.  project: c = B^H Psi, and since chi is 1 on the stabiliser of an admitted b,
//   c[a] = (1 / sqrt(R_a)) sum_{t in the orbit of a} conj(chi(g_t)) Psi[t] = (sqrt(R_a) / |G|) sum_{g in G} conj(chi(g)) Psi[g a]:
// the project kernel walks ALL |G| elements in one fixed order and needs neither a search nor a rule for "seen before".
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ll {

// what the compatibility rule looks at: the role an operator can play, its ring and its sector (n_down < 0: all 2^n_sites states)
enum PauliEmbedRole {
  kPauliEmbedOther = 0,         // no Pauli-sum operator, or one that cannot play the role asked for
  kPauliEmbedTargetFull,        // ll_op_create_pauli_*: all 2^n_sites states
  kPauliEmbedTargetSector,      // ll_op_create_pauli_sector_*
  kPauliEmbedBlockMomentum,     // ll_op_create_pauli_momentum_*: a sector block (n_down >= 0 always)
  kPauliEmbedBlockMomentumFull, // ll_op_create_pauli_momentum_full_*: a full-space block
  kPauliEmbedBlockSymmetric     // ll_op_create_pauli_symmetric_*: either, by n_down
};
struct PauliEmbedSide {
  PauliEmbedRole role = kPauliEmbedOther;
  int n_sites = 0, n_down = -1;
  int elem_bytes = 8;
  bool is_complex = false;
};
inline bool pauli_embed_is_block(PauliEmbedRole r) {
  return r == kPauliEmbedBlockMomentum || r == kPauliEmbedBlockMomentumFull || r == kPauliEmbedBlockSymmetric;
}
inline bool pauli_embed_is_target(PauliEmbedRole r) { return r == kPauliEmbedTargetFull || r == kPauliEmbedTargetSector; }
// nullptr when `block` expands into / is projected from the basis of `target`; else the cause, as the refusal words it.  (The
// kinds themselves are refused by the caller, which can name them.)
inline const char* pauli_block_embed_fault(const PauliEmbedSide& block, const PauliEmbedSide& target) {
  if (!pauli_embed_is_block(block.role)) return "the block operator is no symmetry block";
  if (!pauli_embed_is_target(target.role)) return "the target operator is neither a full-space nor an S_z-sector sum of Pauli strings";
  if (block.n_sites != target.n_sites) return "block and target differ in n_sites";
  if (block.is_complex != target.is_complex || block.elem_bytes != target.elem_bytes) return "block and target differ in their storage type";
  const bool sector_block = block.role == kPauliEmbedBlockMomentum || (block.role == kPauliEmbedBlockSymmetric && block.n_down >= 0);
  if (target.role == kPauliEmbedTargetSector) {
    if (!sector_block) return "a full-space block does not fit an S_z-sector target: use a full-space target";
    if (block.n_down != target.n_down) return "block and target differ in n_down";
  }
  return nullptr;  // a full-space target takes every block: the states outside a sector block's sector are rows of zeros
}

constexpr int kPauliEmbedMaxOrbit = 120;  // R <= |G| <= 4 * 30
// expand: factor[R] = 1 / sqrt(R), R = 1 .. 120 ([0] = 0): one sqrt and one division, each correctly rounded
inline std::vector<double> pauli_block_expand_factors() {
  std::vector<double> f((size_t)kPauliEmbedMaxOrbit + 1, 0.0);
  for (int R = 1; R <= kPauliEmbedMaxOrbit; ++R) f[(size_t)R] = 1.0 / std::sqrt((double)R);
  return f;
}
// project: factor[R] = sqrt(R) / |G| for R = 1 .. |G| (0 elsewhere): the sum runs over the |G| elements, |G| / R of which reach
// every state of the orbit
inline std::vector<double> pauli_block_project_factors(int group_size) {
  std::vector<double> f((size_t)kPauliEmbedMaxOrbit + 1, 0.0);
  for (int R = 1; R <= std::min(group_size, kPauliEmbedMaxOrbit); ++R) f[(size_t)R] = std::sqrt((double)R) / (double)group_size;
  return f;
}
inline int pauli_block_group_size(int n_sites, bool reflection, bool flip) { return n_sites * (reflection ? 2 : 1) * (flip ? 2 : 1); }

constexpr int kPauliBlockExpandBlockBits = 10;  // output indices of a workgroup's block: kBlock lanes with four states each
constexpr int kPauliBlockProjectBlockBits = 8;  // representatives of a workgroup's block: one per lane, as the block kernels
struct PauliEmbedLaunch {
  int bits = 0;
  int64_t units = 0;  // blocks of 2^bits indices
  int grid = 0;       // workgroups: each takes ceil or floor of units / grid trips of the grid-stride loop
};
// count indices (expand: the target's n_local, at most 2^30; project: the block's, below 2^27) in blocks of 2^bits: `forced` is
// the tuning key (negative: the default), at most 30
inline PauliEmbedLaunch pauli_block_embed_launch(int64_t count, int forced, int dflt, int max_grid) {
  PauliEmbedLaunch l;
  l.bits = forced >= 0 ? std::min(forced, 30) : dflt;
  l.units = (count + ((int64_t)1 << l.bits) - 1) >> l.bits;
  l.grid = (int)std::min<int64_t>(l.units, (int64_t)max_grid);
  return l;
}

}  // namespace ll
