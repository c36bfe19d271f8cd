// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) on one momentum block of one magnetisation sector of a ring, for gfx950.
// T is the one-site shift (a basis state rotated left by one bit); H conserves total S_z and commutes with T (creation checks
// both: pauli_operators.cpp create_pauli_momentum).  The basis of block m (momentum 2 pi m / n_sites) is the representatives r — the
// smallest member of each orbit {T^j s} — of the sector whose orbit length R_r satisfies m R_r = 0 (mod n_sites), ascending;
// basis vector |r; m> = (R_r^(1/2) / n_sites) sum_j e^(-2 pi i m j / n_sites) T^j |r>.
//
// With a the i-th representative, the groups, term order, folded i^nY and weights w_g of pauli_sector.hip:
//   y(i) = sum_g w_g(a) sqrt(R_a / R_b) e^(-2 pi i m l / n_sites) v(index of b),     a ^ X_g = T^l b, b a representative,
// over the groups whose partner a ^ X_g stays in the sector and whose b is in the block, in ascending mask order: per group the
// weight is scaled (only where R_a != R_b: the factor is 1 otherwise), multiplied by the phase (only where m != 0), and enters the
// sum by one double fma; one rounding to T at the end.  Per state one fixed chain: the same bits run to run and for every block
// size, grid and alignment.
//
// Geometry, weights and epilogue: pauli_basis_kernel's (pauli_basis.hpp; 2^b indices per block, b = 8 by default, measured
// against 6 and 10: DESIGN.md 3.1; key pauli_momentum_block_bits); a lane loads reps[i], orbit_len[i] and x[i].  Per group and
// state: the partner's sector rank from the two rank tables, then ONE 4-byte gather orbit[rank] = (index of b << 5 | l), all
// ones when the block excludes b's orbit — no rotation search in the kernel.  R_b is n_sites unless the partner has a short
// orbit, which a rotation by n_sites / q for each prime q of n_sites tells in registers; only then orbit_len[index of b] is
// gathered (and never when the block holds no short orbit: nshort = 0).  ratio[] and phase[] are tables of at most 8 KiB and
// 480 bytes that stay in cache.
//
// Bytes per apply: (2 sizeof(T) + 5) D_m (x, y, reps, orbit_len) when every gather is found in cache, up to
// (2 sizeof(T) + 5) D_m + G (sizeof(T) + 4) D_m when none is (G = groups with X_g != 0: one orbit entry and one element each).
#include "pauli_basis.hpp"
#include "pauli_momentum_partner.hpp"  // PauliMomentumPartner: shared with the measuring kernel

namespace ll {

template <typename T>
int launch_pauli_momentum(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                          const ScaleIn<T>* scp) {
  const PauliMomentumImage& im = op.pauli_momentum;
  const PauliMomentumPartner pt = pauli_momentum_partner(im);
  return launch_pauli_basis(pauli_block_bits(op, &Tuning::pauli_momentum_block_bits, kPauliMomentumBlockBits), im.dim, im.terms, pt,
                            x, y, offset, dot_partials, s, scp);
}
#define LL_INST_PAULI_MOMENTUM(T) \
  template int launch_pauli_momentum<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_MOMENTUM)

}  // namespace ll
