// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) on one momentum block of the FULL 2^n_sites space of a ring, for gfx950:
// the block of pauli_momentum.hip without the magnetisation sector, for an H that commutes with the one-site shift T (a basis
// state rotated left by one bit) but need not conserve S_z — the transverse-field Ising ring, XYZ rings, transverse fields
// (creation checks the commutation: pauli_operators.cpp create_pauli_momentum_full).  The basis of block m (momentum
// 2 pi m / n_sites) is the representatives r — the smallest member of each orbit {T^j s} — of ALL states whose orbit length R_r
// satisfies m R_r = 0 (mod n_sites), ascending; basis vector |r; m> = (R_r^(1/2) / n_sites) sum_j e^(-2 pi i m j / n_sites) T^j |r>.
//
// With a the i-th representative and the groups, term order, folded i^nY and weights w_g of pauli.hip:
//   y(i) = sum_g w_g(a) sqrt(R_a / R_b) e^(-2 pi i m l / n_sites) v(index of b),     a ^ X_g = T^l b, b a representative,
// over EVERY group whose b is in the block, in ascending mask order: per group the weight is scaled (only where R_a != R_b),
// multiplied by the phase (only where m != 0), and enters the sum by one double fma; one rounding to T at the end.  Per state
// one fixed chain: the same bits run to run and for every block size, grid and alignment.
//
// There is no table over the 2^n_sites states (4 * 2^n_sites bytes: 4 GiB at 30 sites for vectors of 3.6e7 elements).  Per
// group and state, in registers: n_sites - 1 rotate / compare steps over the partner p = a ^ X_g give b = the smallest rotation,
// the first shift that reaches it and the period R_b (the first j with T^j p = p) — a loop of fixed length, n_sites is
// wave-uniform, no early exit: about 5 n_sites integer VALU operations per partner.  Then l = (R_b - first) mod R_b, and where
// m R_b = 0 (mod n_sites; one bit of a mask over the divisors of n_sites) the number of b by pauli_bucket_search
// (pauli_shared.hpp): b's bucket holds about 8 representatives on average, search_trips is measured at creation.  A group with
// X_g = 0 (the diagonal) needs none of this: b = a, the element is the lane's own.
//
// Geometry, weights and epilogue: pauli_basis_kernel's (pauli_basis.hpp; 2^b indices per block, b = 8 by default; key
// pauli_momentum_full_block_bits); a lane loads reps[i], orbit_len[i] and x[i].
//
// Bytes per apply: (2 sizeof(T) + 5) D_m (x, y, reps, orbit_len) when every gather is found in cache, up to
// (2 sizeof(T) + 5) D_m + G (sizeof(T) + 8 + 4 search_trips) D_m when none is (G = groups with X_g != 0: one element, two bucket
// bounds and at most search_trips representatives each).
#include "pauli_basis.hpp"
#include "pauli_momentum_full_partner.hpp"  // PauliMomentumFullPartner: shared with the measuring kernel

namespace ll {

template <typename T>
int launch_pauli_momentum_full(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                               const ScaleIn<T>* scp) {
  const PauliBlockImage& im = op.pauli_block;
  const PauliMomentumFullPartner pt = pauli_momentum_full_partner(im);
  return launch_pauli_basis(pauli_block_bits(op, &Tuning::pauli_momentum_full_block_bits, kPauliMomentumFullBlockBits), im.dim,
                            im.terms, pt, x, y, offset, dot_partials, s, scp);
}
#define LL_INST_PAULI_MOMENTUM_FULL(T) \
  template int launch_pauli_momentum_full<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_MOMENTUM_FULL)

}  // namespace ll
