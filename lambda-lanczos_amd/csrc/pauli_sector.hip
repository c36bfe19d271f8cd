// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) restricted to one magnetisation sector for gfx950: the basis is the
// D = C(n_sites, n_down) states with n_down set bits (set bit = sigma_z -1), in ascending integer order, for an H that conserves
// total S_z (creation checks it: pauli_operators.cpp create_pauli_sector).
//
// With s_i the i-th state of the sector and the groups, term order, folded i^nY and weights w_g of pauli.hip,
//   y(i) = sum_g w_g(s_i) v(rank(s_i ^ X_g)),   over the groups whose partner s_i ^ X_g stays in the sector,
// in ascending mask order, one double fma per group, one rounding to T: per state the same chain as pauli_kernel's, from which
// the skipped groups (weight exactly 0 there) drop out.  The same bits run to run and for every block size, grid and alignment.
//
// Geometry, weights and epilogue: pauli_basis_kernel's (pauli_basis.hpp; 2^b indices per block, b = 10 by default: one pass of
// the workgroup; key pauli_sector_block_bits); a lane loads states[i] and x[i].  Per group and state: the partner stays in the
// sector when X_g flips as many set bits as clear ones, 2 popcount(s & X_g) == popcount(X_g); its index is
// lo_rank[partner's low h bits] + hi_rank[the other bits] (two small tables that stay in cache), its value one gathered element.
//
// Bytes per apply: 2 sizeof(T) D + 4 D (x, y, states) when every gathered line is found in cache, up to
// (G + 2) sizeof(T) D + 4 D when none is (G = groups with X_g != 0).
#include "pauli_basis.hpp"
#include "pauli_sector_partner.hpp"

namespace ll {

template <typename T>
int launch_pauli_sector(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                        const ScaleIn<T>* scp) {
  const PauliSectorImage& im = op.pauli_sector;
  return launch_pauli_basis(pauli_block_bits(op, &Tuning::pauli_sector_block_bits, kPauliSectorBlockBits), im.dim, im.terms,
                            pauli_sector_partner(im), x, y, offset, dot_partials, s, scp);
}
#define LL_INST_PAULI_SECTOR(T) \
  template int launch_pauli_sector<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_SECTOR)

}  // namespace ll
