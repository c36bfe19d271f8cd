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

namespace ll {

struct PauliMomentumFullPartner {
  const uint32_t* __restrict__ states;  // reps
  const uint8_t* __restrict__ orbit_len;
  const uint32_t* __restrict__ start;
  const double* __restrict__ ratio;
  const double* __restrict__ phase;
  int n_sites, momentum, prefix_shift, search_trips;
  unsigned in_block;  // bit R set: orbits of length R are in the block (m R = 0 mod n_sites)
  __device__ __forceinline__ unsigned length(unsigned i) const { return (unsigned)orbit_len[i]; }
  __device__ __forceinline__ unsigned dead_length() const { return 1u; }
  template <typename T, typename A, int E>
  __device__ __forceinline__ void add_group(unsigned X, const unsigned (&s)[E], const unsigned (&ra)[E], const bool (&live)[E],
                                            const A (&w)[E], const T (&xi)[E], const T* __restrict__ x, unsigned dim,
                                            A (&acc)[E]) const {
    if (X == 0u) {  // the diagonal: the partner is the representative itself (R_b = R_a, l = 0)
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (live[e]) pauli_fma(acc[e], w[e], xi[e]);
      return;
    }
    const unsigned L = (unsigned)n_sites, smask = (1u << L) - 1u, m = (unsigned)momentum;  // L <= 30
    // the partners' representatives: the smallest of the L rotations, the first shift that reaches it, the period
    unsigned cur[E], rep[E], first[E], rb[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      cur[e] = rep[e] = s[e] ^ X;
      first[e] = 0u;
      rb[e] = L;
    }
    for (unsigned j = 1; j < L; ++j) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned p = s[e] ^ X;
        cur[e] = pauli_rotl(cur[e], 1u, L, smask);
        rb[e] = (cur[e] == p && rb[e] == L) ? j : rb[e];
        const bool less = cur[e] < rep[e];
        rep[e] = less ? cur[e] : rep[e];
        first[e] = less ? j : first[e];
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e] && ((in_block >> rb[e]) & 1u) != 0u) {  // the partner's orbit is in the block: reps[] holds b
        const unsigned j = pauli_bucket_search(states, start, prefix_shift, search_trips, rep[e], dim);
        const unsigned l = first[e] == 0u ? 0u : rb[e] - first[e];  // first < R_b: p = T^(R_b - first) b
        A wg = w[e];
        if (rb[e] != ra[e]) wg = momentum_scale(wg, ratio[ra[e] * 32u + rb[e]]);
        if (m != 0u) wg = momentum_phase(wg, phase[2 * l], phase[2 * l + 1]);
        pauli_fma(acc[e], wg, x[j]);
      }
    }
  }
};

template <typename T>
int launch_pauli_momentum_full(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                               const ScaleIn<T>* scp) {
  const PauliBlockImage& im = op.pauli_block;
  unsigned in_block = 0u;
  for (int R = 1; R <= im.n_sites; ++R)
    if (im.n_sites % R == 0 && (im.momentum * R) % im.n_sites == 0) in_block |= 1u << R;
  const PauliMomentumFullPartner pt{im.basis.reps.get(), im.basis.orbit_len.get(), im.basis.start.get(),
                                    im.ratio.get(),      im.phase.get(),           im.n_sites,
                                    im.momentum,         im.basis.prefix_shift,    im.basis.search_trips,
                                    in_block};
  return launch_pauli_basis(pauli_block_bits(op, &Tuning::pauli_momentum_full_block_bits, kPauliMomentumFullBlockBits), im.dim,
                            im.terms, pt, x, y, offset, dot_partials, s, scp);
}
#define LL_INST_PAULI_MOMENTUM_FULL(T) \
  template int launch_pauli_momentum_full<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_MOMENTUM_FULL)

}  // namespace ll
