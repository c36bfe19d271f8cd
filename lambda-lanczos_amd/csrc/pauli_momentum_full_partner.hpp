// The Partner policy (pauli_basis.hpp) of one momentum block of the full 2^n_sites space (ll_internal.hpp PauliBlockImage; the
// text of pauli_momentum_full.hip explains the search).  Shared by the applying kernel (pauli_momentum_full.hip) and the
// measuring kernel (pauli_expect_block.hip): one definition of where a partner lies and with which factor it enters.
#pragma once
#include "pauli_shared.hpp"

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
  // The representatives of the states p = s ^ X: the smallest of the L rotations, the first shift that reaches it, the period.  The ONE
  // definition of that rule: add_group below and the expanding kernel (pauli_block_embed.hip) call it.
  template <int E>
  __device__ __forceinline__ void locate(const unsigned (&s)[E], unsigned X, unsigned (&rep)[E], unsigned (&first)[E],
                                         unsigned (&rb)[E]) const {
    const unsigned L = (unsigned)n_sites, smask = (1u << L) - 1u;  // L <= 30
    unsigned cur[E];
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
  }
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
    const unsigned m = (unsigned)momentum;
    unsigned rep[E], first[E], rb[E];
    locate(s, X, rep, first, rb);
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

inline PauliMomentumFullPartner pauli_momentum_full_partner(const PauliBlockImage& im) {
  unsigned in_block = 0u;
  for (int R = 1; R <= im.n_sites; ++R)
    if (im.n_sites % R == 0 && (im.momentum * R) % im.n_sites == 0) in_block |= 1u << R;
  return PauliMomentumFullPartner{im.basis.reps.get(), im.basis.orbit_len.get(), im.basis.start.get(),
                                  im.ratio.get(),      im.phase.get(),           im.n_sites,
                                  im.momentum,         im.basis.prefix_shift,    im.basis.search_trips,
                                  in_block};
}

}  // namespace ll
