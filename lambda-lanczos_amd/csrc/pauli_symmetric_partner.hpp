// The Partner policy (pauli_basis.hpp) of one block of a ring under momentum, reflection and spin inversion (ll_internal.hpp
// PauliBlockImage; the text of pauli_symmetric.hip explains the streams and the search).  Shared by the applying kernel
// (pauli_symmetric.hip) and the measuring kernel (pauli_expect_block.hip): one definition of where a partner lies and with which
// factor it enters.
#pragma once
#include "pauli_shared.hpp"

namespace ll {

struct PauliSymmetricPartner {
  const uint32_t* __restrict__ states;  // reps
  const uint8_t* __restrict__ orbit_len;
  const uint32_t* __restrict__ start;
  const double* __restrict__ ratio;   // [R_a * kPauliSymmetricRatioStride + |stabiliser of b|] = sqrt(R_a / R_b)
  const double* __restrict__ phase;
  int n_sites, momentum, prefix_shift, search_trips;
  unsigned group_size;                // |G|
  unsigned use_parity, use_inversion; // the streams in use
  unsigned neg_parity, neg_inversion; // the flag carries a factor -1
  __device__ __forceinline__ unsigned length(unsigned i) const { return (unsigned)orbit_len[i]; }
  __device__ __forceinline__ unsigned dead_length() const { return 1u; }
  // one candidate c of the element `code` (shift | rho << 5 | zeta << 6): the smallest so far, who reached it first, how many did
  static __device__ __forceinline__ void take(unsigned c, unsigned code, unsigned& rep, unsigned& who, unsigned& cnt) {
    const bool less = c < rep;
    cnt = less ? 1u : cnt + (c == rep ? 1u : 0u);
    who = less ? code : who;
    rep = less ? c : rep;
  }
  // The representatives of the states p = s ^ X: the smallest of the |G| images, the element that reaches it first (its code), how many
  // reach it (the stabiliser's size).  The ONE definition of that rule: add_group below and the expanding kernel
  // (pauli_block_embed.hip) call it.
  template <int E>
  __device__ __forceinline__ void locate(const unsigned (&s)[E], unsigned X, unsigned (&rep)[E], unsigned (&who)[E],
                                         unsigned (&cnt)[E]) const {
    const unsigned L = (unsigned)n_sites, smask = (1u << L) - 1u;  // 1 <= L <= 30
    const bool use_p = use_parity != 0u, use_z = use_inversion != 0u;
    unsigned cur[E], rev[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      cur[e] = s[e] ^ X;
      rev[e] = __brev(cur[e]) >> (32u - L);
      rep[e] = 0xffffffffu;  // above every state (L <= 30)
      who[e] = 0u;
      cnt[e] = 0u;
    }
    for (unsigned j = 0; j < L; ++j) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        take(cur[e], j, rep[e], who[e], cnt[e]);
        if (use_z) take(cur[e] ^ smask, j | 64u, rep[e], who[e], cnt[e]);
        if (use_p) {
          take(rev[e], j | 32u, rep[e], who[e], cnt[e]);
          if (use_z) take(rev[e] ^ smask, j | 96u, rep[e], who[e], cnt[e]);
          rev[e] = pauli_rotl(rev[e], 1u, L, smask);
        }
        cur[e] = pauli_rotl(cur[e], 1u, L, smask);
      }
    }
  }
  template <typename T, typename A, int E>
  __device__ __forceinline__ void add_group(unsigned X, const unsigned (&s)[E], const unsigned (&ra)[E], const bool (&live)[E],
                                            const A (&w)[E], const T (&xi)[E], const T* __restrict__ x, unsigned dim,
                                            A (&acc)[E]) const {
    if (X == 0u) {  // the diagonal: the partner is the representative itself (R_b = R_a, the identity element)
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (live[e]) pauli_fma(acc[e], w[e], xi[e]);
      return;
    }
    const unsigned L = (unsigned)n_sites, m = (unsigned)momentum;  // 1 <= L <= 30
    const bool use_p = use_parity != 0u, use_z = use_inversion != 0u;
    unsigned rep[E], who[E], cnt[E];
    locate(s, X, rep, who, cnt);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e]) {
        const unsigned j = pauli_bucket_search(states, start, prefix_shift, search_trips, rep[e], dim);
        if (states[j] == rep[e]) {  // b is in the basis
          const unsigned first = who[e] & 31u;
          const unsigned l = first == 0u ? 0u : L - first;  // p = h^-1 b, h = T^first P^rho Z^zeta: the phase of T^(L - first)
          const unsigned flip = ((who[e] >> 5) & neg_parity) ^ ((who[e] >> 6) & neg_inversion);
          A wg = w[e];
          if (cnt[e] * ra[e] != group_size) wg = momentum_scale(wg, ratio[ra[e] * kPauliSymmetricRatioStride + cnt[e]]);
          if (m != 0u) wg = momentum_phase(wg, phase[2 * l], phase[2 * l + 1]);
          if (use_p || use_z) wg = pauli_flip_sign(wg, flip);
          pauli_fma(acc[e], wg, x[j]);
        }
      }
    }
  }
};

inline PauliSymmetricPartner pauli_symmetric_partner(const PauliBlockImage& im) {
  return PauliSymmetricPartner{im.basis.reps.get(),   im.basis.orbit_len.get(),   im.basis.start.get(),
                               im.ratio.get(),        im.phase.get(),             im.n_sites,
                               im.momentum,           im.basis.prefix_shift,      im.basis.search_trips,
                               (unsigned)im.group_size, im.parity != 0 ? 1u : 0u, im.inversion != 0 ? 1u : 0u,
                               im.parity < 0 ? 1u : 0u, im.inversion < 0 ? 1u : 0u};
}

}  // namespace ll
