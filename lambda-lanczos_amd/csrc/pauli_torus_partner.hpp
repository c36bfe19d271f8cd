// The Partner policy (pauli_basis.hpp) of one translation block of an Lx x Ly torus (ll_internal.hpp PauliBlockImage; the text of
// pauli_torus.hip explains the walk and the search).  Shared by the applying kernel (pauli_torus.hip) and the measuring kernel
// (pauli_expect_block.hip): one definition of where a partner lies and with which factor it enters.
#pragma once
#include "pauli_shared.hpp"

namespace ll {

struct PauliTorusPartner {
  const uint32_t* __restrict__ states;  // reps
  const uint8_t* __restrict__ orbit_len;
  const uint32_t* __restrict__ start;
  const double* __restrict__ ratio;   // [R_a * kPauliTorusRatioStride + |stabiliser of b|] = sqrt(R_a / R_b)
  const double* __restrict__ phase;   // [code a + Lx b] = chi(T_x^a T_y^b) as (re, im)
  int prefix_shift, search_trips;
  unsigned lx, ly;                    // 1 <= lx, ly and lx ly <= 30
  unsigned col0;                      // the bits of the sites (0, y): what T_x wraps around to
  unsigned any_momentum;              // m_x != 0 or m_y != 0: the phase is not 1 everywhere
  __device__ __forceinline__ unsigned length(unsigned i) const { return (unsigned)orbit_len[i]; }
  __device__ __forceinline__ unsigned dead_length() const { return 1u; }
  // one candidate c of the element `code` (a + Lx b): the smallest so far, who reached it first, how many did
  static __device__ __forceinline__ void take(unsigned c, unsigned code, unsigned& rep, unsigned& who, unsigned& cnt) {
    const bool less = c < rep;
    cnt = less ? 1u : cnt + (c == rep ? 1u : 0u);
    who = less ? code : who;
    rep = less ? c : rep;
  }
  // The representatives of the states p = s ^ X: the smallest of the Lx Ly images T_x^a T_y^b p, walked b outer, a inner, the
  // code of the element that reaches it first and how many reach it (the stabiliser's size).  T_x rotates every field of Lx
  // bits left by one (the bit that leaves a field at its top comes back at its bottom), T_y the whole word left by Lx bits; Lx
  // steps of T_x give the row's first image back, so one register per state walks the whole group.
  template <int E>
  __device__ __forceinline__ void locate(const unsigned (&s)[E], unsigned X, unsigned (&rep)[E], unsigned (&who)[E],
                                         unsigned (&cnt)[E]) const {
    const unsigned n = lx * ly, smask = (1u << n) - 1u;  // 1 <= n <= 30
    const unsigned keep = smask & ~col0, top = lx - 1u;
    unsigned cur[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      cur[e] = s[e] ^ X;
      rep[e] = 0xffffffffu;  // above every state (n <= 30)
      who[e] = 0u;
      cnt[e] = 0u;
    }
    unsigned code = 0u;
    for (unsigned b = 0; b < ly; ++b) {
      for (unsigned a = 0; a < lx; ++a, ++code) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          take(cur[e], code, rep[e], who[e], cnt[e]);
          cur[e] = ((cur[e] << 1) & keep) | ((cur[e] >> top) & col0);
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) cur[e] = pauli_rotl(cur[e], lx, n, smask);
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
    const unsigned group_size = lx * ly;
    unsigned rep[E], who[E], cnt[E];
    locate(s, X, rep, who, cnt);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e]) {
        const unsigned j = pauli_bucket_search(states, start, prefix_shift, search_trips, rep[e], dim);
        if (states[j] == rep[e]) {  // b is in the basis
          // p = h^-1 b, h = T_x^a T_y^b the element found: the phase of its inverse T_x^(Lx - a) T_y^(Ly - b)
          const unsigned hb = who[e] / lx, ha = who[e] - hb * lx;
          const unsigned l = (ha == 0u ? 0u : lx - ha) + lx * (hb == 0u ? 0u : ly - hb);
          A wg = w[e];
          if (cnt[e] * ra[e] != group_size) wg = momentum_scale(wg, ratio[ra[e] * kPauliTorusRatioStride + cnt[e]]);
          if (any_momentum != 0u) wg = momentum_phase(wg, phase[2 * l], phase[2 * l + 1]);
          pauli_fma(acc[e], wg, x[j]);
        }
      }
    }
  }
};

inline PauliTorusPartner pauli_torus_partner(const PauliBlockImage& im) {
  unsigned col0 = 0u;
  for (int y = 0; y < im.ly; ++y) col0 |= 1u << (im.lx * y);
  return PauliTorusPartner{im.basis.reps.get(), im.basis.orbit_len.get(), im.basis.start.get(), im.ratio.get(), im.phase.get(),
                           im.basis.prefix_shift, im.basis.search_trips, (unsigned)im.lx, (unsigned)im.ly, col0,
                           (im.momentum != 0 || im.momentum_y != 0) ? 1u : 0u};
}

}  // namespace ll
