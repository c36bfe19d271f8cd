// The Partner policy (pauli_basis.hpp) of one momentum block of an S_z sector (ll_internal.hpp PauliMomentumImage; the text of
// pauli_momentum.hip explains the tables).  Shared by the applying kernel (pauli_momentum.hip) and the measuring kernel
// (pauli_expect_block.hip): one definition of where a partner lies and with which factor it enters.
#pragma once
#include "pauli_shared.hpp"

namespace ll {

struct PauliMomentumPartner {
  const uint32_t* __restrict__ states;  // reps
  const uint8_t* __restrict__ orbit_len;
  const uint32_t* __restrict__ orbit;
  const uint32_t* __restrict__ lo_rank;
  const uint32_t* __restrict__ hi_rank;
  const double* __restrict__ ratio;
  const double* __restrict__ phase;
  int n_sites, h, momentum, nshort;
  int short_shift[3];
  __device__ __forceinline__ unsigned length(unsigned i) const { return (unsigned)orbit_len[i]; }
  __device__ __forceinline__ unsigned dead_length() const { return (unsigned)n_sites; }
  template <typename T, typename A, int E>
  __device__ __forceinline__ void add_group(unsigned X, const unsigned (&s)[E], const unsigned (&ra)[E], const bool (&live)[E],
                                            const A (&w)[E], const T (&)[E], const T* __restrict__ x, unsigned, A (&acc)[E]) const {
    const unsigned px = __popc(X), himask = (1u << h) - 1;
    const unsigned L = (unsigned)n_sites, smask = (L >= 32u ? 0u : (1u << L)) - 1u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e] && 2 * __popc(s[e] & X) == px) {  // the partner has n_down set bits too
        const unsigned p = s[e] ^ X;
        const unsigned o = orbit[lo_rank[p & himask] + hi_rank[p >> h]];
        if (o != kPauliOrbitExcluded) {  // the partner's orbit is in the block
          const unsigned j = o >> kPauliOrbitShiftBits, l = o & ((1u << kPauliOrbitShiftBits) - 1);
          bool is_short = false;  // T^(L / q) p == p for a prime q of L: the orbit is shorter than L
          for (int q = 0; q < nshort; ++q) is_short = is_short || pauli_rotl(p, (unsigned)short_shift[q], L, smask) == p;
          const unsigned rb = is_short ? (unsigned)orbit_len[j] : L;
          A wg = w[e];
          if (rb != ra[e]) wg = momentum_scale(wg, ratio[ra[e] * 32u + rb]);
          if (momentum != 0) wg = momentum_phase(wg, phase[2 * l], phase[2 * l + 1]);
          pauli_fma(acc[e], wg, x[j]);
        }
      }
    }
  }
};

inline PauliMomentumPartner pauli_momentum_partner(const PauliMomentumImage& im) {
  return PauliMomentumPartner{im.reps.get(),  im.orbit_len.get(), im.orbit.get(), im.lo_rank.get(),
                              im.hi_rank.get(), im.ratio.get(),   im.phase.get(), im.n_sites,
                              im.h,             im.momentum,      im.nshort,      {im.short_shift[0], im.short_shift[1], im.short_shift[2]}};
}

}  // namespace ll
