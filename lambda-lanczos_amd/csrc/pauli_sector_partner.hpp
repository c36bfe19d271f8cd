// The S_z sector's Partner policy (pauli_basis.hpp): the sector's states and the two tables that give a state's index back
// (ll_internal.hpp PauliSectorImage).  Shared by the applying kernel (pauli_sector.hip) and the measuring kernel
// (pauli_expect.hip): one definition of where a partner lies.
#pragma once
#include "pauli_shared.hpp"

namespace ll {

struct PauliSectorPartner {
  const uint32_t* __restrict__ states;
  const uint32_t* __restrict__ lo_rank;
  const uint32_t* __restrict__ hi_rank;
  int h;
  // the index of the sector's state p; himask = 2^h - 1
  __device__ __forceinline__ unsigned rank(unsigned p, unsigned himask) const { return lo_rank[p & himask] + hi_rank[p >> h]; }
  __device__ __forceinline__ unsigned length(unsigned) const { return 0u; }  // no orbits
  __device__ __forceinline__ unsigned dead_length() const { return 0u; }
  template <typename T, typename A, int E>
  __device__ __forceinline__ void add_group(unsigned X, const unsigned (&s)[E], const unsigned (&)[E], const bool (&live)[E],
                                            const A (&w)[E], const T (&)[E], const T* __restrict__ x, unsigned, A (&acc)[E]) const {
    const unsigned px = __popc(X), himask = (1u << h) - 1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e] && 2 * __popc(s[e] & X) == px) {  // the partner has n_down set bits too
        pauli_fma(acc[e], w[e], x[rank(s[e] ^ X, himask)]);
      }
    }
  }
};

inline PauliSectorPartner pauli_sector_partner(const PauliSectorImage& im) {
  return PauliSectorPartner{im.states.get(), im.lo_rank.get(), im.hi_rank.get(), im.h};
}

}  // namespace ll
