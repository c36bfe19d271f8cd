// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) on an indexed basis, for gfx950: the one kernel of the S_z sector
// (pauli_sector.hip), the momentum block of a sector (pauli_momentum.hip), the momentum block of the full space
// (pauli_momentum_full.hip) and the momentum / reflection / spin-inversion block (pauli_symmetric.hip).  Those files hold what
// differs, a Partner policy: where a group's partner of a basis state lies in the basis and with which factor it enters.
//
// With s_i the i-th basis state and the groups, term order, folded i^nY and weights w_g of pauli.hip,
//   y(i) = sum_g [Partner: w_g(s_i) * factor * v(index of the partner of s_i ^ X_g)]
// in ascending mask order, one double fma per group, one rounding to T: per state one fixed chain, the same in the four
// kernels because it is this text.  The same bits run to run and for every block size, grid and alignment.
//
// Geometry: a workgroup takes blocks of 2^b consecutive indices in a grid-stride loop; a lane loads the state, its orbit length
// and x[i] (consecutive lanes, consecutive addresses) and carries kPauliLaneStates of them through the group loop.  The term
// tables are indexed by loop counters only (wave-uniform loads through the scalar cache): they are plain __restrict__ kernel
// parameters for that reason — inside a by-value struct the qualifier is lost and the loads leave the scalar path.  Epilogue:
// pauli_kernel's (deferred normalisation, + offset x, fused partial Re<x, y>).
//
// A Partner is a struct passed by value that holds the tables indexed per lane and supplies
//   states                         the basis states, ascending
//   length(i), dead_length()       the orbit length of state i (0 where the policy has none) and what a lane past the end carries
//   add_group(X, s, ra, live, w, xi, x, dim, acc)
//                                  acc[e] += w[e] * factor * x[partner's index] for the live states whose partner is in the basis
#pragma once
#include <algorithm>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"
#include "pauli_shared.hpp"

namespace ll {

template <typename T, typename Partner>
__global__ __launch_bounds__(kBlock) void pauli_basis_kernel(int b, unsigned nblocks, unsigned dim, int ngroups,
                                                             const uint32_t* __restrict__ gx, const int32_t* __restrict__ gptr,
                                                             const uint32_t* __restrict__ tz, const double* __restrict__ tc,
                                                             Partner pt, const T* __restrict__ x, T* __restrict__ y,
                                                             double offset, double* __restrict__ dot_partials, ScaleIn<T> sc) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn): x holds w, u = sfac * w
  const unsigned bn = 1u << b;
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    // nblocks = ceil(dim / 2^b): base < dim < 2^31; the three policies over representatives rely on dim < 2^27 (creation
    // refuses more: the orbit table packs index << 5, the search needs room above the last index)
    const unsigned base = blk << b;
    const unsigned end = min(bn, dim - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned s[E], ra[E];
      bool live[E];
      T xi[E];
      A acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;
        live[e] = lo < end;
        s[e] = live[e] ? pt.states[base + lo] : 0u;
        ra[e] = live[e] ? pt.length(base + lo) : pt.dead_length();
        xi[e] = live[e] ? x[base + lo] : zero<T>();
        acc[e] = zero<A>();
      }
      for (int g = 0; g < ngroups; ++g) {
        const unsigned X = gx[g];
        A w[E];
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = zero<A>();
        for (int k = gptr[g], k1 = gptr[g + 1]; k < k1; ++k) {
          const unsigned z = tz[k];
          const A c = PauliWeight<A>::load(tc, k, 0u);
#pragma unroll
          for (int e = 0; e < E; ++e) PauliWeight<A>::add(w[e], c, __popc((s[e] ^ X) & z) & 1u);
        }
        pt.add_group(X, s, ra, live, w, xi, x, dim, acc);
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (live[e]) {
          const unsigned i = base + c0 + e * kBlock + threadIdx.x;
          const T us = rmul(sfac, xi[e]);
          const T out = add(narrow<T>(scale_acc(sfac, acc[e])), rmul(offset, us));
          dot_acc += re_cmul(us, out);
          if (sc.u_out) sc.u_out[i] = us;
          y[i] = out;
        }
      }
    }
  }
  if (dot_partials) {
    const double tot = block_sum(dot_acc, red);
    if (threadIdx.x == 0) dot_partials[blockIdx.x] = tot;
  }
}

// b: the indices of a workgroup's block are 2^b (pauli_block_bits); returns the grid = the partials written
template <typename T, typename Partner>
int launch_pauli_basis(int b, int64_t dim, const PauliTermImage& terms, const Partner& pt, const T* x, T* y, double offset,
                       double* dot_partials, hipStream_t s, const ScaleIn<T>* scp) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  const unsigned nblocks = (unsigned)((dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  hipLaunchKernelGGL((pauli_basis_kernel<T, Partner>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, (unsigned)dim, terms.ngroups,
                     terms.gx.get(), terms.gptr.get(), terms.tz.get(), terms.tc.get(), pt, x, y, offset, dot_partials, sc);
  LL_HIP(hipGetLastError());
  return grid;
}

}  // namespace ll
