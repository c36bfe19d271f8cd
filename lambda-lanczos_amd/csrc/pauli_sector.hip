// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) restricted to one magnetisation sector for gfx950: the basis is the
// D = C(n_sites, n_down) states with n_down set bits (set bit = sigma_z -1), in ascending integer order, for an H that conserves
// total S_z (creation checks it: operators.cpp create_pauli_sector).
//
// With s_i the i-th state of the sector and the groups, term order, folded i^nY and weights w_g of pauli.hip,
//   y(i) = sum_g w_g(s_i) v(rank(s_i ^ X_g)),   over the groups whose partner s_i ^ X_g stays in the sector,
// in ascending mask order, one double fma per group, one rounding to T: per state the same chain as pauli_kernel's, from which
// the skipped groups (weight exactly 0 there) drop out.  The same bits run to run and for every block size, grid and alignment.
//
// Geometry: a workgroup takes blocks of 2^b consecutive indices in a grid-stride loop; a lane loads states[i] and x[i]
// (consecutive lanes, consecutive addresses) and carries kPauliLaneStates of them through the group loop.  The term tables are
// indexed by loop counters only (wave-uniform loads through the scalar cache).  Per group and state: the partner stays in the
// sector when X_g flips as many set bits as clear ones, 2 popcount(s & X_g) == popcount(X_g); its index is
// lo_rank[partner's low h bits] + hi_rank[the other bits] (two small tables that stay in cache), its value one gathered element.
//
// Bytes per apply: 2 sizeof(T) D + 4 D (x, y, states) when every gathered line is found in cache, up to
// (G + 2) sizeof(T) D + 4 D when none is (G = groups with X_g != 0).  Epilogue: pauli_kernel's (deferred normalisation,
// + offset x, fused partial Re<x, y>).
#include <algorithm>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"
#include "pauli_shared.hpp"

namespace ll {

template <typename T>
__global__ __launch_bounds__(kBlock) void pauli_sector_kernel(int b, unsigned nblocks, unsigned dim, int ngroups, int h,
                                                              const uint32_t* __restrict__ gx, const int32_t* __restrict__ gptr,
                                                              const uint32_t* __restrict__ tz, const double* __restrict__ tc,
                                                              const uint32_t* __restrict__ states,
                                                              const uint32_t* __restrict__ lo_rank,
                                                              const uint32_t* __restrict__ hi_rank, const T* __restrict__ x,
                                                              T* __restrict__ y, double offset, double* __restrict__ dot_partials,
                                                              ScaleIn<T> sc) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn): x holds w, u = sfac * w
  const unsigned bn = 1u << b, himask = (1u << h) - 1;
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(dim / 2^b): base < dim < 2^31
    const unsigned end = min(bn, dim - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned s[E];
      bool live[E];
      T xi[E];
      A acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;
        live[e] = lo < end;
        s[e] = live[e] ? states[base + lo] : 0u;
        xi[e] = live[e] ? x[base + lo] : zero<T>();
        acc[e] = zero<A>();
      }
      for (int g = 0; g < ngroups; ++g) {
        const unsigned X = gx[g];
        const unsigned px = __popc(X);
        A w[E];
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = zero<A>();
        for (int k = gptr[g], k1 = gptr[g + 1]; k < k1; ++k) {
          const unsigned z = tz[k];
          const A c = PauliWeight<A>::load(tc, k, 0u);
#pragma unroll
          for (int e = 0; e < E; ++e) PauliWeight<A>::add(w[e], c, __popc((s[e] ^ X) & z) & 1u);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (live[e] && 2 * __popc(s[e] & X) == px) {  // the partner has n_down set bits too
            const unsigned p = s[e] ^ X;
            const unsigned j = lo_rank[p & himask] + hi_rank[p >> h];
            pauli_fma(acc[e], w[e], x[j]);
          }
        }
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

template <typename T>
int launch_pauli_sector(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                        const ScaleIn<T>* scp) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  const PauliSectorImage& im = op.pauli_sector;
  // indices per block: the context's pauli_sector_block_bits, else one pass of the workgroup (kBlock lanes, kPauliLaneStates each)
  const int forced = op.ctx ? op.ctx->tune.pauli_sector_block_bits : -1;
  const int b = forced >= 0 ? std::min(forced, 30) : kPauliSectorBlockBits;
  const unsigned dim = (unsigned)im.dim;
  const unsigned nblocks = (unsigned)((im.dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  hipLaunchKernelGGL((pauli_sector_kernel<T>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, dim, im.ngroups, im.h, im.gx.get(),
                     im.gptr.get(), im.tz.get(), im.tc.get(), im.states.get(), im.lo_rank.get(), im.hi_rank.get(), x, y, offset,
                     dot_partials, sc);
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_PAULI_SECTOR(T) \
  template int launch_pauli_sector<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_SECTOR)

}  // namespace ll
