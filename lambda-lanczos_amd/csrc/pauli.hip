// Matrix-free spin-1/2 Hamiltonian H = sum_t c_t P_t (P_t a Pauli string on n_sites spins, c_t real) for gfx950: the README's
// many-body use of the mv_mul plugin (LL:120-126) without a stored matrix.
//
// Basis state s, bit j of s = site j, bit 0 = sigma_z +1.  A term (x, z, c): site j carries X (x bit only), Z (z bit only), Y (both);
//   (H v)(s) = sum_t c_t i^nY_t (-1)^popcount((s ^ x_t) & z_t) v(s ^ x_t),   nY_t = popcount(x_t & z_t).
// Creation (pauli_operators.cpp create_pauli) folds i^nY into the coefficient, groups the terms by x mask (groups by ascending mask, the
// terms of a group in the caller's order), and the kernel forms for every state, in that fixed order and in double,
//   y(s) = sum_g w_g(s) v(s ^ X_g),   w_g(s) = sum_{t in g} coef_t (-1)^popcount((s ^ X_g) & z_t):
// the same bits run to run, for every tile size, grid and alignment of the vectors.
//
// Geometry: a workgroup owns a tile of 2^b consecutive states and stages it in LDS once.  A group with X_g < 2^b permutes the tile
// (partner values from LDS); otherwise the partner is the whole tile (tile ^ (X_g >> b)) in memory, where consecutive lanes read
// consecutive addresses up to a permutation inside an aligned segment: every line fetched is used fully.  The term tables are
// indexed by loop counters only (wave-uniform loads through the scalar cache), and the share of a term's parity that comes from
// the bits of s at or above b is the same for the whole tile: it is folded into the coefficient on the scalar unit, once per
// workgroup and term.  Per lane and term: and, popcount, sign flip, add.
//
// Bytes per apply: 2 sizeof(T) n when every partner tile is found in cache, (G_remote + 2) sizeof(T) n when none is
// (G_remote = groups touching a bit >= b); the term tables are a few hundred bytes.  Epilogue: the lattice kernel's (deferred
// normalisation, + offset x, fused partial Re<x, y>).
#include <algorithm>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"
#include "pauli_shared.hpp"

namespace ll {

// V: consecutive states per 16-byte access (1: element-wise, for vectors that are not 16-byte aligned and tiles shorter than one
// access); the arithmetic per state is the same for every V.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void pauli_kernel(int b, unsigned ntiles, int ngroups, const uint32_t* __restrict__ gx,
                                                       const int32_t* __restrict__ gptr, const uint32_t* __restrict__ tz,
                                                       const double* __restrict__ tc, const T* __restrict__ x, T* __restrict__ y,
                                                       double offset, double* __restrict__ dot_partials, ScaleIn<T> sc) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates / V;  // 16-byte slots per lane
  extern __shared__ double lds_raw[];
  T* const tile = reinterpret_cast<T*>(lds_raw);
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn): the states hold w, u = sfac * w
  const unsigned tn = 1u << b, lomask = tn - 1;
  for (unsigned t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const T* const xt = x + ((long long)t << b);
    __syncthreads();  // the previous tile's readers are done
    for (unsigned lo = threadIdx.x * V; lo < tn; lo += kBlock * V) {
      T r[V];
      pauli_load<T, V>(xt + lo, r);
      pauli_store<T, V>(tile + lo, r);
    }
    __syncthreads();
    for (unsigned c0 = 0; c0 < tn; c0 += kBlock * kPauliLaneStates) {
      unsigned lo[E];
      A acc[E][V];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        lo[e] = c0 + (e * kBlock + threadIdx.x) * V;
#pragma unroll
        for (int v = 0; v < V; ++v) acc[e][v] = zero<A>();
      }
      for (int g = 0; g < ngroups; ++g) {
        const unsigned X = gx[g], Xlo = X & lomask, Xhi = X >> b;
        const unsigned hi_src = t ^ Xhi;  // the partner tile = the bits >= b of the source state
        A w[E][V];
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
          for (int v = 0; v < V; ++v) w[e][v] = zero<A>();
        for (int k = gptr[g], k1 = gptr[g + 1]; k < k1; ++k) {
          const unsigned z = tz[k], zlo = z & lomask;
          const A c = PauliWeight<A>::load(tc, k, __popc(hi_src & (z >> b)) & 1u);  // wave-uniform: the tile's share of the parity
#pragma unroll
          for (int e = 0; e < E; ++e)
#pragma unroll
            for (int v = 0; v < V; ++v) PauliWeight<A>::add(w[e][v], c, __popc(((lo[e] + v) ^ Xlo) & zlo) & 1u);
        }
        const T* const src = Xhi == 0 ? tile : x + ((long long)hi_src << b);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (lo[e] < tn) {
            T p[V];
            pauli_load<T, V>(src + ((lo[e] ^ Xlo) & ~(unsigned)(V - 1)), p);
            pauli_xor_permute<T, V>(p, Xlo & (V - 1));
#pragma unroll
            for (int v = 0; v < V; ++v) pauli_fma(acc[e][v], w[e][v], p[v]);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (lo[e] < tn) {
          T xi[V], us[V], out[V];
          pauli_load<T, V>(tile + lo[e], xi);
#pragma unroll
          for (int v = 0; v < V; ++v) {
            us[v] = rmul(sfac, xi[v]);
            out[v] = add(narrow<T>(scale_acc(sfac, acc[e][v])), rmul(offset, us[v]));
            dot_acc += re_cmul(us[v], out[v]);
          }
          const long long i = ((long long)t << b) + lo[e];
          if (sc.u_out) pauli_store<T, V>(sc.u_out + i, us);
          pauli_store<T, V>(y + i, out);
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
int launch_pauli(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s, const ScaleIn<T>* scp) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  const PauliImage& im = op.pauli;
  const PauliTermImage& tm = im.terms;
  const int b = pauli_tile_bits<T>(op);  // states per tile
  const unsigned ntiles = 1u << (im.n_sites - b);
  const int grid = (int)std::min<unsigned>(ntiles, (unsigned)kMaxGrid);
  const size_t lds = std::max<size_t>((size_t)sizeof(T) << b, 16);
  constexpr int V = (int)(16 / sizeof(T));
  auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool vec = V > 1 && (1 << b) >= V && aligned16(x) && aligned16(y) && aligned16(sc.u_out);
  if (vec)
    hipLaunchKernelGGL((pauli_kernel<T, V>), dim3(grid), dim3(kBlock), lds, s, b, ntiles, tm.ngroups, tm.gx.get(), tm.gptr.get(),
                       tm.tz.get(), tm.tc.get(), x, y, offset, dot_partials, sc);
  else
    hipLaunchKernelGGL((pauli_kernel<T, 1>), dim3(grid), dim3(kBlock), lds, s, b, ntiles, tm.ngroups, tm.gx.get(), tm.gptr.get(),
                       tm.tz.get(), tm.tc.get(), x, y, offset, dot_partials, sc);
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_PAULI(T) \
  template int launch_pauli<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI)

}  // namespace ll
