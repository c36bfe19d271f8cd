// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) on one momentum block of the FULL 2^n_sites space of a ring, for gfx950:
// the block of pauli_momentum.hip without the magnetisation sector, for an H that commutes with the one-site shift T (a basis
// state rotated left by one bit) but need not conserve S_z — the transverse-field Ising ring, XYZ rings, transverse fields
// (creation checks the commutation: operators.cpp create_pauli_momentum_full).  The basis of block m (momentum
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
// m R_b = 0 (mod n_sites; one bit of a mask over the divisors of n_sites) the number of b by a search:
// start[b >> prefix_shift] and the entry after it bound b's bucket (about 8 representatives on average), and a branch-free
// binary search in reps[] of search_trips halvings — the count the LARGEST bucket needs, measured at creation and the same for
// every lane; a lane whose bucket is down to one candidate loads nothing more.  A group with X_g = 0 (the diagonal) needs none
// of this: b = a, the element is the lane's own.
//
// Geometry: pauli_momentum_kernel's — a workgroup takes blocks of 2^b consecutive indices in a grid-stride loop (b = 8 by default;
// key pauli_momentum_full_block_bits); a lane loads reps[i], period[i] and x[i] (consecutive lanes, consecutive addresses) and
// carries kPauliLaneStates of them through the group loop; the term tables are indexed by loop counters only (wave-uniform loads).
//
// Bytes per apply: (2 sizeof(T) + 5) D_m (x, y, reps, period) when every gather is found in cache, up to
// (2 sizeof(T) + 5) D_m + G (sizeof(T) + 8 + 4 search_trips) D_m when none is (G = groups with X_g != 0: one element, two bucket
// bounds and at most search_trips representatives each).  Epilogue: pauli_kernel's (deferred normalisation, + offset x, fused
// partial Re<x, y>).
#include <algorithm>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"
#include "pauli_shared.hpp"

namespace ll {

namespace {
struct MomentumFullTables {
  const uint32_t* __restrict__ reps;
  const uint8_t* __restrict__ period;
  const uint32_t* __restrict__ start;
  const double* __restrict__ ratio;
  const double* __restrict__ phase;
  int n_sites, momentum, prefix_shift, search_trips;
  unsigned in_block;  // bit R set: orbits of length R are in the block (m R = 0 mod n_sites)
};
}  // namespace

template <typename T>
__global__ __launch_bounds__(kBlock) void pauli_momentum_full_kernel(int b, unsigned nblocks, unsigned dim, int ngroups,
                                                                     const uint32_t* __restrict__ gx,
                                                                     const int32_t* __restrict__ gptr,
                                                                     const uint32_t* __restrict__ tz, const double* __restrict__ tc,
                                                                     MomentumFullTables mt, const T* __restrict__ x,
                                                                     T* __restrict__ y, double offset,
                                                                     double* __restrict__ dot_partials, ScaleIn<T> sc) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn): x holds w, u = sfac * w
  const unsigned bn = 1u << b;
  const unsigned L = (unsigned)mt.n_sites, smask = (1u << L) - 1u, m = (unsigned)mt.momentum;  // L <= 30
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(dim / 2^b): base < dim < 2^27
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
        s[e] = live[e] ? mt.reps[base + lo] : 0u;
        ra[e] = live[e] ? (unsigned)mt.period[base + lo] : 1u;
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
        if (X == 0u) {  // the diagonal: the partner is the representative itself (R_b = R_a, l = 0)
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (live[e]) pauli_fma(acc[e], w[e], xi[e]);
          continue;
        }
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
            cur[e] = ((cur[e] << 1) | (cur[e] >> (L - 1u))) & smask;
            rb[e] = (cur[e] == p && rb[e] == L) ? j : rb[e];
            const bool less = cur[e] < rep[e];
            rep[e] = less ? cur[e] : rep[e];
            first[e] = less ? j : first[e];
          }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
          if (live[e] && ((mt.in_block >> rb[e]) & 1u) != 0u) {  // the partner's orbit is in the block
            const unsigned q = rep[e] >> mt.prefix_shift;
            unsigned lo = mt.start[q], n = mt.start[q + 1u] - lo;  // b's bucket: reps[lo .. lo + n) holds it
            for (int t = 0; t < mt.search_trips; ++t) {
              const unsigned half = n >> 1;
              if (half != 0u && mt.reps[lo + half] <= rep[e]) lo += half;
              n -= half;
            }
            const unsigned j = min(lo, dim - 1u);
            const unsigned l = first[e] == 0u ? 0u : rb[e] - first[e];  // first < R_b: p = T^(R_b - first) b
            A wg = w[e];
            if (rb[e] != ra[e]) wg = momentum_scale(wg, mt.ratio[ra[e] * 32u + rb[e]]);
            if (m != 0u) wg = momentum_phase(wg, mt.phase[2 * l], mt.phase[2 * l + 1]);
            pauli_fma(acc[e], wg, x[j]);
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
int launch_pauli_momentum_full(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                               const ScaleIn<T>* scp) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  const PauliMomentumFullImage& im = op.pauli_momentum_full;
  // indices per block: the context's pauli_momentum_full_block_bits, else kPauliMomentumFullBlockBits (one state per lane)
  const int forced = op.ctx ? op.ctx->tune.pauli_momentum_full_block_bits : -1;
  const int b = forced >= 0 ? std::min(forced, 30) : kPauliMomentumFullBlockBits;
  const unsigned dim = (unsigned)im.dim;
  const unsigned nblocks = (unsigned)((im.dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  MomentumFullTables mt;
  mt.reps = im.reps.get();
  mt.period = im.period.get();
  mt.start = im.start.get();
  mt.ratio = im.ratio.get();
  mt.phase = im.phase.get();
  mt.n_sites = im.n_sites;
  mt.momentum = im.momentum;
  mt.prefix_shift = im.prefix_shift;
  mt.search_trips = im.search_trips;
  mt.in_block = 0u;
  for (int R = 1; R <= im.n_sites; ++R)
    if (im.n_sites % R == 0 && (im.momentum * R) % im.n_sites == 0) mt.in_block |= 1u << R;
  hipLaunchKernelGGL((pauli_momentum_full_kernel<T>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, dim, im.ngroups, im.gx.get(),
                     im.gptr.get(), im.tz.get(), im.tc.get(), mt, x, y, offset, dot_partials, sc);
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_PAULI_MOMENTUM_FULL(T) \
  template int launch_pauli_momentum_full<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_MOMENTUM_FULL)

}  // namespace ll
