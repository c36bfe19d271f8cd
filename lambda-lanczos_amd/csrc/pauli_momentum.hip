// The sum of Pauli strings H = sum_t c_t P_t (pauli.hip) on one momentum block of one magnetisation sector of a ring, for gfx950.
// T is the one-site shift (a basis state rotated left by one bit); H conserves total S_z and commutes with T (creation checks
// both: operators.cpp create_pauli_momentum).  The basis of block m (momentum 2 pi m / n_sites) is the representatives r — the
// smallest member of each orbit {T^j s} — of the sector whose orbit length R_r satisfies m R_r = 0 (mod n_sites), ascending;
// basis vector |r; m> = (R_r^(1/2) / n_sites) sum_j e^(-2 pi i m j / n_sites) T^j |r>.
//
// With a the i-th representative, the groups, term order, folded i^nY and weights w_g of pauli_sector.hip:
//   y(i) = sum_g w_g(a) sqrt(R_a / R_b) e^(-2 pi i m l / n_sites) v(index of b),     a ^ X_g = T^l b, b a representative,
// over the groups whose partner a ^ X_g stays in the sector and whose b is in the block, in ascending mask order: per group the
// weight is scaled (only where R_a != R_b: the factor is 1 otherwise), multiplied by the phase (only where m != 0), and enters the
// sum by one double fma; one rounding to T at the end.  Per state one fixed chain: the same bits run to run and for every block
// size, grid and alignment.
//
// Geometry: pauli_sector_kernel's — a workgroup takes blocks of 2^b consecutive indices in a grid-stride loop (b = 8 by default,
// measured against 6 and 10: DESIGN.md 3.1; key pauli_momentum_block_bits); a lane loads reps[i],
// period[i] and x[i] (consecutive lanes, consecutive addresses) and carries kPauliLaneStates of them through the group loop; the
// term tables are indexed by loop counters only (wave-uniform loads).  Per group and state: the partner's sector rank from the two
// rank tables, then ONE 4-byte gather orbit[rank] = (index of b << 5 | l), all ones when the block excludes b's orbit — no
// rotation search in the kernel.  R_b is n_sites unless the partner has a short orbit, which a rotation by n_sites / q for each
// prime q of n_sites tells in registers; only then period[index of b] is gathered (and never when the block holds no short orbit:
// nshort = 0).  ratio[] and phase[] are tables of at most 8 KiB and 480 bytes that stay in cache.
//
// Bytes per apply: (2 sizeof(T) + 5) D_m (x, y, reps, period) when every gather is found in cache, up to
// (2 sizeof(T) + 5) D_m + G (sizeof(T) + 4) D_m when none is (G = groups with X_g != 0: one orbit entry and one element each).
// Epilogue: pauli_kernel's (deferred normalisation, + offset x, fused partial Re<x, y>).
#include <algorithm>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"
#include "pauli_shared.hpp"

namespace ll {

namespace {
struct MomentumTables {
  const uint32_t* __restrict__ reps;
  const uint8_t* __restrict__ period;
  const uint32_t* __restrict__ orbit;
  const uint32_t* __restrict__ lo_rank;
  const uint32_t* __restrict__ hi_rank;
  const double* __restrict__ ratio;
  const double* __restrict__ phase;
  int n_sites, h, momentum, nshort;
  int short_shift[3];
};
}  // namespace

template <typename T>
__global__ __launch_bounds__(kBlock) void pauli_momentum_kernel(int b, unsigned nblocks, unsigned dim, int ngroups,
                                                                const uint32_t* __restrict__ gx, const int32_t* __restrict__ gptr,
                                                                const uint32_t* __restrict__ tz, const double* __restrict__ tc,
                                                                MomentumTables mt, const T* __restrict__ x, T* __restrict__ y,
                                                                double offset, double* __restrict__ dot_partials, ScaleIn<T> sc) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn): x holds w, u = sfac * w
  const unsigned bn = 1u << b, himask = (1u << mt.h) - 1;
  const unsigned L = (unsigned)mt.n_sites, smask = (L >= 32u ? 0u : (1u << L)) - 1u;
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
        ra[e] = live[e] ? (unsigned)mt.period[base + lo] : L;
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
            const unsigned o = mt.orbit[mt.lo_rank[p & himask] + mt.hi_rank[p >> mt.h]];
            if (o != kPauliOrbitExcluded) {  // the partner's orbit is in the block
              const unsigned j = o >> kPauliOrbitShiftBits, l = o & ((1u << kPauliOrbitShiftBits) - 1);
              bool is_short = false;  // T^(L / q) p == p for a prime q of L: the orbit is shorter than L
              for (int q = 0; q < mt.nshort; ++q) {
                const unsigned r = (unsigned)mt.short_shift[q];
                is_short = is_short || (((p << r) | (p >> (L - r))) & smask) == p;
              }
              const unsigned rb = is_short ? (unsigned)mt.period[j] : L;
              A wg = w[e];
              if (rb != ra[e]) wg = momentum_scale(wg, mt.ratio[ra[e] * 32u + rb]);
              if (mt.momentum != 0) wg = momentum_phase(wg, mt.phase[2 * l], mt.phase[2 * l + 1]);
              pauli_fma(acc[e], wg, x[j]);
            }
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
int launch_pauli_momentum(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                          const ScaleIn<T>* scp) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  const PauliMomentumImage& im = op.pauli_momentum;
  // indices per block: the context's pauli_momentum_block_bits, else kPauliMomentumBlockBits (one state per lane)
  const int forced = op.ctx ? op.ctx->tune.pauli_momentum_block_bits : -1;
  const int b = forced >= 0 ? std::min(forced, 30) : kPauliMomentumBlockBits;
  const unsigned dim = (unsigned)im.dim;
  const unsigned nblocks = (unsigned)((im.dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  MomentumTables mt;
  mt.reps = im.reps.get();
  mt.period = im.period.get();
  mt.orbit = im.orbit.get();
  mt.lo_rank = im.lo_rank.get();
  mt.hi_rank = im.hi_rank.get();
  mt.ratio = im.ratio.get();
  mt.phase = im.phase.get();
  mt.n_sites = im.n_sites;
  mt.h = im.h;
  mt.momentum = im.momentum;
  mt.nshort = im.nshort;
  for (int q = 0; q < 3; ++q) mt.short_shift[q] = im.short_shift[q];
  hipLaunchKernelGGL((pauli_momentum_kernel<T>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, dim, im.ngroups, im.gx.get(),
                     im.gptr.get(), im.tz.get(), im.tc.get(), mt, x, y, offset, dot_partials, sc);
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_PAULI_MOMENTUM(T) \
  template int launch_pauli_momentum<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_MOMENTUM)

}  // namespace ll
