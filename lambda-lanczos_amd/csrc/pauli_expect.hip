// Expectation values of Pauli strings in one sweep over a state, for gfx950 (ll_pauli_expect, lanczos_hip.h): the kernels read
// psi and write scalars only — no n-sized output vector, many observables per sweep.
//
// An observable (x, z, coef), with the conventions of pauli.hip (P|s> = i^nY (-1)^popcount(s & z) |s ^ x>):
//   out = coef * sum_s Re[ conj(psi(s ^ x)) i^nY (-1)^popcount(s & z) psi(s) ];   nothing is divided by <psi|psi>.
// The plan (pauli_expect_plan.hpp) drops the observables that are identically zero, sorts the rest by x mask and cuts the list into
// batches of at most kPauliExpectBatch slots; one launch = one batch = one sweep over psi.  Per batch, group (run of slots with one
// x mask) and state the partner psi(s ^ x) is loaded once and v = conj(partner) psi(s) formed once, in double (float inputs are
// widened; one product for a real psi, real and imaginary part for a complex one); every slot of the group adds
// +-(Re v or Im v) to its own double accumulator.  A lane keeps the batch's accumulators in registers through the workgroup's
// whole grid-stride loop (the slot loop is unrolled: every accumulator has a fixed register); at the end one block reduction
// per accumulator and one partial per workgroup and accumulator, folded over the workgroups in a fixed order by
// reduce_cols_kernel.  The host multiplies by the folded coefficient.  Which lane sums which states depends on the tile / block
// size alone — not on the alignment of psi, not on where it lives: for a given tile or block size the same bits run to run.
//
// Full space (pauli_expect_kernel): the geometry of pauli_kernel.  A workgroup stages a tile of 2^b consecutive states in LDS
// (key pauli_tile_bits); a group with X < 2^b permutes the tile, otherwise the partner tile (tile ^ (X >> b)) is read from
// memory with the same coalescing.  The share of a slot's parity that comes from the bits at or above b is the same for the
// whole tile and is applied once per slot and pass on the scalar unit.
// Bytes per sweep: between sizeof(T) n (every partner tile found in cache, or all observables diagonal) and
// (1 + G_remote) sizeof(T) n (G_remote = x masks of the batch that touch a bit at or above b).  Sweeps = batches.
//
// Sector (pauli_expect_sector_kernel): the block loop of pauli_basis_kernel (2^b indices per block, key pauli_sector_block_bits)
// with the states and the rank lookup of PauliSectorPartner; a partner outside the sector contributes nothing.
// Bytes per sweep: (sizeof(T) + 4) D up to (1 + G) sizeof(T) D + 4 D (G = x masks of the batch that are not 0: gathered).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 3.5 holds the table; no kernel uses scratch.
#include <cmath>

#include "dev_helpers.hpp"
#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_expect_plan.hpp"
#include "pauli_measure.hpp"
#include "pauli_sector_partner.hpp"
#include "pauli_shared.hpp"

namespace ll {

namespace {
constexpr int kPauliExpectBatch = 32;  // B: accumulators (doubles) a lane carries; chosen from the resource report

// v = conj(p) x in double: one product (real: im stays 0 and is never read), (re, im) (complex).  Plain doubles, no struct: a
// member picked by a run-time flag would turn the products into an indexed array (scratch, or LDS)
template <typename T> inline constexpr bool kExpectComplex = scalar_traits<T>::is_complex;
__device__ __forceinline__ void expect_product(double p, double x, double& re, double&) { re = p * x; }
__device__ __forceinline__ void expect_product(float p, float x, double& re, double&) { re = (double)p * (double)x; }
__device__ __forceinline__ void expect_product(zc p, zc x, double& re, double& im) {
  re = fma(p.re, x.re, p.im * x.im);
  im = fma(p.re, x.im, -(p.im * x.re));
}
__device__ __forceinline__ void expect_product(cf p, cf x, double& re, double& im) { expect_product(to_acc(p), to_acc(x), re, im); }

// one block reduction per accumulator; thread 0 writes partials[workgroup][slot], count slots per row
template <int B>
__device__ __forceinline__ void expect_write_partials(const double (&acc)[B], int count, double* __restrict__ partials, double* red) {
#pragma unroll
  for (int k = 0; k < B; ++k) {
    if (k < count) {  // the same in every lane of the workgroup
      const double tot = block_sum(acc[k], red);
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * count + k] = tot;
    }
  }
}
}  // namespace

// VEC: 16-byte accesses (psi 16-byte aligned and the tile at least one access long); else element-wise.  A lane takes the same
// states either way — kPauliLaneStates / VM runs of VM = 16 / sizeof(T) consecutive states — so the sums are the same bits.
template <typename T, bool VEC, int B>
__global__ __launch_bounds__(kBlock) void pauli_expect_kernel(int b, unsigned ntiles, int count, const uint32_t* __restrict__ sx,
                                                              const uint32_t* __restrict__ sz, const uint32_t* __restrict__ sf,
                                                              const T* __restrict__ x, double* __restrict__ partials) {
  constexpr int VM = (int)(16 / sizeof(T));
  constexpr int E = kPauliLaneStates / VM;
  constexpr int V = VEC ? VM : 1;  // elements per access
  extern __shared__ double lds_raw[];
  T* const tile = reinterpret_cast<T*>(lds_raw);
  __shared__ double red[4];
  double acc[B];
#pragma unroll
  for (int k = 0; k < B; ++k) acc[k] = 0.0;
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
      T xi[E][VM];
      double vre[E][VM], vim[E][VM];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        lo[e] = c0 + (e * kBlock + threadIdx.x) * VM;
        if constexpr (VEC) {  // tn is a multiple of VM: the run is inside the tile or past it
          if (lo[e] < tn) pauli_load<T, VM>(tile + lo[e], xi[e]);
          else
#pragma unroll
            for (int u = 0; u < VM; ++u) xi[e][u] = zero<T>();
        } else {
#pragma unroll
          for (int u = 0; u < VM; ++u) xi[e][u] = lo[e] + u < tn ? tile[lo[e] + u] : zero<T>();
        }
#pragma unroll
        for (int u = 0; u < VM; ++u) vre[e][u] = vim[e][u] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < B; ++k) {
        if (k < count) {  // wave-uniform, as everything read from the slot tables
          const unsigned f = sf[k], z = sz[k];
          if (f & kExpectSlotNewGroup) {
            const unsigned X = sx[k], Xlo = X & lomask, Xhi = X >> b;
            const T* const src = Xhi == 0 ? tile : x + ((long long)(t ^ Xhi) << b);  // the partner tile
#pragma unroll
            for (int e = 0; e < E; ++e) {
              if constexpr (VEC) {
                if (lo[e] < tn) {
                  T p[VM];
                  pauli_load<T, VM>(src + ((lo[e] ^ Xlo) & ~(unsigned)(VM - 1)), p);
                  pauli_xor_permute<T, VM>(p, Xlo & (VM - 1));
#pragma unroll
                  for (int u = 0; u < VM; ++u) expect_product(p[u], xi[e][u], vre[e][u], vim[e][u]);
                }
              } else {
#pragma unroll
                for (int u = 0; u < VM; ++u)
                  if (lo[e] + u < tn) expect_product(src[(lo[e] + u) ^ Xlo], xi[e][u], vre[e][u], vim[e][u]);
              }
            }
          }
          const unsigned zlo = z & lomask;
          double sum = 0.0;
          if (kExpectComplex<T> && (f & kExpectSlotImag) != 0) {  // wave-uniform: the slot sums Im v
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
              for (int u = 0; u < VM; ++u) sum += pauli_flip_sign(vim[e][u], __popc((lo[e] + u) & zlo) & 1u);
          } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
              for (int u = 0; u < VM; ++u) sum += pauli_flip_sign(vre[e][u], __popc((lo[e] + u) & zlo) & 1u);
          }
          acc[k] += pauli_flip_sign(sum, __popc(t & (z >> b)) & 1u);  // the tile's share of the parity
        }
      }
    }
  }
  expect_write_partials<B>(acc, count, partials, red);
}

template <typename T, int B>
__global__ __launch_bounds__(kBlock) void pauli_expect_sector_kernel(int b, unsigned nblocks, unsigned dim, int count,
                                                                     const uint32_t* __restrict__ sx, const uint32_t* __restrict__ sz,
                                                                     const uint32_t* __restrict__ sf, PauliSectorPartner pt,
                                                                     const T* __restrict__ x, double* __restrict__ partials) {
  constexpr int E = kPauliLaneStates;
  __shared__ double red[4];
  double acc[B];
#pragma unroll
  for (int k = 0; k < B; ++k) acc[k] = 0.0;
  const unsigned bn = 1u << b, himask = (1u << pt.h) - 1;
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(dim / 2^b): base < dim < 2^31
    const unsigned end = min(bn, dim - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned s[E];
      bool live[E];
      T xi[E];
      double vre[E], vim[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;
        live[e] = lo < end;
        s[e] = live[e] ? pt.states[base + lo] : 0u;
        xi[e] = live[e] ? x[base + lo] : zero<T>();
        vre[e] = vim[e] = 0.0;
      }
#pragma unroll
      for (int k = 0; k < B; ++k) {
        if (k < count) {  // wave-uniform
          const unsigned f = sf[k], z = sz[k];
          if (f & kExpectSlotNewGroup) {
            const unsigned X = sx[k], px = __popc(X);
#pragma unroll
            for (int e = 0; e < E; ++e) {
              vre[e] = vim[e] = 0.0;
              if (live[e] && 2 * __popc(s[e] & X) == px)  // the partner stays in the sector
                expect_product(x[pt.rank(s[e] ^ X, himask)], xi[e], vre[e], vim[e]);
            }
          }
          double sum = 0.0;
          if (kExpectComplex<T> && (f & kExpectSlotImag) != 0) {  // wave-uniform: the slot sums Im v
#pragma unroll
            for (int e = 0; e < E; ++e) sum += pauli_flip_sign(vim[e], __popc(s[e] & z) & 1u);
          } else {
#pragma unroll
            for (int e = 0; e < E; ++e) sum += pauli_flip_sign(vre[e], __popc(s[e] & z) & 1u);
          }
          acc[k] += sum;
        }
      }
    }
  }
  expect_write_partials<B>(acc, count, partials, red);
}

namespace {
// one batch on the full space: returns the grid = the rows of partials written
template <typename T>
int launch_pauli_expect(const ll_operator& op, int count, const uint32_t* sx, const uint32_t* sz, const uint32_t* sf, const T* x,
                        double* partials, hipStream_t s) {
  constexpr int B = kPauliExpectBatch;
  const int b = pauli_tile_bits<T>(op);  // the tile of launch_pauli (pauli.hip)
  const unsigned ntiles = 1u << (op.pauli.n_sites - b);
  const int grid = (int)std::min<unsigned>(ntiles, (unsigned)kMaxGrid);
  const size_t lds = std::max<size_t>((size_t)sizeof(T) << b, 16);
  constexpr int VM = (int)(16 / sizeof(T));
  const bool vec = VM > 1 && (1 << b) >= VM && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((pauli_expect_kernel<T, true, B>), dim3(grid), dim3(kBlock), lds, s, b, ntiles, count, sx, sz, sf, x, partials);
  else
    hipLaunchKernelGGL((pauli_expect_kernel<T, false, B>), dim3(grid), dim3(kBlock), lds, s, b, ntiles, count, sx, sz, sf, x, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T>
int launch_pauli_expect_sector(const ll_operator& op, int count, const uint32_t* sx, const uint32_t* sz, const uint32_t* sf,
                               const T* x, double* partials, hipStream_t s) {
  constexpr int B = kPauliExpectBatch;
  const PauliSectorImage& im = op.pauli_sector;
  const int b = pauli_block_bits(op, &Tuning::pauli_sector_block_bits, kPauliSectorBlockBits);
  const unsigned nblocks = (unsigned)((im.dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  hipLaunchKernelGGL((pauli_expect_sector_kernel<T, B>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, (unsigned)im.dim, count, sx, sz,
                     sf, pauli_sector_partner(im), x, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
}  // namespace

template <typename T>
void pauli_expect_run(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs, const void* psi,
                      double* out, int64_t* sweeps_out) {
  constexpr int B = kPauliExpectBatch;
  const bool sector = op->kind == ll_operator::PAULI_SECTOR;
  check_observables(sector ? op->pauli_sector.n_sites : op->pauli.n_sites, n_obs, obs);
  const PauliExpectPlan plan = pauli_expect_plan(scalar_traits<T>::is_complex, sector, n_obs, obs, B);
  for (int64_t j = 0; j < n_obs; ++j) out[j] = 0.0;  // what the identically zero observables keep: +0.0
  const int64_t nslots = plan.nslots();
  if (sweeps_out) *sweeps_out = plan.nbatches();
  if (nslots == 0) return;  // nothing has touched the device

  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<T> staged;
  const T* const x = stage_in(ctx, staged, psi, op->n_local);
  // the slot tables [x | z | flags]
  std::vector<uint32_t> tab((size_t)3 * nslots);
  std::copy(plan.x.begin(), plan.x.end(), tab.begin());
  std::copy(plan.z.begin(), plan.z.end(), tab.begin() + nslots);
  std::copy(plan.flags.begin(), plan.flags.end(), tab.begin() + 2 * nslots);
  DevBuf<uint32_t> dtab;
  dtab.alloc(ctx, tab.size());
  LL_HIP(hipMemcpyAsync(dtab.p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  const std::vector<double> sums = pauli_measure_sweeps(ctx, plan, (size_t)kMaxGrid * B, [&](int64_t k, double* partials) {
    const int count = (int)plan.batch_count(k);
    const uint32_t *sx = dtab.p + plan.batch_begin(k), *sz = sx + nslots, *sf = sz + nslots;
    return sector ? launch_pauli_expect_sector<T>(*op, count, sx, sz, sf, x, partials, s)
                  : launch_pauli_expect<T>(*op, count, sx, sz, sf, x, partials, s);
  });
  for (int64_t i = 0; i < nslots; ++i) out[plan.obs[(size_t)i]] = plan.coef[(size_t)i] * sums[(size_t)i];
}

// what capi.cpp calls: the checks that do not depend on the storage type, then the operator's type
void pauli_expect(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs, const void* psi, double* out,
                  int64_t* sweeps_out) {
  LL_REQUIRE(ctx != nullptr && op != nullptr, "null argument");
  LL_REQUIRE(n_obs >= 0, "n_obs is negative");
  LL_REQUIRE(n_obs == 0 || (obs != nullptr && psi != nullptr && out != nullptr), "null argument");
  pauli_measure_prologue(ctx, "expectation values", {{op, "the operator"}});
  if (op->kind == ll_operator::PAULI_MOMENTUM || op->kind == ll_operator::PAULI_MOMENTUM_FULL || op->kind == ll_operator::PAULI_SYMMETRIC)
    LL_REQUIRE(false, std::string("the operator is ") + operator_kind_name(op->kind) +
                          ": symmetrised observables are not built (an observable must be summed over the block's group first); "
                          "measure on a full-space or S_z-sector operator");
  LL_REQUIRE(op->kind == ll_operator::PAULI || op->kind == ll_operator::PAULI_SECTOR,
             std::string("the operator is ") + operator_kind_name(op->kind) +
                 ": expectation values of Pauli strings need an operator that defines a spin basis (full-space or S_z-sector "
                 "sum of Pauli strings)");
  if (sweeps_out) *sweeps_out = 0;
  if (n_obs == 0) return;
  for_storage_type(*op, [&](auto t) { pauli_expect_run<decltype(t)>(ctx, op, n_obs, obs, psi, out, sweeps_out); });
}

}  // namespace ll
