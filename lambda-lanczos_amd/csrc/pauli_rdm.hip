// Reduced density matrices of up to six sites in one sweep over a state, for gfx950 (ll_pauli_rdm, lanczos_hip.h): the kernels
// read psi once and write 4^m numbers — no n-sized workspace.
//
//   rho[a][a'] = sum_e psi(a, e) conj psi(a', e),   bit k of a = site sites[k], e = the configuration of the other sites;
// nothing is divided by <psi|psi>.  It is a rank-k update rho += sum_rows f f^H, a row f being the 2^m amplitudes of one
// environment configuration.  The kernels are templated on the storage type and on m; the geometry — which state lies where —
// is planned on the host (pauli_rdm_plan.hpp, CPU-tested) and the kernels call the same functions.
//
// Ownership (plan): rho is cut into R x R blocks (R = 1, 1, 2, 4, 4, 4 for m = 1 .. 6) and the NB blocks of the upper triangle
// (3, 10, 10, 10, 36, 136) are dealt to the 256 lanes: lane tid owns block tid % NB for the row slice tid / NB, S = 256 / NB
// slices (85, 25, 25, 25, 7, 1).  A lane loads the R amplitudes of its block row and the R of its block column from LDS per row,
// widens them to double and adds the R^2 products to register accumulators (complex: re += ar br + ai bi, im += ai br - ar bi,
// one fma per product, 16 complex entries = 32 doubles at m = 4, 5, 6).  After the workgroup's last row the S slices of an entry
// are folded in slice order through LDS and the workgroup writes one row of partials [workgroup][block][i][j][re, im];
// reduce_cols_kernel folds the workgroups in a fixed order.  The host keeps a <= a' and mirrors: rho is Hermitian bit for bit.
// Which lane sums which rows depends on m and the tile / block size alone: the same bits run to run, for every alignment.
//
// Full space (pauli_rdm_kernel): a workgroup walks SUPER-TILES in a grid-stride loop — the 2^h tiles of 2^t consecutive states
// that differ only in the h subsystem sites at or above t — loads them with the coalesced accesses of pauli_load into
// LDS [tile][offset] (2^(t + h) sizeof(T) <= 32 KiB; key pauli_rdm_tile_bits forces t) and runs the super-tile's 2^(t - n_lo) rows
// out of LDS.  Every element of psi is read from memory once.  Bytes per call: sizeof(T) n + 8 P grid (P doubles per workgroup).
//
// Sector (pauli_rdm_sector_kernel): a grid-stride loop over batches of 2^b environment configurations e (key
// pauli_rdm_block_bits; 2^(b + m) sizeof(T) <= 32 KiB).  e admits the a with popcount(a) = p = n_down - popcount(e): those
// C(m, p) amplitudes are gathered through PauliSectorPartner::rank into the LDS row, the others are zero; a configuration with
// p outside [0, m] is skipped, and so is, per row, every lane whose block holds no pair with popcount(a) = popcount(a') = p.
// Bytes per call: sizeof(T) D gathered + the rank tables (two 4-byte look-ups per element, cached) + the partials.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 3.6 holds the table; no kernel uses scratch.
#include <string>

#include "dev_helpers.hpp"
#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_measure.hpp"
#include "pauli_rdm_plan.hpp"
#include "pauli_sector_partner.hpp"
#include "pauli_shared.hpp"

namespace ll {

namespace {
static_assert(kPauliRdmThreads == kBlock, "the thread-to-entry map is made for the workgroup of the kernels");
constexpr int kPauliRdmLdsBytes = kPauliTileBytes;       // a super-tile / a batch of rows
constexpr size_t kPauliRdmPartialBytes = (size_t)8 << 20;  // the partials of one call at most: bounds the grid at m = 5, 6

template <typename T> inline constexpr bool kRdmComplex = scalar_traits<T>::is_complex;

// acc += f conj(g) in double; the products are exact inside the fma, one rounding per addition
__device__ __forceinline__ void rdm_update(double f, double g, double& re, double&) { re = fma(f, g, re); }
__device__ __forceinline__ void rdm_update(zc f, zc g, double& re, double& im) {
  re = fma(f.re, g.re, re);
  re = fma(f.im, g.im, re);
  im = fma(f.im, g.re, im);
  im = fma(-f.re, g.im, im);
}

// what a lane owns
template <int M> struct RdmOwner {
  static constexpr int R = pauli_rdm_block_edge(M), NB = pauli_rdm_blocks(M), S = pauli_rdm_slices(M);
  int blk, slice, bi, bj;
  bool owns;
  __device__ __forceinline__ RdmOwner() {
    blk = (int)threadIdx.x % NB;
    slice = (int)threadIdx.x / NB;
    owns = slice < S;
    const PauliRdmBlock b = pauli_rdm_block_of(pauli_rdm_blocks_per_side(M), blk);
    bi = b.bi;
    bj = b.bj;
  }
};

// the S slices of every entry folded in slice order; lanes of slice 0 write partials[workgroup][block][i][j][part].
// red: kBlock doubles
template <typename T, int M>
__device__ __forceinline__ void rdm_write_partials(const RdmOwner<M>& o, const double (&re)[RdmOwner<M>::R][RdmOwner<M>::R],
                                                   const double (&im)[RdmOwner<M>::R][RdmOwner<M>::R], double* __restrict__ partials,
                                                   double* red) {
  constexpr int R = RdmOwner<M>::R, NB = RdmOwner<M>::NB, S = RdmOwner<M>::S;
  constexpr int NC = kRdmComplex<T> ? 2 : 1;
  double* const mine = partials + (size_t)blockIdx.x * (NB * R * R * NC) + (size_t)o.blk * (R * R * NC);
#pragma unroll
  for (int i = 0; i < R; ++i) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double v = c == 0 ? re[i][j] : im[i][j];
        if constexpr (S == 1) {
          if (o.owns) mine[(i * R + j) * NC + c] = v;
        } else {
          __syncthreads();  // the readers of the part before are done
          red[threadIdx.x] = v;
          __syncthreads();
          if (o.slice == 0) {
            double tot = v;
            for (int s = 1; s < S; ++s) tot += red[o.blk + s * NB];
            mine[(i * R + j) * NC + c] = tot;
          }
        }
      }
    }
  }
}

// one row of 2^M amplitudes at LDS index base | off: the lane's R x R products
template <typename T, int R>
__device__ __forceinline__ void rdm_row(const T* __restrict__ lds, unsigned base, const unsigned (&offa)[R], const unsigned (&offb)[R],
                                        double (&re)[R][R], double (&im)[R][R]) {
  acc_t<T> fa[R], fb[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    fa[i] = to_acc(lds[base | offa[i]]);
    fb[i] = to_acc(lds[base | offb[i]]);
  }
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) rdm_update(fa[i], fb[j], re[i][j], im[i][j]);
}
}  // namespace

// VEC: 16-byte accesses (psi 16-byte aligned and a tile at least one access long); else element-wise.  The copy into LDS is the
// same either way, and so is every sum.
template <typename T, int M, bool VEC>
__global__ __launch_bounds__(kBlock) void pauli_rdm_kernel(PauliRdmGeom g, unsigned nsuper, const T* __restrict__ x,
                                                           double* __restrict__ partials) {
  constexpr int R = RdmOwner<M>::R, S = RdmOwner<M>::S;
  constexpr int V = VEC ? (int)(16 / sizeof(T)) : 1;
  constexpr int U = 4;  // accesses a lane has in flight while a super-tile is loaded
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  T* const lds = reinterpret_cast<T*>(lds_raw);
  __shared__ double red[kBlock];
  const RdmOwner<M> o;
  unsigned offa[R], offb[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    offa[i] = pauli_rdm_deposit((unsigned)(o.bi * R + i), g.lds_bit, M);
    offb[i] = pauli_rdm_deposit((unsigned)(o.bj * R + i), g.lds_bit, M);
  }
  double re[R][R], im[R][R];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) re[i][j] = im[i][j] = 0.0;
  const unsigned tn = 1u << g.t, total = tn << g.h, nrows = 1u << (g.t - g.n_lo);
  for (unsigned u = blockIdx.x; u < nsuper; u += gridDim.x) {
    __syncthreads();  // the previous super-tile's readers are done
    for (unsigned idx0 = threadIdx.x * V; idx0 < total; idx0 += kBlock * V * U) {  // U loads in flight, then their stores
      T r[U][V];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        unsigned idx = idx0 + k * kBlock * V;  // tn is a multiple of V: an access stays in its tile
        idx = idx < total ? idx : idx0;        // past the super-tile: the lane's first access again, not stored
        const unsigned tile = pauli_rdm_tile_number(g, u, idx >> g.t);  // < 2^(n_sites - t)
        pauli_load<T, V>(x + (((long long)tile << g.t) | (idx & (tn - 1))), r[k]);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const unsigned idx = idx0 + k * kBlock * V;
        if (idx < total) pauli_store<T, V>(lds + idx, r[k]);
      }
    }
    __syncthreads();
    if (o.owns)
      for (unsigned r = (unsigned)o.slice; r < nrows; r += S)
        rdm_row<T, R>(lds, pauli_rdm_insert_zeros(r, g.lo_bit, g.n_lo), offa, offb, re, im);
  }
  rdm_write_partials<T, M>(o, re, im, partials, red);
}

template <typename T, int M>
__global__ __launch_bounds__(kBlock) void pauli_rdm_sector_kernel(PauliRdmGeom g, int b, unsigned nbatches, unsigned nenv, int n_down,
                                                                  PauliSectorPartner pt, const T* __restrict__ x,
                                                                  double* __restrict__ partials) {
  constexpr int R = RdmOwner<M>::R, S = RdmOwner<M>::S;
  extern __shared__ __attribute__((aligned(16))) double lds_raw[];
  T* const lds = reinterpret_cast<T*>(lds_raw);
  __shared__ double red[kBlock];
  const RdmOwner<M> o;
  unsigned offa[R], offb[R], live = 0, live_b = 0;  // live: the popcounts p at which the lane's block holds a pair
#pragma unroll
  for (int i = 0; i < R; ++i) {
    offa[i] = (unsigned)(o.bi * R + i);
    offb[i] = (unsigned)(o.bj * R + i);
    live |= 1u << __popc(offa[i]);
    live_b |= 1u << __popc(offb[i]);
  }
  live &= live_b;
  double re[R][R], im[R][R];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) re[i][j] = im[i][j] = 0.0;
  const unsigned himask = (1u << pt.h) - 1;
  for (unsigned bt = blockIdx.x; bt < nbatches; bt += gridDim.x) {
    const unsigned e0 = bt << b;  // nbatches = ceil(nenv / 2^b): e0 < nenv <= 2^29
    const unsigned cnt = min(1u << b, nenv - e0);
    __syncthreads();  // the previous batch's readers are done
    for (unsigned idx = threadIdx.x; idx < (cnt << M); idx += kBlock) {
      const unsigned e = e0 + (idx >> M), a = idx & ((1u << M) - 1);
      T v = zero<T>();
      if ((int)__popc(a) == pauli_rdm_sector_popcount(n_down, e))  // the state has n_down set bits: it is in the sector
        v = x[pt.rank(pauli_rdm_state(g, a, e), himask)];
      lds[idx] = v;
    }
    __syncthreads();
    if (o.owns)
      for (unsigned r = (unsigned)o.slice; r < cnt; r += S) {
        const int p = pauli_rdm_sector_popcount(n_down, e0 + r);
        if (p < 0 || p > M || ((live >> p) & 1u) == 0) continue;  // no a at all, or none in this lane's block
        rdm_row<T, R>(lds, r << M, offa, offb, re, im);
      }
  }
  rdm_write_partials<T, M>(o, re, im, partials, red);
}

namespace {
// the grid: one workgroup per unit of work at most, and partials within kPauliRdmPartialBytes
int rdm_grid(int64_t units, int per_workgroup) {
  const int64_t cap = std::max<int64_t>(1, (int64_t)(kPauliRdmPartialBytes / sizeof(double)) / per_workgroup);
  return (int)std::min<int64_t>(std::min<int64_t>(units, kMaxGrid), cap);
}

template <typename T, int M>
int launch_pauli_rdm(const ll_operator& op, const int32_t* sites, const T* x, double* partials, hipStream_t s) {
  const int n_sites = op.pauli.n_sites;
  const int forced = op.ctx ? op.ctx->tune.pauli_rdm_tile_bits : -1;
  const int t = pauli_rdm_tile_bits(n_sites, M, sites, (int)sizeof(T), forced, kPauliRdmLdsBytes);
  const PauliRdmGeom g = pauli_rdm_geom(n_sites, M, sites, t);
  const int64_t nsuper = pauli_rdm_super_tiles(g);
  const int grid = rdm_grid(nsuper, pauli_rdm_partials(M, kRdmComplex<T>));
  const size_t lds = std::max<size_t>((size_t)sizeof(T) << (g.t + g.h), 16);
  constexpr int VM = (int)(16 / sizeof(T));
  const bool vec = VM > 1 && (1 << t) >= VM && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (vec) hipLaunchKernelGGL((pauli_rdm_kernel<T, M, true>), dim3(grid), dim3(kBlock), lds, s, g, (unsigned)nsuper, x, partials);
  else hipLaunchKernelGGL((pauli_rdm_kernel<T, M, false>), dim3(grid), dim3(kBlock), lds, s, g, (unsigned)nsuper, x, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T, int M>
int launch_pauli_rdm_sector(const ll_operator& op, const int32_t* sites, const T* x, double* partials, hipStream_t s) {
  const PauliSectorImage& im = op.pauli_sector;
  const int forced = op.ctx ? op.ctx->tune.pauli_rdm_block_bits : -1;
  const int b = pauli_rdm_block_bits(im.n_sites, M, (int)sizeof(T), forced, kPauliRdmLdsBytes);
  const PauliRdmGeom g = pauli_rdm_geom(im.n_sites, M, sites, 0);
  const int64_t nenv = (int64_t)1 << (im.n_sites - M);
  const int64_t nbatches = (nenv + ((int64_t)1 << b) - 1) >> b;
  const int grid = rdm_grid(nbatches, pauli_rdm_partials(M, kRdmComplex<T>));
  const size_t lds = std::max<size_t>((size_t)sizeof(T) << (b + M), 16);
  hipLaunchKernelGGL((pauli_rdm_sector_kernel<T, M>), dim3(grid), dim3(kBlock), lds, s, g, b, (unsigned)nbatches, (unsigned)nenv,
                     (int)im.n_down, pauli_sector_partner(im), x, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T, int M>
int launch_pauli_rdm_any(const ll_operator& op, const int32_t* sites, const T* x, double* partials, hipStream_t s) {
  return op.kind == ll_operator::PAULI_SECTOR ? launch_pauli_rdm_sector<T, M>(op, sites, x, partials, s)
                                              : launch_pauli_rdm<T, M>(op, sites, x, partials, s);
}
}  // namespace

template <typename T>
void pauli_rdm_run(ll_context* ctx, const ll_operator* op, int m, const int32_t* sites, const void* psi, double* out,
                   int64_t* sweeps_out) {
  constexpr bool cplx = kRdmComplex<T>;
  const bool sector = op->kind == ll_operator::PAULI_SECTOR;
  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<T> staged;
  const T* const x = stage_in(ctx, staged, psi, op->n_local);
  // one batch: the 4^m numbers of the upper triangle are its slots
  const int count = pauli_rdm_partials(m, cplx);
  const std::vector<double> host =
      pauli_measure_sweeps(ctx, PauliBatches{count, count}, (size_t)rdm_grid(kMaxGrid, count) * count, [&](int64_t, double* partials) {
        switch (m) {
          case 1: return launch_pauli_rdm_any<T, 1>(*op, sites, x, partials, s);
          case 2: return launch_pauli_rdm_any<T, 2>(*op, sites, x, partials, s);
          case 3: return launch_pauli_rdm_any<T, 3>(*op, sites, x, partials, s);
          case 4: return launch_pauli_rdm_any<T, 4>(*op, sites, x, partials, s);
          case 5: return launch_pauli_rdm_any<T, 5>(*op, sites, x, partials, s);
          default: return launch_pauli_rdm_any<T, 6>(*op, sites, x, partials, s);
        }
      });
  if (sweeps_out) *sweeps_out = 1;
  // the upper triangle, mirrored: out[a'][a] = conj(out[a][a']) with every zero imaginary part +0.0
  const int dim = 1 << m;
  for (int a = 0; a < dim; ++a) {
    for (int ap = a; ap < dim; ++ap) {
      const int i = pauli_rdm_partial_index(m, cplx, a, ap);
      double re = host[(size_t)i], im = (cplx && ap != a) ? host[(size_t)i + 1] : 0.0;
      if (sector && __builtin_popcount((unsigned)a) != __builtin_popcount((unsigned)ap)) re = im = 0.0;  // by rule
      double* const up = out + 2 * ((size_t)a * dim + ap);
      double* const low = out + 2 * ((size_t)ap * dim + a);
      low[0] = re;
      low[1] = 0.0 - im;
      up[0] = re;
      up[1] = im;
    }
  }
}

// what capi.cpp calls: the checks, all before the device is touched, then the operator's type
void pauli_rdm(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites, const void* psi, double* out,
               int64_t* sweeps_out) {
  LL_REQUIRE(ctx != nullptr && op != nullptr && sites != nullptr && psi != nullptr && out != nullptr, "null argument");
  pauli_measure_prologue(ctx, "reduced density matrices", {{op, "the operator"}});
  if (op->kind == ll_operator::PAULI_MOMENTUM || op->kind == ll_operator::PAULI_MOMENTUM_FULL || op->kind == ll_operator::PAULI_SYMMETRIC)
    LL_REQUIRE(false, std::string("the operator is ") + operator_kind_name(op->kind) +
                          ": reduced density matrices of symmetry blocks are not built (a site is not a tensor factor of the "
                          "block's basis); measure on a full-space or S_z-sector operator");
  LL_REQUIRE(op->kind == ll_operator::PAULI || op->kind == ll_operator::PAULI_SECTOR,
             std::string("the operator is ") + operator_kind_name(op->kind) +
                 ": a reduced density matrix needs an operator that defines a spin basis (full-space or S_z-sector sum of Pauli "
                 "strings)");
  const int n_sites = op->kind == ll_operator::PAULI_SECTOR ? op->pauli_sector.n_sites : op->pauli.n_sites;
  int which = -1;
  const PauliRdmSiteError err = pauli_rdm_check_sites(n_sites, n_sub, sites, &which);
  LL_REQUIRE(err != kRdmBadCount, "n_sub = " + std::to_string(n_sub) + ": the subsystem holds 1 to min(6, n_sites = " +
                                      std::to_string(n_sites) + ") sites");
  LL_REQUIRE(err != kRdmSiteOutOfRange, "site " + std::to_string(which) + " of the list (" +
                                            std::to_string(which >= 0 ? sites[which] : 0) + ") is outside [0, n_sites = " +
                                            std::to_string(n_sites) + ")");
  LL_REQUIRE(err != kRdmSiteRepeated, "site " + std::to_string(which) + " of the list (" +
                                          std::to_string(which >= 0 ? sites[which] : 0) + ") is repeated");
  for_storage_type(*op, [&](auto t) { pauli_rdm_run<decltype(t)>(ctx, op, n_sub, sites, psi, out, sweeps_out); });
}

}  // namespace ll
