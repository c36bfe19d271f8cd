// Reduced density matrices of 4 to 13 sites on the f64 matrix cores of gfx950 (ll_pauli_rdm_tiled, lanczos_hip.h):
//
//   rho[a][a'] = sum_e psi(a, e) conj psi(a', e)   is the Hermitian rank-K update rho = F F^H,
// F the 2^m x 2^(n - m) matrix of fibres.  The geometry — the internal row order, the macro-tiles, which state a lane loads and
// which entry a lane's accumulator register holds — is planned on the host (pauli_rdm_tiled_plan.hpp, CPU-tested) and the
// kernels index through the same functions.
//
// pauli_rdm_tiled_kernel<T, Sector, KC>: one workgroup of 256 lanes per (macro-tile of 64 x 64, slice of K).  Per K-step the
// workgroup stages KC environment configurations of the 64 rows of the row block, and of the column block unless it is the same,
// into LDS as doubles (floats widened on load), real and imaginary parts in separate planes [k][row] of stride 80 doubles: the
// 16 consecutive rows that an MFMA operand reads at k and at k + 1 fall into the two halves of the 64 banks, so a ds_read_b64
// of a wave is conflict-free.  The values of the NEXT K-step are loaded from memory into registers before this step's MFMAs
// and stored to LDS after them: the loads are in flight while the matrix cores run.  Wave w owns the quadrant (w >> 1, w & 1),
// 2 x 2 tiles of v_mfma_f64_16x16x4_f64: 16 accumulator doubles per lane for real storage, 32 for complex, where an entry takes
// four MFMAs per k-step of 4:  re += Ar Br^T + Ai Bi^T,  im += Ai Br^T + Ar (-Bi)^T, the sign flipped on the operand register.
// A sector differs in the loader alone: a state with n_down set bits is fetched through PauliSectorPartner::rank, every other
// one is an exact zero with no table read.  No atomics, no inline assembly.
//
// pauli_rdm_tiled_finish_kernel: one lane per entry a <= a' of the CALLER's order; it deposits both indices into the internal
// order, folds the k-slices of the entry in slice order and writes both triangles — the mirror with the same real bits and the
// negated imaginary part, every zero +0.0 — and the zeros by rule of a sector.  For a given (KC, ksplit) the same bits run to
// run, for a host and a device psi and for every alignment.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 3.6.1 holds the table; no kernel uses scratch.
#include <string>
#include <vector>

#include "dev_helpers.hpp"
#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_measure.hpp"
#include "pauli_rdm_tiled_plan.hpp"
#include "pauli_sector_partner.hpp"

namespace ll {

namespace {
typedef double rdm_d4 __attribute__((ext_vector_type(4)));

static_assert(kPauliRdmThreads == kBlock, "four waves per macro-tile");
static_assert(kPauliRdmTiledEdge == 64 && kPauliRdmTiledRowBits == 6, "the quadrant map is made for 64 x 64");

template <typename T> inline constexpr bool kTiledComplex = scalar_traits<T>::is_complex;

__device__ __forceinline__ void tiled_parts(double v, double& re, double&) { re = v; }
__device__ __forceinline__ void tiled_parts(float v, double& re, double&) { re = (double)v; }
__device__ __forceinline__ void tiled_parts(zc v, double& re, double& im) { re = v.re, im = v.im; }
__device__ __forceinline__ void tiled_parts(cf v, double& re, double& im) { re = (double)v.re, im = (double)v.im; }

// what a lane loads of a panel per K-step: NL elements, the same offsets for every block and step
template <int NL> struct TiledLoadMap {
  unsigned off[NL];   // OR into the panel's base state
  unsigned lds[NL];   // index into a panel plane
  bool live[NL];      // the counter is inside the panel (fewer rows at m < 6, fewer columns where 2^(n - m) < KC)
  __device__ __forceinline__ explicit TiledLoadMap(const PauliRdmTiledGeom& g) {
    const unsigned elems = pauli_rdm_tiled_panel_elems(g);
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const unsigned counter = threadIdx.x + (unsigned)i * kBlock;
      live[i] = counter < elems;
      off[i] = pauli_rdm_tiled_panel_offset(g, live[i] ? counter : 0u);
      lds[i] = pauli_rdm_tiled_lds_index(pauli_rdm_tiled_offset_row(g, off[i]), pauli_rdm_tiled_offset_k(g, off[i]));
    }
  }
};

template <typename T, bool Sector, int NL>
__device__ __forceinline__ void tiled_load(const TiledLoadMap<NL>& map, unsigned base, int n_down, const PauliSectorPartner& pt,
                                           unsigned himask, const T* __restrict__ x, T (&r)[NL]) {
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    const unsigned state = base | map.off[i];
    r[i] = T{};
    if constexpr (Sector) {
      if (map.live[i] && pauli_rdm_tiled_admits(n_down, state)) r[i] = x[pt.rank(state, himask)];
    } else {
      if (map.live[i]) r[i] = x[state];
    }
  }
}
template <typename T, int NL>
__device__ __forceinline__ void tiled_store(const TiledLoadMap<NL>& map, const T (&r)[NL], double* re_plane, double* im_plane) {
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    if (!map.live[i]) continue;
    double re = 0.0, im = 0.0;
    tiled_parts(r[i], re, im);
    re_plane[map.lds[i]] = re;
    if constexpr (kTiledComplex<T>) im_plane[map.lds[i]] = im;
  }
}
}  // namespace

template <typename T, bool Sector, int KC>
__global__ __launch_bounds__(kBlock) void pauli_rdm_tiled_kernel(PauliRdmTiledGeom g, unsigned ksplit, unsigned steps_per_slice,
                                                                 unsigned tiles, int n_down, PauliSectorPartner pt,
                                                                 const uint32_t* __restrict__ tile_list, const T* __restrict__ x,
                                                                 double* __restrict__ partials) {
  constexpr bool CX = kTiledComplex<T>;
  constexpr int NP = CX ? 2 : 1;
  constexpr int NL = (kPauliRdmTiledEdge * KC) / kBlock;  // elements of a panel per lane
  constexpr int PLANE = KC * kPauliRdmTiledLdsStride;
  static_assert(NL >= 1 && KC % 4 == 0, "a K-step is at least one element per lane and whole MFMA steps");
  __shared__ double lds[2 * NP * PLANE];  // [panel A, B][re, im][k][row]
  const unsigned launched = blockIdx.x / ksplit, slice = blockIdx.x % ksplit;
  const unsigned tile = tile_list ? tile_list[launched] : launched;
  const PauliRdmBlock blk = pauli_rdm_block_of(1 << g.bb, (int)tile);
  const bool diagonal = blk.bi == blk.bj;
  double* const a_re = lds;
  double* const a_im = lds + (NP - 1) * PLANE;
  double* const b_re = diagonal ? a_re : lds + NP * PLANE;
  double* const b_im = diagonal ? a_im : lds + (2 * NP - 1) * PLANE;
  for (int i = (int)threadIdx.x; i < 2 * NP * PLANE; i += kBlock) lds[i] = 0.0;  // the padding rows and columns stay zero
  const TiledLoadMap<NL> map(g);
  const unsigned himask = Sector ? (1u << pt.h) - 1u : 0u;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const bool wave_live = pauli_rdm_tiled_wave_live(diagonal, wave);
  const unsigned row_a = (unsigned)(pauli_rdm_tiled_wave_row0(wave) + pauli_mfma_f64_ab_row(lane));
  const unsigned row_b = (unsigned)(pauli_rdm_tiled_wave_col0(wave) + pauli_mfma_f64_ab_row(lane));
  rdm_d4 c_re[2][2], c_im[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) c_re[ti][tj] = c_im[ti][tj] = rdm_d4{0.0, 0.0, 0.0, 0.0};

  const unsigned step0 = slice * steps_per_slice;
  T ra[NL], rb[NL];
  tiled_load<T, Sector, NL>(map, pauli_rdm_tiled_panel_base(g, (unsigned)blk.bi, step0), n_down, pt, himask, x, ra);
  if (!diagonal) tiled_load<T, Sector, NL>(map, pauli_rdm_tiled_panel_base(g, (unsigned)blk.bj, step0), n_down, pt, himask, x, rb);
  for (unsigned st = 0; st < steps_per_slice; ++st) {
    __syncthreads();  // the step before is read (the first time: the zeros are written)
    tiled_store<T, NL>(map, ra, a_re, a_im);
    if (!diagonal) tiled_store<T, NL>(map, rb, b_re, b_im);
    __syncthreads();
    if (st + 1 < steps_per_slice) {  // the next step's values travel while this one's MFMAs run
      tiled_load<T, Sector, NL>(map, pauli_rdm_tiled_panel_base(g, (unsigned)blk.bi, step0 + st + 1), n_down, pt, himask, x, ra);
      if (!diagonal)
        tiled_load<T, Sector, NL>(map, pauli_rdm_tiled_panel_base(g, (unsigned)blk.bj, step0 + st + 1), n_down, pt, himask, x, rb);
    }
    if (wave_live) {
#pragma unroll
      for (int kk = 0; kk < KC / 4; ++kk) {
        const unsigned k = (unsigned)(kk * 4 + pauli_mfma_f64_ab_k(lane));
        double ar[2], ai[2], br[2], bi[2], nbi[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          ar[t] = a_re[pauli_rdm_tiled_lds_index(row_a + 16u * t, k)];
          br[t] = b_re[pauli_rdm_tiled_lds_index(row_b + 16u * t, k)];
          if constexpr (CX) {
            ai[t] = a_im[pauli_rdm_tiled_lds_index(row_a + 16u * t, k)];
            bi[t] = b_im[pauli_rdm_tiled_lds_index(row_b + 16u * t, k)];
            nbi[t] = -bi[t];
          }
        }
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj) {
            c_re[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[ti], br[tj], c_re[ti][tj], 0, 0, 0);
            if constexpr (CX) {
              c_re[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[ti], bi[tj], c_re[ti][tj], 0, 0, 0);
              c_im[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[ti], br[tj], c_im[ti][tj], 0, 0, 0);
              c_im[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[ti], nbi[tj], c_im[ti][tj], 0, 0, 0);
            }
          }
      }
    }
  }
  if (!wave_live) return;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = pauli_rdm_tiled_entry_row(wave, ti, lane, reg), col = pauli_rdm_tiled_entry_col(wave, tj, lane);
        partials[pauli_rdm_tiled_partial_index(tiles, CX, slice, tile, 0, row, col)] = c_re[ti][tj][reg];
        if constexpr (CX) partials[pauli_rdm_tiled_partial_index(tiles, CX, slice, tile, 1, row, col)] = c_im[ti][tj][reg];
      }
}

// out: 2 * 4^m doubles, row-major in the caller's order with interleaved (re, im)
__global__ __launch_bounds__(kBlock) void pauli_rdm_tiled_finish_kernel(PauliRdmTiledGeom g, unsigned ksplit, unsigned tiles,
                                                                        bool complex_storage, bool sector, int n_down,
                                                                        const double* __restrict__ partials,
                                                                        double* __restrict__ out) {
  const unsigned long long idx = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  const unsigned dim = 1u << g.m;
  const unsigned a = (unsigned)(idx >> g.m), ap = (unsigned)(idx & (dim - 1u));
  if (a >= dim || a > ap) return;
  double re = 0.0, im = 0.0;
  const bool by_rule = sector && (__popc(a) != __popc(ap) || pauli_rdm_tiled_row_is_zero(g.n_sites, g.m, n_down, a));
  if (!by_rule) {
    unsigned ia = pauli_rdm_tiled_internal(g, a), iap = pauli_rdm_tiled_internal(g, ap);
    const bool swapped = ia > iap;  // the internal order turns the pair round: the entry is the conjugate of the one computed
    if (swapped) {
      const unsigned t = ia;
      ia = iap;
      iap = t;
    }
    const int tile = pauli_rdm_block_number(1 << g.bb, (int)(ia >> kPauliRdmTiledRowBits), (int)(iap >> kPauliRdmTiledRowBits));
    const int row = (int)(ia & (kPauliRdmTiledEdge - 1)), col = (int)(iap & (kPauliRdmTiledEdge - 1));
    re = partials[pauli_rdm_tiled_partial_index(tiles, complex_storage, 0, tile, 0, row, col)];
    for (unsigned s = 1; s < ksplit; ++s) re += partials[pauli_rdm_tiled_partial_index(tiles, complex_storage, s, tile, 0, row, col)];
    if (complex_storage && a != ap) {
      im = partials[pauli_rdm_tiled_partial_index(tiles, complex_storage, 0, tile, 1, row, col)];
      for (unsigned s = 1; s < ksplit; ++s) im += partials[pauli_rdm_tiled_partial_index(tiles, complex_storage, s, tile, 1, row, col)];
      if (swapped) im = 0.0 - im;
    }
    re += 0.0;  // a zero is +0.0
    im += 0.0;
  }
  double* const up = out + 2 * ((size_t)a * dim + ap);
  double* const low = out + 2 * ((size_t)ap * dim + a);
  low[0] = re;
  low[1] = 0.0 - im;
  up[0] = re;
  up[1] = im;
}

namespace {
template <typename T, bool Sector>
void launch_pauli_rdm_tiled(int kc, int64_t grid, const PauliRdmTiledGeom& g, int64_t ksplit, int64_t steps, int64_t tiles, int n_down,
                            const PauliSectorPartner& pt, const uint32_t* tile_list, const T* x, double* partials, hipStream_t s) {
  const dim3 gr((unsigned)grid), bl(kBlock);
  switch (kc) {
    case 4:
      hipLaunchKernelGGL((pauli_rdm_tiled_kernel<T, Sector, 4>), gr, bl, 0, s, g, (unsigned)ksplit, (unsigned)steps, (unsigned)tiles, n_down,
                         pt, tile_list, x, partials);
      break;
    case 8:
      hipLaunchKernelGGL((pauli_rdm_tiled_kernel<T, Sector, 8>), gr, bl, 0, s, g, (unsigned)ksplit, (unsigned)steps, (unsigned)tiles, n_down,
                         pt, tile_list, x, partials);
      break;
    default:
      hipLaunchKernelGGL((pauli_rdm_tiled_kernel<T, Sector, 16>), gr, bl, 0, s, g, (unsigned)ksplit, (unsigned)steps, (unsigned)tiles,
                         n_down, pt, tile_list, x, partials);
      break;
  }
  LL_HIP(hipGetLastError());
}
}  // namespace

template <typename T>
void pauli_rdm_tiled_run(ll_context* ctx, const ll_operator* op, int m, const int32_t* sites, const void* psi, void* out,
                         int64_t* sweeps_out) {
  constexpr bool cplx = kTiledComplex<T>;
  const bool sector = op->kind == ll_operator::PAULI_SECTOR;
  const int n_sites = sector ? op->pauli_sector.n_sites : op->pauli.n_sites;
  const int n_down = sector ? (int)op->pauli_sector.n_down : 0;
  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int kc = pauli_rdm_tiled_kc(ctx->tune.pauli_rdm_tiled_kc);
  const PauliRdmTiledGeom g = pauli_rdm_tiled_geom(n_sites, m, sites, kc);
  const int64_t tiles = pauli_rdm_tiled_tiles(g), nb = pauli_rdm_tiled_blocks_per_side(g);
  const int64_t ksplit = pauli_rdm_tiled_ksplit(g, cplx, ctx->tune.pauli_rdm_tiled_ksplit, kCUs);
  const int64_t steps = pauli_rdm_tiled_ksteps(g) / ksplit;
  // a sector: the macro-tiles whose blocks share no popcount are not launched (their slots are never read)
  std::vector<uint32_t> live;
  if (sector && g.bb > g.rb) {
    for (int64_t t = 0; t < tiles; ++t) {
      const PauliRdmBlock b = pauli_rdm_block_of((int)nb, (int)t);
      if (pauli_rdm_tiled_tile_live((uint32_t)b.bi, (uint32_t)b.bj, g.rb)) live.push_back((uint32_t)t);
    }
  }
  const int64_t launched = live.empty() ? tiles : (int64_t)live.size();
  DevBuf<uint32_t> tile_list;
  if (!live.empty()) stage_table(ctx, tile_list, live);
  DevBuf<T> staged;
  const T* const x = stage_in(ctx, staged, psi, op->n_local);
  DevBuf<double> partials, staged_out;
  partials.alloc(ctx, (size_t)(ksplit * tiles) * pauli_rdm_tiled_tile_doubles(cplx));
  const int64_t out_doubles = (int64_t)2 << (2 * m);
  double* const dout = stage_out<double>(ctx, staged_out, out, out_doubles);
  const PauliSectorPartner pt = sector ? pauli_sector_partner(op->pauli_sector) : PauliSectorPartner{nullptr, nullptr, nullptr, 0};
  if (sector)
    launch_pauli_rdm_tiled<T, true>(kc, launched * ksplit, g, ksplit, steps, tiles, n_down, pt, tile_list.p, x, partials.p, s);
  else
    launch_pauli_rdm_tiled<T, false>(kc, launched * ksplit, g, ksplit, steps, tiles, n_down, pt, tile_list.p, x, partials.p, s);
  const int64_t entries = (int64_t)1 << (2 * m);
  hipLaunchKernelGGL(pauli_rdm_tiled_finish_kernel, dim3((unsigned)((entries + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, g,
                     (unsigned)ksplit, (unsigned)tiles, cplx, sector, n_down, (const double*)partials.p, dout);
  LL_HIP(hipGetLastError());
  stage_out_finish<double>(ctx, staged_out, out, out_doubles);
  LL_HIP(hipStreamSynchronize(s));  // the staged vectors, the table and a pageable psi are no longer read
  if (sweeps_out) *sweeps_out = 1;
}

// what capi.cpp calls: the checks, all before the device is touched, then the operator's type
void pauli_rdm_tiled(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites, const void* psi, void* out,
                     int64_t* sweeps_out) {
  LL_REQUIRE(ctx != nullptr && op != nullptr && sites != nullptr && psi != nullptr && out != nullptr, "null argument");
  pauli_measure_prologue(ctx, "reduced density matrices", {{op, "the operator"}});
  if (op->kind == ll_operator::PAULI_MOMENTUM || op->kind == ll_operator::PAULI_MOMENTUM_FULL || op->kind == ll_operator::PAULI_SYMMETRIC)
    LL_REQUIRE(false, std::string("the operator is ") + operator_kind_name(op->kind) +
                          ": reduced density matrices of symmetry blocks are not built (a site is not a tensor factor of the "
                          "block's basis); expand the block state (ll_pauli_block_expand) and measure on its full-space or "
                          "S_z-sector target");
  LL_REQUIRE(op->kind == ll_operator::PAULI || op->kind == ll_operator::PAULI_SECTOR,
             std::string("the operator is ") + operator_kind_name(op->kind) +
                 ": a reduced density matrix needs an operator that defines a spin basis (full-space or S_z-sector sum of Pauli "
                 "strings)");
  const int n_sites = op->kind == ll_operator::PAULI_SECTOR ? op->pauli_sector.n_sites : op->pauli.n_sites;
  int which = -1;
  const PauliRdmSiteError err = pauli_rdm_tiled_check_sites(n_sites, n_sub, sites, &which);
  LL_REQUIRE(err != kRdmBadCount, "n_sub = " + std::to_string(n_sub) + ": the tiled form takes " + std::to_string(kPauliRdmTiledMinSites) +
                                      " to min(" + std::to_string(kPauliRdmTiledMaxSites) + ", n_sites = " + std::to_string(n_sites) +
                                      ") sites");
  LL_REQUIRE(err != kRdmSiteOutOfRange, "site " + std::to_string(which) + " of the list (" +
                                            std::to_string(which >= 0 ? sites[which] : 0) + ") is outside [0, n_sites = " +
                                            std::to_string(n_sites) + ")");
  LL_REQUIRE(err != kRdmSiteRepeated, "site " + std::to_string(which) + " of the list (" +
                                          std::to_string(which >= 0 ? sites[which] : 0) + ") is repeated");
  for_storage_type(*op, [&](auto t) { pauli_rdm_tiled_run<decltype(t)>(ctx, op, n_sub, sites, psi, out, sweeps_out); });
}

}  // namespace ll
