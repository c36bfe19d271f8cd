// Hand-written HIP kernels for gfx950 (MI355X / CDNA4): the device side of the Lanczos hot path.
//
// Every kernel here is HBM-bandwidth bound (SpMV 0.15 flop/B, BLAS-1 <= 0.25 flop/B, ridge ~10
// flop/B), so there is no MFMA anywhere; what matters is coalesced 16-byte-per-lane streaming, enough loads
// in flight per CU, LDS-staged partial sums, 64-wide wavefront reductions and XCD-aware tile placement.
//
// Reference rows:
//   a1/a2/a3  spmv_stream      mv_mul (LL:243, EX:108) + offset update (LL:244-246) + alpha dot (LL:248, EX:110)
//   a4        mdot (prologue)  three-term update (LL:251-257, EX:112-118)
//   a5/a6     mdot + maxpy     Gram-Schmidt against locked + Krylov vectors (LA:132-144 at LL:259-260, EX:121)
//   a7        maxpy (epilogue) ||w||^2 (LA:56-60 at LL:262, EX:145)
//   a8        scale            normalize (LA:65-80 at LL:285, EX:160)
//   a9/a10    gemv_basis       Ritz vectors (LL:51-57) / exp(aA)v (EX:166-170)
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"

namespace ll {


// ================================================================= a1/a2/a3: CSR SpMV ("CSR-stream")
// One tile = a run of whole rows holding <= kSpmvTileNnz nonzeros (built at upload time).  The workgroup streams
// the tile's (val, col) pairs with perfectly coalesced loads regardless of the row lengths, multiplies by the
// gathered x entries and stages the products in LDS; then a power-of-two group of lanes per row folds its
// segment of the LDS array (wavefront shuffles), adds offset*x_i (a2), writes y_i and accumulates
// Re(conj(x_i) y_i) (a3) — one pass over the matrix, no separate offset or dot sweeps.
// A row longer than a tile is its own tile and is folded by the whole workgroup.
template <typename T, typename RP>
__global__ __launch_bounds__(kBlock) void spmv_stream(int ntiles, const int32_t* __restrict__ tile_rows,
                                                      const RP* __restrict__ rp, const int32_t* __restrict__ ci,
                                                      const T* __restrict__ va, const T* __restrict__ xf,
                                                      const T* __restrict__ xl, T* __restrict__ y, double offset,
                                                      double* __restrict__ dot_partials, ScaleIn<T> sc, int part) {
  // part (sharded operators whose image is split by column ownership, operators.cpp build_csr_split): 0 = the whole matrix in
  // one pass; 1 = the own-column part, y = A_own x + offset x (runs under the all-gather, no dot product yet);
  // 2 = the other ranks' columns, y += A_rem x, then Re<x, y> of the finished rows.
  __shared__ T prod[kSpmvTileNnz];
  __shared__ double red[4 * scalar_traits<T>::reals + 5];
  const int tid = threadIdx.x;
  double dot_acc = 0.0;
  // deferred normalisation: xf / xl hold w, the kernel works with u = sfac * w (linear: applied to the row sums and to x_i)
  const double sfac = scale_in_factor<T>(sc, red);

  for (TileWalk tw(ntiles); tw.first < tw.end; tw.first += tw.step) {
    const int t = tw.first;
    const int r0 = tile_rows[t], r1 = tile_rows[t + 1];
    const long long p0 = (long long)rp[r0], p1 = (long long)rp[r1];
    const int cnt = (int)min(p1 - p0, (long long)kSpmvTileNnz + 1);
    const int nr = r1 - r0;
    if (nr == 1 && p1 - p0 > kSpmvTileNnz) {
      // long row: the whole workgroup strides over it
      acc_t<T> acc = zero<acc_t<T>>();
      for (long long p = p0 + tid; p < p1; p += kBlock) fma_acc(acc, va[p], xf[ci[p]]);
      acc_t<T> tot;
      if constexpr (scalar_traits<T>::is_complex) {
        double a = block_sum(acc.re, red);
        double b = block_sum(acc.im, red);
        tot = zc{a, b};
      } else {
        tot = block_sum(acc, red);
      }
      if (tid == 0) {
        const T xi = rmul(sfac, xl[r0]);
        if (sc.u_out) sc.u_out[r0] = xi;
        T yi = part == 2 ? add(y[r0], narrow<T>(scale_acc(sfac, tot))) : add(narrow<T>(scale_acc(sfac, tot)), rmul(offset, xi));
        y[r0] = yi;
        if (part != 1) dot_acc += re_cmul(xi, yi);
      }
      continue;
    }
    (void)cnt;
    const int len = (int)(p1 - p0);
    __syncthreads();  // previous tile's readers are done with prod[]
#pragma unroll 4
    for (int i = tid; i < len; i += kBlock) {
      const long long p = p0 + i;
      prod[i] = mul(va[p], xf[ci[p]]);
    }
    __syncthreads();
    // lanes per row: largest power of two with nr * lanes <= kBlock, at most 64
    int lanes = 1;
    while (lanes < 64 && nr * (lanes << 1) <= kBlock) lanes <<= 1;
    const int g = tid / lanes, l = tid - g * lanes;
    acc_t<T> acc = zero<acc_t<T>>();
    int row = r0 + g;
    if (g < nr) {
      const int a = (int)((long long)rp[row] - p0), b = (int)((long long)rp[row + 1] - p0);
      for (int i = a + l; i < b; i += lanes) acc = add(acc, to_acc(prod[i]));
    }
    for (int d = lanes >> 1; d > 0; d >>= 1) {
      if constexpr (scalar_traits<T>::is_complex) {
        acc.re += __shfl_down(acc.re, d, 64);
        acc.im += __shfl_down(acc.im, d, 64);
      } else {
        acc += __shfl_down(acc, d, 64);
      }
    }
    if (g < nr && l == 0) {
      const T xi = rmul(sfac, xl[row]);
      if (sc.u_out) sc.u_out[row] = xi;
      T yi = part == 2 ? add(y[row], narrow<T>(scale_acc(sfac, acc))) : add(narrow<T>(scale_acc(sfac, acc)), rmul(offset, xi));
      y[row] = yi;
      if (part != 1) dot_acc += re_cmul(xi, yi);
    }
  }
  if (dot_partials) {
    double tot = block_sum(dot_acc, red);
    if (tid == 0) dot_partials[blockIdx.x] = tot;
  }
}

// Persistent grid of the CSR-stream kernel: 8 workgroups per CU for 4- and 8-byte values, 16 for complex double (20 KB
// of matrix per tile: 24.8 us instead of 27.4 us per SpMV on config 5, 68 % instead of 62 % of the roofline; config 2 is
// best at 8: 17.8 us against 18.2 us; profiles/r02_csr_stream_grid_sweep.txt).
static int spmv_grid(int ntiles, size_t elem_bytes) {
  const int cap = elem_bytes >= 16 ? kMaxSpmvGrid : kMaxGrid;
  int g = ntiles < cap ? ((ntiles + kXcds - 1) / kXcds) * kXcds : cap;
  return g < kXcds ? kXcds : g;
}

template <typename T>
int launch_spmv(const ll_operator& op, const T* x_full, const T* x_local, T* y, double offset, double* dot_partials,
                hipStream_t s, const ScaleIn<T>* scp, int part) {
  // part 1 / 2: the two halves of a column-split image (x_full = the local shard for part 1, the gathered vector for part 2)
  const CsrImage& im = part == 1 ? op.csr_own : (part == 2 ? op.csr_rem : op.csr);
  const int ntiles = im.ntiles;
  const int32_t* tiles = im.tiles.get();
  const void* rp = im.row_ptr.get();
  const int32_t* ci = im.col.get();
  const void* va = im.val.get();
  const int grid = spmv_grid(ntiles, sizeof(T));
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  // (the kernel that publishes an iteration's scalars may complete that iteration's event itself: ll_context::stop_next)
  hipEvent_t stop = part != 1 ? op.ctx->stop_next : nullptr;
  op.ctx->stop_next = stop ? nullptr : op.ctx->stop_next;
  if (im.rp64)
    LL_LAUNCH_STOP(stop, (spmv_stream<T, int64_t>), dim3(grid), dim3(kBlock), 0, s, ntiles, tiles, (const int64_t*)rp, ci,
                   (const T*)va, x_full, x_local, y, offset, part == 1 ? nullptr : dot_partials, sc, part);
  else
    LL_LAUNCH_STOP(stop, (spmv_stream<T, int32_t>), dim3(grid), dim3(kBlock), 0, s, ntiles, tiles, (const int32_t*)rp, ci,
                   (const T*)va, x_full, x_local, y, offset, part == 1 ? nullptr : dot_partials, sc, part);
  LL_HIP(hipGetLastError());
  return grid;
}

// ---- column split of a sharded CSR image: entries over the rank's own columns (rebased to the local shard) and the rest
template <typename RP>
__global__ __launch_bounds__(256) void csr_count_own_kernel(long long n_local, long long col0, long long col1,
                                                            const RP* __restrict__ rp, const int32_t* __restrict__ ci,
                                                            int32_t* __restrict__ own_cnt) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_local; i += (long long)gridDim.x * 256) {
    int c = 0;
    for (long long p = (long long)rp[i]; p < (long long)rp[i + 1]; ++p) c += (ci[p] >= col0 && ci[p] < col1) ? 1 : 0;
    own_cnt[i] = c;
  }
}
template <typename T, typename RP>
__global__ __launch_bounds__(256) void csr_split_kernel(long long n_local, long long col0, long long col1,
                                                        const RP* __restrict__ rp, const int32_t* __restrict__ ci,
                                                        const T* __restrict__ va, const RP* __restrict__ rp_own,
                                                        const RP* __restrict__ rp_rem, int32_t* __restrict__ ci_own,
                                                        T* __restrict__ va_own, int32_t* __restrict__ ci_rem,
                                                        T* __restrict__ va_rem) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_local; i += (long long)gridDim.x * 256) {
    long long qo = (long long)rp_own[i], qr = (long long)rp_rem[i];
    for (long long p = (long long)rp[i]; p < (long long)rp[i + 1]; ++p) {  // the order inside a row is kept in both halves
      const int c = ci[p];
      if (c >= col0 && c < col1) {
        ci_own[qo] = (int32_t)(c - col0);
        va_own[qo++] = va[p];
      } else {
        ci_rem[qr] = c;
        va_rem[qr++] = va[p];
      }
    }
  }
}
template <typename T>
void launch_csr_count_own(const ll_operator& op, int32_t* own_cnt, hipStream_t s) {
  const int grid = (int)std::max<long long>(1, std::min<long long>(kMaxGrid, (op.n_local + 255) / 256));
  const long long c0 = op.row_begin, c1 = op.row_begin + op.n_local;
  const CsrImage& a = op.csr;
  if (a.rp64)
    hipLaunchKernelGGL((csr_count_own_kernel<int64_t>), dim3(grid), dim3(256), 0, s, (long long)op.n_local, c0, c1,
                       (const int64_t*)a.row_ptr.get(), a.col.get(), own_cnt);
  else
    hipLaunchKernelGGL((csr_count_own_kernel<int32_t>), dim3(grid), dim3(256), 0, s, (long long)op.n_local, c0, c1,
                       (const int32_t*)a.row_ptr.get(), a.col.get(), own_cnt);
  LL_HIP(hipGetLastError());
}
template <typename T> void launch_csr_split(const ll_operator& op, const CsrImage& own, const CsrImage& rem, hipStream_t s) {
  const int grid = (int)std::max<long long>(1, std::min<long long>(kMaxGrid, (op.n_local + 255) / 256));
  const long long c0 = op.row_begin, c1 = op.row_begin + op.n_local;
  const CsrImage& a = op.csr;
  if (a.rp64)
    hipLaunchKernelGGL((csr_split_kernel<T, int64_t>), dim3(grid), dim3(256), 0, s, (long long)op.n_local, c0, c1,
                       (const int64_t*)a.row_ptr.get(), a.col.get(), (const T*)a.val.get(), (const int64_t*)own.row_ptr.get(),
                       (const int64_t*)rem.row_ptr.get(), own.col.get(), (T*)own.val.get(), rem.col.get(), (T*)rem.val.get());
  else
    hipLaunchKernelGGL((csr_split_kernel<T, int32_t>), dim3(grid), dim3(256), 0, s, (long long)op.n_local, c0, c1,
                       (const int32_t*)a.row_ptr.get(), a.col.get(), (const T*)a.val.get(), (const int32_t*)own.row_ptr.get(),
                       (const int32_t*)rem.row_ptr.get(), own.col.get(), (T*)own.val.get(), rem.col.get(), (T*)rem.val.get());
  LL_HIP(hipGetLastError());
}
#define LL_INST_SPMV(T)                                                                                                       \
  template int launch_spmv<T>(const ll_operator&, const T*, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*, int); \
  template void launch_csr_count_own<T>(const ll_operator&, int32_t*, hipStream_t);                                            \
  template void launch_csr_split<T>(const ll_operator&, const CsrImage&, const CsrImage&, hipStream_t);
LL_INST_SPMV(double) LL_INST_SPMV(zc) LL_INST_SPMV(float) LL_INST_SPMV(cf)


// ================================================================= strip geometry of the BLAS-1 kernels
// A workgroup owns strips of kBlock*EPT consecutive elements; every lane keeps EPT elements of w in registers as
// 16-byte pieces, so one strip of one basis vector is EPT*sizeof(T)/16 dwordx4 loads per lane.
constexpr int kJB = 4;  // basis vectors per trip of the streaming multi-dot / multi-axpy loops

template <typename T> struct strip {
  static constexpr int EPT = (int)(64 / sizeof(T));  // 64 B per lane per vector: 16 float, 8 double / cf, 4 zc
  static constexpr int ELEMS = kBlock * EPT;
};
// The Gram-Schmidt kernels come in two geometries: STREAMING (below; vectors of >= 4 MiB: enough 16 KiB strips to fill
// the chip, every load a full line) and SMALL-VECTOR (mdot_small / maxpy_small further down; n <~ 5e5 doubles, the
// reference's everyday sizes).  The boundary is Tuning::blas_small_bytes (LL_BLAS_SMALL_BYTES: 0 = always streaming,
// huge = always small), handed to the launchers by the caller.
static bool blas_small(int64_t n, size_t elem_bytes, int64_t limit) { return n * (int64_t)elem_bytes < limit; }

// Balanced persistent grid: every workgroup walks the same number of strips (grid-stride), so no tail round.
// (Measured alternative, round 2: equal CONTIGUOUS shares per workgroup instead of strips dealt out round-robin —
// perfectly balanced, but 8 % slower on the Gram-Schmidt kernels (5.35 vs 5.83 TB/s at n = 1e7): with the round-robin
// walk the whole chip sweeps each basis vector front to back, which is what the HBM row buffers like.)
// Grid target: 1024 workgroups, but ONE per CU once a vector has more than ~2.25 16-KiB strips per CU (> 9 MiB): every
// workgroup then sweeps several strips back to back — config 3 (80 MB vectors): 6.0 instead of 5.9 TB/s; the 40 / 20 /
// 10 MB shards of config 4: Gram-Schmidt -13 % / -9 % / -3 % (profiles/r02_strip_grid_sweep.txt).  At 8 MiB (config 2,
// 489 strips) the small grid is 2 % slower: too few strips to balance.
static int strip_grid(int64_t n, int elems) {
  int64_t strips = (n + elems - 1) / elems;
  if (strips < 1) strips = 1;
  const bool streaming = elems >= 1024;  // the small-vector kernels' strips are 64 .. 256 elements
  const int target = streaming && strips > 2 * kCUs + kCUs / 4 ? kCUs : 1024;
  const int64_t per = (strips + target - 1) / target;
  return (int)((strips + per - 1) / per);
}

// A lane's EPT elements are contiguous (64 B = four 16-byte pieces) and lanes are adjacent: the four loads of a wave
// cover 4 KiB of consecutive memory, each of them touching the same 32 lines (the 2nd to 4th hit in L1 / merge with
// the outstanding misses).  Measured alternatives, round 2 (A/B in one process through a device flag): 16-byte pieces
// laid out so that every single instruction is contiguous over the workgroup, or over the wave: 5.67-5.71 vs
// 5.71-5.80 TB/s at n = 1e7 (no gain) and slower at n = 1e6 — this layout stays.
template <typename T>
__device__ __forceinline__ void load_strip(const T* __restrict__ v, int64_t base, int64_t n, T (&r)[strip<T>::EPT]) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int PIECES = 4;
  const int64_t i0 = base + (int64_t)threadIdx.x * EPT;
  if (i0 + EPT <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(v + i0);
    uint4 c[PIECES];
#pragma unroll
    for (int e = 0; e < PIECES; ++e) c[e] = p[e];
    __builtin_memcpy(&r[0], c, sizeof(c));
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = (i0 + e < n) ? v[i0 + e] : zero<T>();
  }
}
template <typename T>
__device__ __forceinline__ void store_strip(T* __restrict__ v, int64_t base, int64_t n,
                                            const T (&r)[strip<T>::EPT]) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int PIECES = 4;
  const int64_t i0 = base + (int64_t)threadIdx.x * EPT;
  if (i0 + EPT <= n) {
    uint4 c[PIECES];
    __builtin_memcpy(c, &r[0], sizeof(c));
    uint4* p = reinterpret_cast<uint4*>(v + i0);
#pragma unroll
    for (int e = 0; e < PIECES; ++e) p[e] = c[e];
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (i0 + e < n) v[i0 + e] = r[e];
  }
}

// One trip of the multi-dot: NV basis strips against the strip of w held in registers; the NV (x2 for complex) wave
// sums are added to the wave's LDS row `mine_col[0 .. R*NV)`.
template <typename T, int NV>
__device__ __forceinline__ void mdot_trip(const T* __restrict__ u0, int64_t ld, int64_t base, int64_t n,
                                          const T (&wr)[strip<T>::EPT], double* mine_col, int lane) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int R = scalar_traits<T>::reals;
  T ur[NV][EPT];
#pragma unroll
  for (int b = 0; b < NV; ++b) load_strip<T>(u0 + (int64_t)b * ld, base, n, ur[b]);
  // (complex types: real and imaginary parts in transposed reductions of their own, at most NV = 4 sums each — with all 2 NV
  // sums in one reduction the compiler sends part of the array through scratch memory, a round trip with a full drain of the
  // memory pipeline in every trip; checked in the ISA, round 5)
  double a[NV], ai[NV];
#pragma unroll
  for (int b = 0; b < NV; ++b) {
    acc_t<T> acc = zero<acc_t<T>>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) cfma_acc(acc, ur[b][e], wr[e]);
    if constexpr (scalar_traits<T>::is_complex) {
      a[b] = acc.re;
      ai[b] = acc.im;
    } else {
      a[b] = acc;
      ai[b] = 0.0;
    }
  }
  wave_sum_transposed<NV>(a, lane);
  constexpr int LPI = 64 / NV;  // lanes that end up holding the same sum
  if constexpr (scalar_traits<T>::is_complex) {
    wave_sum_transposed<NV>(ai, lane);
    if ((lane & (LPI - 1)) == 0) {
      mine_col[2 * (lane / LPI)] += a[0];
      mine_col[2 * (lane / LPI) + 1] += ai[0];
    }
  } else {
    if ((lane & (LPI - 1)) == 0) mine_col[lane / LPI] += a[0];
  }
  (void)R;
}

// One trip of the multi-axpy: w -= sum_b h_b u_b for NV basis strips, coefficients from LDS.
template <typename T, int NV>
__device__ __forceinline__ void maxpy_trip(const T* __restrict__ u0, int64_t ld, int64_t base, int64_t n,
                                           T (&wr)[strip<T>::EPT], const double* hcol) {
  constexpr int EPT = strip<T>::EPT;
  T ur[NV][EPT];
#pragma unroll
  for (int b = 0; b < NV; ++b) load_strip<T>(u0 + (int64_t)b * ld, base, n, ur[b]);
#pragma unroll
  for (int b = 0; b < NV; ++b) {
    acc_t<T> hj;
    if constexpr (scalar_traits<T>::is_complex) hj = zc{hcol[2 * b], hcol[2 * b + 1]};
    else hj = hcol[b];
#pragma unroll
    for (int e = 0; e < EPT; ++e) fnma_acc(wr[e], hj, ur[b][e]);
  }
}

// ================================================================= a4 + a5/a6 (projection half): multi-dot
// h_j = <u_j, w> for every vector of the segments, plus ||w||^2, in ONE pass that keeps the strip of w in
// registers while the basis strips stream through (k+1 vector reads for k dots instead of 2k).  Optionally the
// three-term update w = w - beta u_prev - alpha u_cur is applied on the fly (saves 3R 1W of a separate sweep).
// Per-wave partial sums live in LDS ([4][ncols]) across all strips of the workgroup; each workgroup finally writes
// one row of ncols partials which reduce_cols folds in a fixed order (deterministic, no atomics).
template <typename T>
__global__ __launch_bounds__(kBlock) void mdot_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs,
                                                      ThreeTerm<T> tt, NormRefs pred, int predicated,
                                                      double* __restrict__ partials, int ncols) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  constexpr int JB = kJB;
  constexpr int R = scalar_traits<T>::reals;
  extern __shared__ double lds[];  // [4 waves][ncols]
  if (predicated && !second_pass_due(pred)) return;  // predicated second DGKS pass
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * ncols; i += kBlock) lds[i] = 0.0;
  __syncthreads();
  double* mine = lds + (size_t)wave * ncols;

  double alpha = 0.0, beta = 0.0;
  const bool do_tt = tt.u_cur != nullptr;
  if (do_tt) {
    if (tt.alpha_partials) {  // deferred alpha: fold the operator kernel's partials here (ThreeTerm)
      __shared__ double fold_scratch[5];
      alpha = fold_partials_all(tt.alpha_partials, tt.alpha_nparts, fold_scratch);
      if (blockIdx.x == 0 && tid == 0) *tt.alpha_out = alpha;
    } else {
      alpha = *tt.alpha;
    }
    if (tt.u_prev) beta = sqrt(final_norm2(tt.prev));
  }

  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * ELEMS;
    T wr[EPT];
    load_strip<T>(w, base, n, wr);
    if (do_tt) {
      T uc[EPT];
      load_strip<T>(tt.u_cur, base, n, uc);
      if (tt.u_prev) {
        T up[EPT];
        load_strip<T>(tt.u_prev, base, n, up);
#pragma unroll
        for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, up[e])), rmul(alpha, uc[e]));
      } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, uc[e]));
      }
      store_strip<T>(w, base, n, wr);
    }
    int col = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      // JB basis vectors per trip: all JB strips are requested before the first one is consumed, and their JB (x2 for
      // complex) wave sums are formed together
      int j = 0;
      for (; j + JB <= cnt; j += JB, col += R * JB) mdot_trip<T, JB>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, mine + col, lane);
      if (j + 2 <= cnt) { mdot_trip<T, 2>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, mine + col, lane); j += 2; col += R * 2; }
      if (j < cnt) { mdot_trip<T, 1>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, mine + col, lane); j += 1; col += R; }
    }
    double nn = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) nn += abs2(wr[e]);
    nn = wave_sum(nn);
    if (lane == 0) mine[ncols - 1] += nn;
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock)
    out[i] = (lds[i] + lds[ncols + i]) + (lds[2 * ncols + i] + lds[3 * ncols + i]);
}

// ================================================================= lagged block Gram-Schmidt: ONE sweep over the basis per iteration
// Block classical Gram-Schmidt needs the coefficients h = U^H w (a global reduction) before it can update w, hence two
// sweeps over the basis per iteration (mdot, maxpy above).  The whole-loop drivers on one GPU apply the update ONE
// ITERATION LATE instead, in the same sweep that computes the next iteration's coefficients.  Notation for iteration k
// (u_0 .. u_{k-2} complete in the basis, nb = k-1 of them):
//   r     raw w_{k-1}: neither corrected nor normalised,   g = U^H r,   beta^2 = ||r||^2 - |g|^2   (previous fold),
//   x~    = r / beta = u_{k-1} + e,  e = U c,  c = g / beta: what the operator kernel was applied to (it scales on the fly),
//   y     = A x~.
// One pass per strip forms   wr = y - alpha x~ - beta u_{k-2}             (three-term update on the perturbed input)
//                            u_{k-1} = (r - sum_j g_j u_j) / beta         (the late update, written to its basis slot)
//                            m_j = <u_j, wr>  for j < k-1
//                            w  = wr - sum_{j<k-1} d_j u_j - d_{k-1} u_{k-1}   (compensation, see below; replaces y)
//                            m_{k-1} = <u_{k-1}, w>,  ||w||^2.
// The basis streams through ONCE (k+2 vector reads, 2 writes instead of 2k+3 reads, 2 writes).
//
// Compensation.  Left alone, the perturbation e feeds itself: (A - alpha) e lies in span(U) with coefficients
// (T - alpha) c, which become the next iteration's g, so |c| grows by ||T - alpha|| / beta ~ 2 per iteration (1e-16 -> 1
// in about fifty iterations; measured).  But c is KNOWN, and so is the image of e: the stored
// vectors satisfy A u_j = beta_{j-1} u_{j-1} + alpha_j u_j + beta_j u_{j+1} to rounding, hence
//   (A - alpha) e = sum_i d_i u_i,   d = Tbar c - alpha [c; 0]    (Tbar: the (k x k-1) tridiagonal of recorded alpha, beta)
// is subtracted from w in the same sweep (the u_i stream through anyway), and the measured coefficients are corrected
// by linearity, <u_j, w> = m_j - d_j.  alpha = <x~, A x~> carries 2 Re <e, A u_{k-1}> = 2 Re g_{k-2} (only u_{k-2} couples
// to u_{k-1}) and <e, A e> = Re c^H t; both are removed before use (lagged_alpha).  Nothing else is nonlinear in e, so
// the algebra is exact for ANY size of c (an injected |c| = 0.5 leaves the traces at 1e-14, which matters near breakdown
// where beta ~ eps makes c = g / beta large without tripping the DGKS test).  What is left in w along span(U) is fresh
// rounding, as in the two-sweep form: |c| stays at a few eps for hundreds of iterations (tests/test_gpu_round3.py), the recorded
// alpha / beta agree with the two-sweep form to ~1e-14 relative.  t = Tbar c comes from the fold kernel below
// (lagged_fold_kernel); d_j = t_j - alpha c_j is formed here because alpha is only known now.
// The DGKS case (|g|^2 > ||r||^2 / 2: cancellation, the derived norm is inaccurate) is detected by the host from the
// published norms like before and repaired with the two-sweep kernels on the then complete u_{k-1} (engine.cpp,
// LoopState).
// alpha of a lagged iteration without the perturbation's terms: <u + e, A (u + e)> = alpha + 2 Re <e, A u> + <e, A e> with
// <e, A u_{k-1}> = conj(c_{k-2}) beta_{k-2} = conj(g_{k-2}) and q = <e, A e> = Re c^H t (lagged_fold_kernel).  Same
// operations in the sweep and in the fold: same bits.
__device__ __forceinline__ double lagged_alpha(double alpha, double g_last_re, double q) {
  return fma(-2.0, g_last_re, alpha) - q;
}

// Strip geometry of the one-sweep kernel: PC 16-byte pieces per lane and vector.  4 (64 B per lane, 16 KiB strips) is the
// streaming geometry of mdot / maxpy; vectors of 1 .. 3 MB have too few such strips to occupy the chip (n = 2e5 doubles:
// 99 workgroups, 2.4 TB/s), so they take 2 pieces per lane: twice the workgroups, each wave's chain of trips as long as
// before but with half the bytes.  Laplacian, window 100, it/s with 4 / 2 / 1 pieces: n = 2.0e5 15.6 k / 18.4 k / 18.2 k,
// 3.6e5 14.0 k / 14.6 k / 13.7 k, 5.0e5 12.1 k / 10.0 k / 11.5 k, 1e6 7.9 k / 7.2 k / 6.9 k, config 3 604 / 589:
// 2 pieces below 200 strips of 16 KiB, 4 from there (profiles/r03_small_vector_kernel_gaps.txt).
template <typename T, int PC> struct lstrip {
  static constexpr int EPT = (int)(PC * 16 / sizeof(T));
  static constexpr int ELEMS = kBlock * EPT;
};
template <typename T, int PC>
__device__ __forceinline__ void load_lstrip(const T* __restrict__ v, int64_t base, int64_t n, T (&r)[lstrip<T, PC>::EPT]) {
  constexpr int EPT = lstrip<T, PC>::EPT;
  const int64_t i0 = base + (int64_t)threadIdx.x * EPT;
  if (i0 + EPT <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(v + i0);
    uint4 c[PC];
#pragma unroll
    for (int e = 0; e < PC; ++e) c[e] = p[e];
    __builtin_memcpy(&r[0], c, sizeof(c));
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = (i0 + e < n) ? v[i0 + e] : zero<T>();
  }
}
template <typename T, int PC>
__device__ __forceinline__ void store_lstrip(T* __restrict__ v, int64_t base, int64_t n, const T (&r)[lstrip<T, PC>::EPT]) {
  constexpr int EPT = lstrip<T, PC>::EPT;
  const int64_t i0 = base + (int64_t)threadIdx.x * EPT;
  if (i0 + EPT <= n) {
    uint4 c[PC];
    __builtin_memcpy(c, &r[0], sizeof(c));
    uint4* p = reinterpret_cast<uint4*>(v + i0);
#pragma unroll
    for (int e = 0; e < PC; ++e) p[e] = c[e];
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (i0 + e < n) v[i0 + e] = r[e];
  }
}
template <typename T, int NV, int PC>
__device__ __forceinline__ void lagged_trip(const T* __restrict__ u0, int64_t ld, int64_t base, int64_t n,
                                            const T (&wr)[lstrip<T, PC>::EPT], T (&wp)[lstrip<T, PC>::EPT], T (&uc)[lstrip<T, PC>::EPT],
                                            const double* __restrict__ gcol, const double* __restrict__ tcol, double as,
                                            double* mine_col, int lane) {
  constexpr int EPT = lstrip<T, PC>::EPT;
  constexpr int R = scalar_traits<T>::reals;
  T ur[NV][EPT];
#pragma unroll
  for (int b = 0; b < NV; ++b) load_lstrip<T, PC>(u0 + (int64_t)b * ld, base, n, ur[b]);
  double a[NV], ai[NV];  // (complex: real and imaginary parts reduced separately, see mdot_trip)
#pragma unroll
  for (int b = 0; b < NV; ++b) {
    // g_j and d_j = t_j - (alpha / beta) g_j: wave-uniform addresses in read-only memory (scalar loads, no LDS copy, so
    // the LDS budget belongs to the partial columns alone)
    acc_t<T> gj, dj;
    if constexpr (scalar_traits<T>::is_complex) {
      gj = zc{gcol[2 * b], gcol[2 * b + 1]};
      dj = zc{fma(-as, gj.re, tcol[2 * b]), fma(-as, gj.im, tcol[2 * b + 1])};
    } else {
      gj = gcol[b];
      dj = fma(-as, gj, tcol[b]);
    }
    acc_t<T> acc = zero<acc_t<T>>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      fnma_acc(uc[e], gj, ur[b][e]);   // late update of the previous vector
      fnma_acc(wp[e], dj, ur[b][e]);   // compensation of the new one
      cfma_acc(acc, ur[b][e], wr[e]);  // this iteration's (raw) coefficient
    }
    if constexpr (scalar_traits<T>::is_complex) {
      a[b] = acc.re;
      ai[b] = acc.im;
    } else {
      a[b] = acc;
      ai[b] = 0.0;
    }
  }
  wave_sum_transposed<NV>(a, lane);
  constexpr int LPI = 64 / NV;
  if constexpr (scalar_traits<T>::is_complex) {
    wave_sum_transposed<NV>(ai, lane);
    if ((lane & (LPI - 1)) == 0) {
      mine_col[2 * (lane / LPI)] += a[0];
      mine_col[2 * (lane / LPI) + 1] += ai[0];
    }
  } else {
    if ((lane & (LPI - 1)) == 0) mine_col[lane / LPI] += a[0];
  }
  (void)R;
}

template <typename T, int PC>
__global__ __launch_bounds__(kBlock) void lagged_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs, int nb,
                                                        Lagged<T> lg, const double* __restrict__ g,
                                                        const double* __restrict__ t, ThreeTerm<T> tt,
                                                        double* __restrict__ partials) {
  constexpr int EPT = lstrip<T, PC>::EPT;
  constexpr int ELEMS = lstrip<T, PC>::ELEMS;
  constexpr int JB = kJB;
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = R * (nb + 1) + 1;
  extern __shared__ double lds[];  // [4 waves][ncols] partial columns
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * ncols; i += kBlock) lds[i] = 0.0;
  double alpha;
  if (tt.alpha_partials) {  // deferred alpha: fold the operator kernel's partials here (ThreeTerm)
    __shared__ double fold_scratch[5];
    alpha = fold_partials_all(tt.alpha_partials, tt.alpha_nparts, fold_scratch);
    if (blockIdx.x == 0 && tid == 0) *tt.alpha_out = alpha;  // as measured; lagged_fold_kernel corrects it in place
  } else {
    alpha = *tt.alpha;
  }
  alpha = lagged_alpha(alpha, g[R * (nb - 1)], t[R * (nb + 1)]);  // lagged_fold_kernel publishes the same value
  const double beta = sqrt(*lg.beta2), s = 1.0 / beta;
  const double as = alpha * s;
  __syncthreads();
  double* mine = lds + (size_t)wave * ncols;
  acc_t<T> dlast;  // the component on u_{k-1} itself
  if constexpr (scalar_traits<T>::is_complex) dlast = zc{t[R * nb], t[R * nb + 1]};
  else dlast = t[R * nb];

  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * ELEMS;
    T wr[EPT], wp[EPT], uc[EPT];
    load_lstrip<T, PC>(w, base, n, wr);
    load_lstrip<T, PC>(lg.r, base, n, uc);
    if (tt.u_prev) {
      T up[EPT];
      load_lstrip<T, PC>(tt.u_prev, base, n, up);
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, up[e])), rmul(alpha, rmul(s, uc[e])));
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, rmul(s, uc[e])));
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) wp[e] = wr[e];
    int col = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      int j = 0;
      for (; j + JB <= cnt; j += JB, col += R * JB)
        lagged_trip<T, JB, PC>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, wp, uc, g + col, t + col, as, mine + col, lane);
      if (j + 2 <= cnt) {
        lagged_trip<T, 2, PC>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, wp, uc, g + col, t + col, as, mine + col, lane);
        j += 2;
        col += R * 2;
      }
      if (j < cnt) {
        lagged_trip<T, 1, PC>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, wp, uc, g + col, t + col, as, mine + col, lane);
        j += 1;
        col += R;
      }
    }
    // u_{k-1} is complete: normalise, store; finish w with its own component, take the last coefficient and ||w||^2
    acc_t<T> last = zero<acc_t<T>>();
    double nn = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      uc[e] = rmul(s, uc[e]);
      fnma_acc(wp[e], dlast, uc[e]);
      cfma_acc(last, uc[e], wp[e]);
      nn += abs2(wp[e]);
    }
    store_lstrip<T, PC>(lg.u_out, base, n, uc);
    store_lstrip<T, PC>(w, base, n, wp);
    if constexpr (scalar_traits<T>::is_complex) {
      const double lr = wave_sum(last.re), li = wave_sum(last.im);
      if (lane == 0) {
        mine[R * nb] += lr;
        mine[R * nb + 1] += li;
      }
    } else {
      const double lr = wave_sum(last);
      if (lane == 0) mine[R * nb] += lr;
    }
    nn = wave_sum(nn);
    if (lane == 0) mine[ncols - 1] += nn;
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock)
    out[i] = (lds[i] + lds[ncols + i]) + (lds[2 * ncols + i] + lds[3 * ncols + i]);
}
template <typename T>
__global__ void lagged_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs, int nb, Lagged<T> lg,
                                    const double* __restrict__ g, const double* __restrict__ t, ThreeTerm<T> tt,
                                    double* __restrict__ partials);  // (further down, with the small-vector kernels)
int small_lagged_lds_doubles(int ncols, int ept_times_reals);
template <typename T>
int launch_lagged(int64_t n, T* w, const BasisSegs<T>& segs, const Lagged<T>& lg, const ThreeTerm<T>& tt, double* partials,
                  int pieces, int64_t small_limit, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = R * (nb + 1) + 1;
  if (n * (int64_t)sizeof(T) < small_limit) {  // small-vector geometry: four waves per 1 KiB strip split the basis
    const int grid = strip_grid(n, (int)(64 * (16 / sizeof(T))));
    const size_t lds_small = (size_t)small_lagged_lds_doubles(ncols, (int)(16 / sizeof(T)) * R) * sizeof(double);
    hipLaunchKernelGGL((lagged_small_kernel<T>), dim3(grid), dim3(kBlock), lds_small, s, n, w, segs, nb, lg, lg.g, lg.t, tt, partials);
    LL_HIP(hipGetLastError());
    return grid;
  }
  const size_t lds_bytes = (size_t)4 * ncols * sizeof(double);
  // pieces per lane: enough workgroups for the chip (see lstrip)
  const int64_t strips16k = (n * (int64_t)sizeof(T) + 16383) / 16384;
  int pc = strips16k >= kLaggedFullStrips ? 4 : 2;
  if (pieces == 2 || pieces == 4) pc = pieces;  // test hook (Tuning::lagged_pieces)
  int grid;
  if (pc == 4) {
    grid = strip_grid(n, lstrip<T, 4>::ELEMS);
    hipLaunchKernelGGL((lagged_kernel<T, 4>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, nb, lg, lg.g, lg.t, tt, partials);
  } else {
    grid = strip_grid(n, lstrip<T, 2>::ELEMS);
    hipLaunchKernelGGL((lagged_kernel<T, 2>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, nb, lg, lg.g, lg.t, tt, partials);
  }
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_LAGGED(T) \
  template int launch_lagged<T>(int64_t, T*, const BasisSegs<T>&, const Lagged<T>&, const ThreeTerm<T>&, double*, int, int64_t, hipStream_t);
LL_INST_LAGGED(double) LL_INST_LAGGED(zc) LL_INST_LAGGED(float) LL_INST_LAGGED(cf)

// The fold of a lagged iteration k (one workgroup; replaces derive_norm_kernel there).  Columns: L locked eigenvectors
// first, then the Lanczos vectors u_0 .. u_{k-1}; K = L + k.  `m` holds the reals * K column sums of the sweep (raw
// coefficients; the last one was taken on the finished w), *c0 = ||w||^2.
//   g_i   = m_i - d_i  for the columns the sweep took on wr (prev_g != nullptr: d from the previous fold's t, g and this
//           iteration's alpha, exactly as the sweep formed it);  g = m after a clean iteration (operator applied to a
//           complete u_{k-1}: mdot_kernel, nothing to compensate)
//   c1    = ||w||^2 - |g|^2 = beta_{k-1}^2,  c = g / beta_{k-1}
//   t     = the image of the next operator input's perturbation in the same columns (reals * (K + 1) values): Tbar c for
//           the Lanczos columns, lambda_i c_i for a locked eigenvector (A z_i = lambda_i z_i + r_i; c_i r_i is second
//           order in quantities of the size of the convergence tolerance); then q = Re c^H t
//   alpha_{k-1}, beta_{k-1} appended to the device copy of T; the four per-iteration scalars published to the host.
__global__ __launch_bounds__(256) void lagged_fold_kernel(double* __restrict__ m, int K, int L, int reals, double* __restrict__ t_out,
                                                          const double* c0, double* c0_out, double* __restrict__ c1,
                                                          double* __restrict__ alpha, const double* __restrict__ prev_g,
                                                          const double* __restrict__ prev_t, const double* __restrict__ prev_c1,
                                                          double* __restrict__ hist_alpha, double* __restrict__ hist_beta,
                                                          const double* __restrict__ lambda, double* __restrict__ host) {
  __shared__ double red[4];
  __shared__ double sh[2];
  const int tid = threadIdx.x;
  const int k = K - L;
  const int cnt = reals * K;
  double a = *alpha;
  if (prev_g) a = lagged_alpha(a, prev_g[reals * (K - 2)], prev_t[reals * K]);
  double acc = 0.0;
  if (prev_g) {
    const double as = a * (1.0 / sqrt(*prev_c1));
    for (int i = tid; i < cnt; i += 256) {
      double g = m[i];
      if (i < cnt - reals) {
        g -= fma(-as, prev_g[i], prev_t[i]);
        m[i] = g;
      }
      acc = fma(g, g, acc);
    }
  } else {
    for (int i = tid; i < cnt; i += 256) acc = fma(m[i], m[i], acc);
  }
  const double tot = block_sum(acc, red);
  if (tid == 0) {
    const double before = *c0;
    double v = before - tot;
    v = v > 0.0 ? v : 0.0;
    *c0_out = before;  // (sharded: out of the all-reduced buffer)
    *c1 = v;
    *alpha = a;
    hist_alpha[k - 1] = a;
    hist_beta[k - 1] = sqrt(v);
    sh[0] = a;
    sh[1] = sqrt(v);
    host[0] = a;
    host[1] = v;
    host[2] = before;
    host[3] = v;
  }
  __syncthreads();  // (also orders the m[i] updates above before the reads below)
  const double beta = sh[1], inv = beta > 0.0 ? 1.0 / beta : 0.0;
  double qacc = 0.0;
  for (int i = tid; i < reals * (K + 1); i += 256) {
    const int col = i / reals;
    double t = 0.0;
    if (col < L) {
      t = lambda[col] * m[i];
    } else {
      const int j = col - L;  // component on u_j
      if (j < k) t = (j == k - 1 ? sh[0] : hist_alpha[j]) * m[i];
      if (j + 1 < k) t = fma(hist_beta[j], m[i + reals], t);
      if (j >= 1) t = fma(j == k ? beta : hist_beta[j - 1], m[i - reals], t);
    }
    t *= inv;
    t_out[i] = t;
    if (col < K) qacc = fma(m[i] * inv, t, qacc);
  }
  const double q = block_sum(qacc, red);
  if (tid == 0) t_out[reals * (K + 1)] = q;
}
void launch_lagged_fold(double* m, int K, int L, int reals, double* t_out, const double* c0, double* c0_out, double* c1,
                        double* alpha, const double* prev_g, const double* prev_t, const double* prev_c1,
                        double* hist_alpha, double* hist_beta, const double* lambda, double* host_mapped, hipStream_t s, hipEvent_t stop) {
  LL_LAUNCH_STOP(stop, lagged_fold_kernel, dim3(1), dim3(256), 0, s, m, K, L, reals, t_out, c0, c0_out, c1, alpha, prev_g, prev_t,
                 prev_c1, hist_alpha, hist_beta, lambda, host_mapped);
  LL_HIP(hipGetLastError());
}

// ================================================================= TWO iterations per sweep over the basis ("pair" form)
// The one-sweep form above reads the basis once per iteration; here the operator is applied TWICE between sweeps and ONE
// sweep serves both iterations: s n (P + 12) bytes per two iterations instead of 2 s n (P + 4).  Executable specification,
// kernel by kernel, with the derivation and the numbers: tools/pair_gs_model.py (profiles/r05_pair_gs_model.txt).
// State between sweeps (P stored, complete, orthonormal vectors S = u_0 .. u_{P-1}; T recorded up to alpha_P, beta_P):
//   r1 -> u_P      raw, measured g1 = S^H r1,  rho1^2 = |r1|^2 - |g1|^2
//   r2 -> u_{P+1}  raw, measured g2 = S^H r2,  gam = <u_P, r2>,  rho2^2 = |r2|^2 - |g2|^2 - |gam|^2
// One pair:
//   y1 = A (r2 / rho2), e1 = <x2, y1>          operator kernel (scales its input, fused dot)
//   r3 = y1 - e1 x2 - rho2 x1                   pair_three_term_kernel (raw vectors only: every O(1) coefficient multiplies a
//   y2 = A (r3 / |r3|), e2                      raw vector; also |r3|^2 and <r1, r3>)
//   r4 = y2 - e2 x3 - |r3| x2                   pair_three_term_kernel
//   p4 = predicted S^H r4                       pair_predict_kernel: through the recorded tridiagonal, eps-sized numbers
//   ONE sweep (pair_sweep_kernel):  u_P = (r1 - S g1) / rho1,  u_{P+1} = (r2 - S g2 - gam u_P) / rho2  written to the basis,
//       m3 = S^H r3, m4 = S^H r4 measured, r4 -= S p4 (the NEXT operator input carries fresh rounding only along S),
//       in-strip <u_P, r3>, <u_{P+1}, r3>, <u_P, r4>, <u_{P+1}, r4>, <r3, r4>, |r4|^2
//   pair_fold_kernel: alpha_{P+1}, beta_{P+1}, alpha_{P+2}, beta_{P+2} and the next pair's (g1, rho1, g2, gam, rho2).
// Every stored vector is written with MEASURED coefficients, one sweep late; every measured coefficient is eps-sized.  The
// first-order effects of the perturbed operator inputs are measured and removed like in the one-sweep form; terms of
// SECOND order in the coefficients are not tracked here, so the form is only used while every coefficient stays below
// kPairGate relative to its vector (the fold publishes the largest one; near breakdown, where beta -> eps makes them grow,
// the host falls back to the one-sweep form, which is exact for coefficients of any size).
template <typename T>
__global__ __launch_bounds__(kBlock) void pair_three_term_kernel(int64_t n, T* __restrict__ y, const T* __restrict__ x,
                                                                 const T* __restrict__ p, double* __restrict__ e,
                                                                 const double* __restrict__ e_partials, int e_nparts,
                                                                 const double* __restrict__ cx2, const double* __restrict__ cp2,
                                                                 double* __restrict__ partials, int colmajor) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  __shared__ double red[4][1 + R];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double ev;
  if (e_partials) {  // deferred alpha: every workgroup folds the operator kernel's partials in the same fixed order (ThreeTerm)
    __shared__ double fold_scratch[5];
    ev = fold_partials_all(e_partials, e_nparts, fold_scratch);
    if (blockIdx.x == 0 && tid == 0) *e = ev;
  } else {
    ev = *e;
  }
  const double nx = sqrt(*cx2);
  const double ca = ev / nx;            // y - (e / |x|) x_raw - (|x| / |p|) p_raw
  const double cb = nx / sqrt(*cp2);
  double nn = 0.0;
  acc_t<T> dp = zero<acc_t<T>>();
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * ELEMS;
    T yr[EPT], xr[EPT], pr[EPT];
    load_strip<T>(y, base, n, yr);
    load_strip<T>(x, base, n, xr);
    load_strip<T>(p, base, n, pr);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      yr[i] = sub(sub(yr[i], rmul(ca, xr[i])), rmul(cb, pr[i]));
      nn += abs2(yr[i]);
      cfma_acc(dp, pr[i], yr[i]);
    }
    store_strip<T>(y, base, n, yr);
  }
  nn = wave_sum(nn);
  const acc_t<T> ds = wave_sum(dp);
  if (lane == 0) {
    red[wave][0] = nn;
    if constexpr (scalar_traits<T>::is_complex) {
      red[wave][1] = ds.re;
      red[wave][2] = ds.im;
    } else {
      red[wave][1] = ds;
    }
  }
  __syncthreads();
  // colmajor: column c of every workgroup contiguous (partials[c * grid + b]) — the form in which the next operator kernel
  // (ScaleIn) and pair_predict_kernel fold the columns themselves; else [b][1 + R] for reduce_cols_kernel
  if (tid < 1 + R)
    partials[colmajor ? (size_t)tid * gridDim.x + blockIdx.x : (size_t)blockIdx.x * (1 + R) + tid] =
        (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
template <typename T>
int launch_pair_three_term(int64_t n, T* y, const T* x, const T* p, double* e, const double* e_partials, int e_nparts,
                           const double* cx2, const double* cp2, double* partials, bool colmajor, hipStream_t s) {
  const int grid = strip_grid(n, strip<T>::ELEMS);
  hipLaunchKernelGGL((pair_three_term_kernel<T>), dim3(grid), dim3(kBlock), 0, s, n, y, x, p, e, e_partials, e_nparts, cx2, cp2,
                     partials, colmajor ? 1 : 0);
  LL_HIP(hipGetLastError());
  return grid;
}

// The stored-basis components of r4, predicted through the recorded tridiagonal (one workgroup; P coefficients each).
//   c1 = g1 / rho1, c2 = g2 / rho2 (S^H x1, S^H x2), <u_P, x2> = gam / rho2
//   p3 = T c2 [+ beta_{P-1} <u_P, x2> in the last row] - e1 c2 - rho2 c1                       (predicted S^H r3)
//   <u_P, r3> ~ (<r1, r3> - g1^H p3) / rho1
//   p4 = (T p3 [+ beta_{P-1} <u_P, r3> in the last row] - e2 p3) / |r3| - |r3| c2                (predicted S^H r4)
struct PairScalars {
  const double* rho1sq;
  const double* rho2sq;
  const double* gam;    // reals
  double* n3sq;         // |r3|^2, then <r1, r3> (reals) behind it
  const double* d13_partials;  // nullable: column-major partials of the three-term kernel ([1 + reals][nparts]); <r1, r3> is folded
  int d13_nparts;              // here into n3sq[1 ..] (|r3|^2 was folded by the second operator kernel, ScaleIn::c1_out)
  const double* e1;
  double* e2;
  const double* e2_partials;  // nullable: the second operator kernel's partial sums of <x3, A x3>, folded here into *e2
  int e2_nparts;
};
// Columns: L locked eigenvectors first (A z_i = lambda_i z_i + r_i: their image is lambda_i times the coefficient, the residual
// term is what LoopState::begin_pass gates), then the P Lanczos vectors u_0 .. u_{P-1}; K = L + P.
__global__ __launch_bounds__(256) void pair_predict_kernel(int P, int L, int reals, const double* __restrict__ g1,
                                                           const double* __restrict__ g2, PairScalars sc,
                                                           const double* __restrict__ hist_alpha,
                                                           const double* __restrict__ hist_beta,
                                                           const double* __restrict__ lambda, double* __restrict__ p3,
                                                           double* __restrict__ p4) {
  __shared__ double red[4];
  __shared__ double sh[2];
  const int tid = threadIdx.x;
  const double rho1 = sqrt(*sc.rho1sq), rho2 = sqrt(*sc.rho2sq), n3 = sqrt(sc.n3sq[0]);
  const double i1 = 1.0 / rho1, i2 = 1.0 / rho2, i3 = 1.0 / n3;
  double e2;
  if (sc.e2_partials) {  // (the order of reduce_one_kernel, like every other fold of these partials)
    __shared__ double fold_scratch[5];
    e2 = fold_partials_all(sc.e2_partials, sc.e2_nparts, fold_scratch);
    if (tid == 0) *sc.e2 = e2;
  } else {
    e2 = *sc.e2;
  }
  if (sc.d13_partials) {
    __shared__ double fold_scratch2[5];
    for (int q = 0; q < reals; ++q) {
      const double v = fold_partials_all(sc.d13_partials + (size_t)(1 + q) * sc.d13_nparts, sc.d13_nparts, fold_scratch2);
      if (tid == 0) sc.n3sq[1 + q] = v;
      __syncthreads();
    }
  }
  const double e1 = *sc.e1;
  const double bl = hist_beta[P - 1];  // couples u_{P-1} and u_P
  const int K = L + P;
  // p3
  for (int i = tid; i < reals * K; i += 256) {
    const int col = i / reals, q = i - col * reals;
    double t;
    if (col < L) {
      t = lambda[col] * g2[i];
    } else {
      const int j = col - L;
      t = hist_alpha[j] * g2[i];
      if (j >= 1) t = fma(hist_beta[j - 1], g2[i - reals], t);
      if (j + 1 < P) t = fma(hist_beta[j], g2[i + reals], t);
      else t = fma(bl, sc.gam[q], t);
    }
    t *= i2;                                     // T c2 (+ the neighbour behind the last stored vector)
    p3[i] = t - e1 * (g2[i] * i2) - rho2 * (g1[i] * i1);
  }
  __syncthreads();
  // <u_P, r3> = (<r1, r3> - g1^H p3) / rho1      (conj(g1) . p3)
  double are = 0.0, aim = 0.0;
  for (int j = tid; j < K; j += 256) {
    if (reals == 2) {
      const double gr = g1[2 * j], gi = g1[2 * j + 1], pr = p3[2 * j], pi = p3[2 * j + 1];
      are += gr * pr + gi * pi;
      aim += gr * pi - gi * pr;
    } else {
      are += g1[j] * p3[j];
    }
  }
  const double sre = block_sum(are, red);
  if (tid == 0) sh[0] = (sc.n3sq[1] - sre) * i1;
  if (reals == 2) {
    const double sim = block_sum(aim, red);
    if (tid == 0) sh[1] = (sc.n3sq[2] - sim) * i1;
  } else if (tid == 0) {
    sh[1] = 0.0;
  }
  __syncthreads();
  for (int i = tid; i < reals * K; i += 256) {
    const int col = i / reals, q = i - col * reals;
    double t;
    if (col < L) {
      t = lambda[col] * p3[i];
    } else {
      const int j = col - L;
      t = hist_alpha[j] * p3[i];
      if (j >= 1) t = fma(hist_beta[j - 1], p3[i - reals], t);
      if (j + 1 < P) t = fma(hist_beta[j], p3[i + reals], t);
      else t = fma(bl, sh[q], t);
    }
    p4[i] = (t - e2 * p3[i]) * i3 - n3 * (g2[i] * i2);
  }
}
void launch_pair_predict(int P, int L, int reals, const double* g1, const double* g2, const double* rho1sq, const double* rho2sq,
                         const double* gam, double* n3sq, const double* d13_partials, int d13_nparts, const double* e1, double* e2,
                         const double* e2_partials, int e2_nparts, const double* hist_alpha, const double* hist_beta,
                         const double* lambda, double* p3, double* p4, hipStream_t s) {
  const PairScalars sc{rho1sq, rho2sq, gam, n3sq, d13_partials, d13_nparts, e1, e2, e2_partials, e2_nparts};
  hipLaunchKernelGGL(pair_predict_kernel, dim3(1), dim3(256), 0, s, P, L, reals, g1, g2, sc, hist_alpha, hist_beta, lambda, p3, p4);
  LL_HIP(hipGetLastError());
}

// Address-space casts for the pipelined sweeps.  A pointer that reaches a load through a table or a lambda has lost what lets
// the compiler pick the cheap instruction: uniform reads of data no kernel writes while it runs (coefficients, the pointer table)
// go through the CONSTANT address space (s_load: scalar cache, no vmcnt slot — a vector load in the middle of a trip would be
// younger than the prefetched strips and turn the trip's wait into a full drain), strips through the GLOBAL one (global_load with
// an SGPR base instead of flat_load, which also occupies the LDS counter).
__device__ __forceinline__ double ld_const(const double* p, int i) {
  return reinterpret_cast<const __attribute__((address_space(4))) double*>(reinterpret_cast<uintptr_t>(p))[i];
}
template <typename T> __device__ __forceinline__ const T* ld_const_ptr(const T* const* tab, int i) {
  return reinterpret_cast<const T*>(reinterpret_cast<const __attribute__((address_space(4))) uintptr_t*>(reinterpret_cast<uintptr_t>(tab))[i]);
}
typedef unsigned int ll_u4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) char* ll_gcp;
typedef __attribute__((address_space(1))) char* ll_gp;
__device__ __forceinline__ uint4 ld_global16(const char* uniform_base, unsigned lane_off) {
  const ll_gcp g = (ll_gcp)uniform_base;  // generic -> global
  const ll_u4v v = *(const __attribute__((address_space(1))) ll_u4v*)(g + lane_off);
  uint4 r;
  __builtin_memcpy(&r, &v, sizeof(r));
  return r;
}
__device__ __forceinline__ void st_global16(char* uniform_base, unsigned lane_off, uint4 x) {
  const ll_gp g = (ll_gp)uniform_base;
  ll_u4v v;
  __builtin_memcpy(&v, &x, sizeof(v));
  *(__attribute__((address_space(1))) ll_u4v*)(g + lane_off) = v;
}
// One trip of the pair sweep: NV basis strips; two late updates, the compensation of r4, two measured column sets.
// nv <= NV of the strips are real (a prefix): the others are re-reads of the last real vector that the pipelined loop below issues
// to keep every trip's loads unconditional — their coefficients are zero (x - 0 u = x exactly) and their column sums are dropped.
template <typename T, int NV, int PC>
__device__ __forceinline__ void pair_trip_compute(const T (&ur)[NV][lstrip<T, PC>::EPT], int nv,
                                                  T (&a1)[lstrip<T, PC>::EPT], T (&a2)[lstrip<T, PC>::EPT],
                                                  const T (&b3)[lstrip<T, PC>::EPT], const T (&b4r)[lstrip<T, PC>::EPT],
                                                  T (&b4)[lstrip<T, PC>::EPT], const double* __restrict__ g1c,
                                                  const double* __restrict__ g2c, const double* __restrict__ p4c, double* mine3,
                                                  double* mine4, int lane) {
  constexpr int EPT = lstrip<T, PC>::EPT;
  double a3[NV], a4[NV], a3i[NV], a4i[NV];  // (imaginary parts: complex types only)
#pragma unroll
  for (int b = 0; b < NV; ++b) {
    // wave-uniform addresses in read-only memory: scalar loads, unconditional (a column beyond the real ones reads the last real
    // one's coefficients and zeroes them)
    acc_t<T> c1, c2, c4;
    const int bb = b < nv ? b : nv - 1;
    const bool real = b < nv;  // (uniform: scalar selects, the coefficients stay in SGPRs)
    if constexpr (scalar_traits<T>::is_complex) {
      const double x1 = ld_const(g1c, 2 * bb), y1 = ld_const(g1c, 2 * bb + 1), x2 = ld_const(g2c, 2 * bb), y2 = ld_const(g2c, 2 * bb + 1),
                   x4 = ld_const(p4c, 2 * bb), y4 = ld_const(p4c, 2 * bb + 1);
      c1 = zc{real ? x1 : 0.0, real ? y1 : 0.0};
      c2 = zc{real ? x2 : 0.0, real ? y2 : 0.0};
      c4 = zc{real ? x4 : 0.0, real ? y4 : 0.0};
    } else {
      const double x1 = ld_const(g1c, bb), x2 = ld_const(g2c, bb), x4 = ld_const(p4c, bb);
      c1 = real ? x1 : 0.0;
      c2 = real ? x2 : 0.0;
      c4 = real ? x4 : 0.0;
    }
    acc_t<T> s3 = zero<acc_t<T>>(), s4 = zero<acc_t<T>>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      fnma_acc(a1[e], c1, ur[b][e]);     // late update of u_P
      fnma_acc(a2[e], c2, ur[b][e]);     // late update of u_{P+1}
      fnma_acc(b4[e], c4, ur[b][e]);     // compensation of the next operator input
      cfma_acc(s3, ur[b][e], b3[e]);     // measured coefficients of r3 and of the raw r4
      cfma_acc(s4, ur[b][e], b4r[e]);
    }
    if constexpr (scalar_traits<T>::is_complex) {
      a3[b] = s3.re;
      a3i[b] = s3.im;
      a4[b] = s4.re;
      a4i[b] = s4.im;
    } else {
      a3[b] = s3;
      a4[b] = s4;
      a3i[b] = a4i[b] = 0.0;
    }
  }
  // (transposed reductions of at most NV = 4 sums each: with 8 or 16 sums at once the compiler sends part of the array through
  // scratch memory — a round trip with a full drain of the memory pipeline in every trip; checked in the ISA.  The butterfly adds
  // the lanes in the same order whatever NV and whatever the column's position in the trip: a column's bits do not depend on how
  // the stored vectors are cut into trips.)
  wave_sum_transposed<NV>(a3, lane);
  wave_sum_transposed<NV>(a4, lane);
  constexpr int LPI = 64 / NV;  // lanes that end up holding the same sum
  if constexpr (scalar_traits<T>::is_complex) {
    wave_sum_transposed<NV>(a3i, lane);
    wave_sum_transposed<NV>(a4i, lane);
    if ((lane & (LPI - 1)) == 0 && lane / LPI < nv) {
      const int b = lane / LPI;
      mine3[2 * b] += a3[0];
      mine3[2 * b + 1] += a3i[0];
      mine4[2 * b] += a4[0];
      mine4[2 * b + 1] += a4i[0];
    }
  } else {
    if ((lane & (LPI - 1)) == 0 && lane / LPI < nv) {
      mine3[lane / LPI] += a3[0];
      mine4[lane / LPI] += a4[0];
    }
  }
}
template <typename T, int NV, int PC>
__device__ __forceinline__ void pair_trip(const T* __restrict__ u0, int64_t ld, int64_t base, int64_t n,
                                          T (&a1)[lstrip<T, PC>::EPT], T (&a2)[lstrip<T, PC>::EPT],
                                          const T (&b3)[lstrip<T, PC>::EPT], const T (&b4r)[lstrip<T, PC>::EPT],
                                          T (&b4)[lstrip<T, PC>::EPT], const double* __restrict__ g1c,
                                          const double* __restrict__ g2c, const double* __restrict__ p4c, double* mine3,
                                          double* mine4, int lane) {
  constexpr int EPT = lstrip<T, PC>::EPT;
  T ur[NV][EPT];
#pragma unroll
  for (int b = 0; b < NV; ++b) load_lstrip<T, PC>(u0 + (int64_t)b * ld, base, n, ur[b]);
  pair_trip_compute<T, NV, PC>(ur, NV, a1, a2, b3, b4r, b4, g1c, g2c, p4c, mine3, mine4, lane);
}

// Partial columns per workgroup: [m3: R*P][m4: R*P][<u_P,r3>][<u_{P+1},r3>][<u_P,r4>][<u_{P+1},r4>][<r3,r4>] (R each) [|r4|^2].
template <typename T, int PC>
__global__ __launch_bounds__(kBlock) void pair_sweep_kernel(int64_t n, BasisSegs<T> segs, int P, int col0, int Pl, int flags,
                                                            const T* r1, const T* __restrict__ r2,   // (r1 may alias uP_out, see the
                                                            const T* __restrict__ r3, T* __restrict__ r4, T* uP_out,  // pipelined kernel)
                                                            T* __restrict__ uQ_out, T* __restrict__ part4,
                                                            const double* __restrict__ g1, const double* __restrict__ g2,
                                                            const double* __restrict__ gam, const double* __restrict__ p4,
                                                            const double* __restrict__ rho1sq, const double* __restrict__ rho2sq,
                                                            const double* __restrict__ e2, const double* __restrict__ n3sq,
                                                            double* __restrict__ partials) {
  // A sweep over more stored vectors than one workgroup's LDS holds columns for is SPLIT into launches over consecutive ranges of
  // the stored vectors (segs = vectors [col0, col0 + Pl) of the P stored ones; flags: kPairFirst / kPairLast).  Between launches the
  // two late updates travel through their basis slots (uP_out, uQ_out: unnormalised) and the partly compensated r4 through part4;
  // r4 itself keeps y2 until the last launch, which finishes everything.  Every coefficient column is summed in exactly one launch,
  // over the same strips by the same waves, and a strip written and read back is the same bits: the split changes no result.
  constexpr int EPT = lstrip<T, PC>::EPT;
  constexpr int ELEMS = lstrip<T, PC>::ELEMS;
  constexpr int JB = kJB;
  constexpr int R = scalar_traits<T>::reals;
  const bool first = (flags & kPairFirst) != 0, last = (flags & kPairLast) != 0;
  const int ncols = 2 * R * P + 5 * R + 1;               // columns of the whole sweep (layout of `partials`)
  const int lcols = 2 * R * Pl + (last ? 5 * R + 1 : 0);  // columns this launch sums
  extern __shared__ double lds[];  // [4 waves][lcols]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * lcols; i += kBlock) lds[i] = 0.0;
  const double s1 = 1.0 / sqrt(*rho1sq), s2 = 1.0 / sqrt(*rho2sq);
  // the buffer r4 holds y2 = A (r3 / |r3|) on entry: the second three-term update r4 = y2 - (e2 / |r3|) r3 - (|r3| / rho2) r2 is
  // formed here, from strips this sweep reads anyway (a separate kernel would move 4 more vectors)
  const double n3 = sqrt(*n3sq);
  const double ca = *e2 / n3, cb = n3 * s2;
  acc_t<T> gm;
  if constexpr (scalar_traits<T>::is_complex) gm = zc{gam[0], gam[1]};
  else gm = gam[0];
  __syncthreads();
  double* mine = lds + (size_t)wave * lcols;
  double* tail = mine + 2 * R * Pl;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * ELEMS;
    T a1[EPT], a2[EPT], b3[EPT], b4r[EPT], b4[EPT];
    load_lstrip<T, PC>(first ? r1 : uP_out, base, n, a1);
    load_lstrip<T, PC>(r2, base, n, a2);
    load_lstrip<T, PC>(r3, base, n, b3);
    load_lstrip<T, PC>(r4, base, n, b4r);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      b4r[e] = sub(sub(b4r[e], rmul(ca, b3[e])), rmul(cb, a2[e]));
      b4[e] = b4r[e];
    }
    if (!first) {  // (uniform) the late update of r2 and the compensated r4 as the launch before left them
      load_lstrip<T, PC>(uQ_out, base, n, a2);
      load_lstrip<T, PC>(part4, base, n, b4);
    }
    int col = R * col0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      int j = 0;
      for (; j + JB <= cnt; j += JB, col += R * JB)
        pair_trip<T, JB, PC>(ub + (int64_t)j * segs.ld, segs.ld, base, n, a1, a2, b3, b4r, b4, g1 + col, g2 + col, p4 + col,
                             mine + (col - R * col0), mine + R * Pl + (col - R * col0), lane);
      if (j + 2 <= cnt) {
        pair_trip<T, 2, PC>(ub + (int64_t)j * segs.ld, segs.ld, base, n, a1, a2, b3, b4r, b4, g1 + col, g2 + col, p4 + col,
                            mine + (col - R * col0), mine + R * Pl + (col - R * col0), lane);
        j += 2;
        col += R * 2;
      }
      if (j < cnt) {
        pair_trip<T, 1, PC>(ub + (int64_t)j * segs.ld, segs.ld, base, n, a1, a2, b3, b4r, b4, g1 + col, g2 + col, p4 + col,
                            mine + (col - R * col0), mine + R * Pl + (col - R * col0), lane);
        j += 1;
        col += R;
      }
    }
    if (!last) {  // (uniform) hand the three running strips to the next launch
      store_lstrip<T, PC>(uP_out, base, n, a1);
      store_lstrip<T, PC>(uQ_out, base, n, a2);
      store_lstrip<T, PC>(part4, base, n, b4);
      continue;
    }
    // u_P and u_{P+1} are complete: normalise, store; the in-strip coefficients and raw dots
    acc_t<T> t3p = zero<acc_t<T>>(), t3q = zero<acc_t<T>>(), t4p = zero<acc_t<T>>(), t4q = zero<acc_t<T>>(),
             d34 = zero<acc_t<T>>();
    double nn = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      a1[e] = rmul(s1, a1[e]);
      fnma_acc(a2[e], gm, a1[e]);
      a2[e] = rmul(s2, a2[e]);
      cfma_acc(t3p, a1[e], b3[e]);
      cfma_acc(t3q, a2[e], b3[e]);
      cfma_acc(t4p, a1[e], b4[e]);
      cfma_acc(t4q, a2[e], b4[e]);
      cfma_acc(d34, b3[e], b4[e]);
      nn += abs2(b4[e]);
    }
    store_lstrip<T, PC>(uP_out, base, n, a1);
    store_lstrip<T, PC>(uQ_out, base, n, a2);
    store_lstrip<T, PC>(r4, base, n, b4);
    const acc_t<T> sums[5] = {wave_sum(t3p), wave_sum(t3q), wave_sum(t4p), wave_sum(t4q), wave_sum(d34)};
    nn = wave_sum(nn);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        if constexpr (scalar_traits<T>::is_complex) {
          tail[2 * c] += sums[c].re;
          tail[2 * c + 1] += sums[c].im;
        } else {
          tail[c] += sums[c];
        }
      }
      tail[5 * R] += nn;
    }
  }
  __syncthreads();
  // this launch's columns into the sweep's layout: <u_j, r3> at R col0.., <u_j, r4> at R P + R col0.., the tail at 2 R P
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < lcols; i += kBlock) {
    const double v = (lds[i] + lds[lcols + i]) + (lds[2 * lcols + i] + lds[3 * lcols + i]);
    const int g = i < R * Pl ? R * col0 + i : (i < 2 * R * Pl ? R * P + R * col0 + (i - R * Pl) : 2 * R * P + (i - 2 * R * Pl));
    out[g] = v;
  }
}
// ---- the same sweep, software-pipelined (the production form; the kernel above is its A/B reference, key sweep_pipeline = 0)
// Unpipelined, every wave alternates between waiting for the 4 strips of its trip and 0.3 us of arithmetic on them, and the
// prologue / epilogue of every strip (4 raw strips in, 3 out, six wave reductions) is exposed in full: 5.26 TB/s where the chip
// streams 6.3.  Here the NEXT trip's strips are requested before the current trip is consumed — two register buffers with
// compile-time roles — so a wave always has a trip in flight while it computes.  What that takes:
//   * every trip requests the same JB loads, UNCONDITIONALLY and in straight-line code (the consuming trip's s_waitcnt then names
//     exactly the older trip; a load under a branch, divergent or not, makes the compiler drain the memory pipeline): whole
//     strips take this path (a uniform branch per strip; the vector's ragged last strip takes the guarded loads of the
//     reference kernel inside the same loop structure);
//   * the stored vectors are addressed through a device table of pointers (vtab[c] = column c: the locked eigenvectors, then
//     u_0, u_1, ...; written by fill_ptrs_kernel when a slab is added) instead of a walk over the segment list: one scalar load
//     per vector, trips run across slab boundaries, and a trip beyond the last stored vector re-reads the last one (a cache hit)
//     with zero coefficients and its column sums dropped (pair_trip_compute);
//   * a lane's address is a uniform base plus a 32-bit lane offset (global_load with an SGPR base): no 64-bit address
//     arithmetic per load.
// Same additions in the same order as the kernel above: identical bits (tests/test_gpu_pair.py compares the two).
template <typename T, int PC, bool FULL>
__device__ __forceinline__ void load_lstrip_u(const T* __restrict__ v, int64_t base, int64_t n, T (&r)[lstrip<T, PC>::EPT]) {
  if constexpr (FULL) {
    constexpr int EPT = lstrip<T, PC>::EPT;
    const char* sb = reinterpret_cast<const char*>(v + base);  // uniform
    const unsigned off = threadIdx.x * (unsigned)(EPT * sizeof(T));
    uint4 c[PC];
#pragma unroll
    for (int e = 0; e < PC; ++e) c[e] = ld_global16(sb, off + 16u * e);
    __builtin_memcpy(&r[0], c, sizeof(c));
  } else {
    load_lstrip<T, PC>(v, base, n, r);
  }
}
template <typename T, int PC, bool FULL>
__device__ __forceinline__ void store_lstrip_u(T* __restrict__ v, int64_t base, int64_t n, const T (&r)[lstrip<T, PC>::EPT]) {
  if constexpr (FULL) {
    constexpr int EPT = lstrip<T, PC>::EPT;
    char* sb = reinterpret_cast<char*>(v + base);
    const unsigned off = threadIdx.x * (unsigned)(EPT * sizeof(T));
    uint4 c[PC];
    __builtin_memcpy(c, &r[0], sizeof(c));
#pragma unroll
    for (int e = 0; e < PC; ++e) st_global16(sb, off + 16u * e, c[e]);
  } else {
    store_lstrip<T, PC>(v, base, n, r);
  }
}
template <typename T>
__global__ void fill_ptrs_kernel(const T** tab, int start, int count, const T* base, long long ld) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) tab[start + i] = base + (long long)i * ld;
}
template <typename T> void launch_fill_ptrs(const T** tab, int start, int count, const T* base, int64_t ld, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL((fill_ptrs_kernel<T>), dim3((count + 255) / 256), dim3(256), 0, s, tab, start, count, base, (long long)ld);
  LL_HIP(hipGetLastError());
}
constexpr int kPipeJB = 2;  // stored vectors per trip of the pipelined sweep (two trips resident: see the register budget in DESIGN.md 3.2)
template <typename T, int PC, int JB>
__global__ __launch_bounds__(kBlock) void pair_sweep_pipe_kernel(int64_t n, const T* const* __restrict__ vtab, int P, int col0, int Pl,
                                                                 int flags, const T* r1, const T* __restrict__ r2,
                                                                 const T* __restrict__ r3, T* __restrict__ r4, T* uP_out,
                                                                 T* __restrict__ uQ_out, T* __restrict__ part4,
                                                                 const double* __restrict__ g1, const double* __restrict__ g2,
                                                                 const double* __restrict__ gam, const double* __restrict__ p4,
                                                                 const double* __restrict__ rho1sq, const double* __restrict__ rho2sq,
                                                                 const double* __restrict__ e2, const double* __restrict__ n3sq,
                                                                 double* __restrict__ partials) {
  // (r1 and uP_out may be the SAME buffer — entering the pair form from the one-sweep state, u_{k-2} is already complete in its
  // slot and is "updated" with zero coefficients: every lane reads its strip before it writes it; neither is __restrict__)
  constexpr int EPT = lstrip<T, PC>::EPT;
  constexpr int ELEMS = lstrip<T, PC>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  const bool first = (flags & kPairFirst) != 0, last = (flags & kPairLast) != 0;
  const int ncols = 2 * R * P + 5 * R + 1;               // columns of the whole sweep (layout of `partials`)
  const int lcols = 2 * R * Pl + (last ? 5 * R + 1 : 0);  // columns this launch sums
  extern __shared__ double lds[];  // [4 waves][lcols]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * lcols; i += kBlock) lds[i] = 0.0;
  const double s1 = 1.0 / sqrt(*rho1sq), s2 = 1.0 / sqrt(*rho2sq);
  const double n3 = sqrt(*n3sq);
  const double ca = *e2 / n3, cb = n3 * s2;
  acc_t<T> gm;
  if constexpr (scalar_traits<T>::is_complex) gm = zc{gam[0], gam[1]};
  else gm = gam[0];
  __syncthreads();
  double* mine = lds + (size_t)wave * lcols;
  double* tail = mine + 2 * R * Pl;
  const T* const* tab = vtab + col0;
  const double *g1c = g1 + R * col0, *g2c = g2 + R * col0, *p4c = p4 + R * col0;
  const int ntrips = (Pl + JB - 1) / JB;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;

  auto do_strip = [&](auto full_c, const int64_t base) {
    constexpr bool FULL = decltype(full_c)::value;
    T a1[EPT], a2[EPT], b3[EPT], b4r[EPT], b4[EPT];
    load_lstrip_u<T, PC, FULL>(first ? r1 : uP_out, base, n, a1);
    load_lstrip_u<T, PC, FULL>(r2, base, n, a2);
    load_lstrip_u<T, PC, FULL>(r3, base, n, b3);
    load_lstrip_u<T, PC, FULL>(r4, base, n, b4r);
    auto issue = [&](T (&buf)[JB][EPT], int t) {
      const T* ptr[JB];
#pragma unroll
      for (int b = 0; b < JB; ++b) ptr[b] = ld_const_ptr<T>(tab, min(JB * t + b, Pl - 1));  // uniform; beyond the end: the last stored vector again
#pragma unroll
      for (int b = 0; b < JB; ++b) load_lstrip_u<T, PC, FULL>(ptr[b], base, n, buf[b]);
    };
    T ua[JB][EPT], ub[JB][EPT];
    if (ntrips > 0) {
      __builtin_amdgcn_sched_barrier(0);
      issue(ua, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      b4r[e] = sub(sub(b4r[e], rmul(ca, b3[e])), rmul(cb, a2[e]));
      b4[e] = b4r[e];
    }
    if (!first) {  // (uniform) the late update of r2 and the compensated r4 as the launch before left them
      load_lstrip_u<T, PC, FULL>(uQ_out, base, n, a2);
      load_lstrip_u<T, PC, FULL>(part4, base, n, b4);
    }
    for (int t = 0; t < ntrips; t += 2) {
      __builtin_amdgcn_sched_barrier(0);
      issue(ub, t + 1);
      __builtin_amdgcn_sched_barrier(0);
      pair_trip_compute<T, JB, PC>(ua, min(JB, Pl - JB * t), a1, a2, b3, b4r, b4, g1c + R * JB * t, g2c + R * JB * t, p4c + R * JB * t,
                                   mine + R * JB * t, mine + R * Pl + R * JB * t, lane);
      if (t + 1 >= ntrips) break;
      __builtin_amdgcn_sched_barrier(0);
      issue(ua, t + 2);
      __builtin_amdgcn_sched_barrier(0);
      pair_trip_compute<T, JB, PC>(ub, min(JB, Pl - JB * (t + 1)), a1, a2, b3, b4r, b4, g1c + R * JB * (t + 1), g2c + R * JB * (t + 1),
                                   p4c + R * JB * (t + 1), mine + R * JB * (t + 1), mine + R * Pl + R * JB * (t + 1), lane);
    }
    if (!last) {  // (uniform) hand the three running strips to the next launch
      store_lstrip_u<T, PC, FULL>(uP_out, base, n, a1);
      store_lstrip_u<T, PC, FULL>(uQ_out, base, n, a2);
      store_lstrip_u<T, PC, FULL>(part4, base, n, b4);
      return;
    }
    acc_t<T> t3p = zero<acc_t<T>>(), t3q = zero<acc_t<T>>(), t4p = zero<acc_t<T>>(), t4q = zero<acc_t<T>>(),
             d34 = zero<acc_t<T>>();
    double nn = 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      a1[e] = rmul(s1, a1[e]);
      fnma_acc(a2[e], gm, a1[e]);
      a2[e] = rmul(s2, a2[e]);
      cfma_acc(t3p, a1[e], b3[e]);
      cfma_acc(t3q, a2[e], b3[e]);
      cfma_acc(t4p, a1[e], b4[e]);
      cfma_acc(t4q, a2[e], b4[e]);
      cfma_acc(d34, b3[e], b4[e]);
      nn += abs2(b4[e]);
    }
    store_lstrip_u<T, PC, FULL>(uP_out, base, n, a1);
    store_lstrip_u<T, PC, FULL>(uQ_out, base, n, a2);
    store_lstrip_u<T, PC, FULL>(r4, base, n, b4);
    const acc_t<T> sums[5] = {wave_sum(t3p), wave_sum(t3q), wave_sum(t4p), wave_sum(t4q), wave_sum(d34)};
    nn = wave_sum(nn);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        if constexpr (scalar_traits<T>::is_complex) {
          tail[2 * c] += sums[c].re;
          tail[2 * c + 1] += sums[c].im;
        } else {
          tail[c] += sums[c];
        }
      }
      tail[5 * R] += nn;
    }
  };
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * ELEMS;
    if (base + ELEMS <= n) do_strip(std::true_type{}, base);
    else do_strip(std::false_type{}, base);
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < lcols; i += kBlock) {
    const double v = (lds[i] + lds[lcols + i]) + (lds[2 * lcols + i] + lds[3 * lcols + i]);
    const int g = i < R * Pl ? R * col0 + i : (i < 2 * R * Pl ? R * P + R * col0 + (i - R * Pl) : 2 * R * P + (i - 2 * R * Pl));
    out[g] = v;
  }
}
// groups: the stored vectors in launch order (every group within pair_sweep_max_vecs<T>() vectors and kMaxSegs segments);
// part4: an n-vector of scratch, needed (and touched) only when there is more than one group.
template <typename T>
int launch_pair_sweep(int64_t n, const std::vector<BasisSegs<T>>& groups, int P, const T* r1, const T* r2, const T* r3, T* r4,
                      T* uP_out, T* uQ_out, T* part4, const double* g1, const double* g2, const double* gam, const double* p4,
                      const double* rho1sq, const double* rho2sq, const double* e2, const double* n3sq, double* partials, int pieces,
                      hipStream_t s, const T* const* vtab, bool force_pipeline) {
  constexpr int R = scalar_traits<T>::reals;
  const int64_t strips16k = (n * (int64_t)sizeof(T) + 16383) / 16384;
  int pc = strips16k >= kLaggedFullStrips ? 4 : 2;
  if (pieces == 2 || pieces == 4) pc = pieces;
  const int grid = pc == 4 ? strip_grid(n, lstrip<T, 4>::ELEMS) : strip_grid(n, lstrip<T, 2>::ELEMS);
  BasisSegs<T> none;
  none.nseg = 0;
  none.ld = groups.empty() ? 0 : groups[0].ld;
  const size_t ng = std::max<size_t>(groups.size(), 1);
  int col0 = 0;
  for (size_t gi = 0; gi < ng; ++gi) {
    const BasisSegs<T>& segs = groups.empty() ? none : groups[gi];
    int Pl = 0;
    for (int i = 0; i < segs.nseg; ++i) Pl += segs.count[i];
    const int flags = (gi == 0 ? kPairFirst : 0) | (gi + 1 == ng ? kPairLast : 0);
    const size_t lds_bytes = (size_t)4 * (size_t)(2 * R * Pl + ((flags & kPairLast) ? 5 * R + 1 : 0)) * sizeof(double);
    // The software-pipelined form where the sweep is a STREAM: vectors of more than ~9 MiB, every workgroup walking several strips
    // back to back (strip_grid's one-workgroup-per-CU mode).  Config 3 (80 MB vectors, k <= 300): 822 -> 808 us per sweep.  Shorter
    // vectors have one strip per workgroup and more workgroups than CUs: their sweeps are latency chains of k / JB trips, and two
    // vectors per trip instead of four cost more than the prefetch brings — config 2 (8 MB vectors, 3 368 iterations to
    // convergence): 4.76 s of sweeps with the reference kernel, 5.09 s pipelined (profiles/r06_pair_sweep_pipeline_ab.txt).
    const bool streaming = force_pipeline || strips16k > 2 * kCUs + kCUs / 4;  // (force: key sweep_pipeline = 2, parity tests on small cases)
    if (vtab != nullptr && streaming) {  // the stored vectors through the pointer table (columns [col0, col0 + Pl))
      if (pc == 4)
        hipLaunchKernelGGL((pair_sweep_pipe_kernel<T, 4, kPipeJB>), dim3(grid), dim3(kBlock), lds_bytes, s, n, vtab, P, col0, Pl, flags, r1, r2, r3,
                           r4, uP_out, uQ_out, part4, g1, g2, gam, p4, rho1sq, rho2sq, e2, n3sq, partials);
      else
        hipLaunchKernelGGL((pair_sweep_pipe_kernel<T, 2, kPipeJB>), dim3(grid), dim3(kBlock), lds_bytes, s, n, vtab, P, col0, Pl, flags, r1, r2, r3,
                           r4, uP_out, uQ_out, part4, g1, g2, gam, p4, rho1sq, rho2sq, e2, n3sq, partials);
    } else if (pc == 4) {
      hipLaunchKernelGGL((pair_sweep_kernel<T, 4>), dim3(grid), dim3(kBlock), lds_bytes, s, n, segs, P, col0, Pl, flags, r1, r2, r3, r4,
                         uP_out, uQ_out, part4, g1, g2, gam, p4, rho1sq, rho2sq, e2, n3sq, partials);
    } else {
      hipLaunchKernelGGL((pair_sweep_kernel<T, 2>), dim3(grid), dim3(kBlock), lds_bytes, s, n, segs, P, col0, Pl, flags, r1, r2, r3, r4,
                         uP_out, uQ_out, part4, g1, g2, gam, p4, rho1sq, rho2sq, e2, n3sq, partials);
    }
    LL_HIP(hipGetLastError());
    col0 += Pl;
  }
  return grid;
}

// The fold of a pair (one workgroup).  m: the 2 R P + 5 R + 1 folded columns of the sweep.  Outputs:
//   rec3 = g3 (R (K+2): coefficients of r3 against the K = L + P stored columns, u_P, u_{P+1}),  rec4 = g4 (R (K+2)) followed by
//   gam' = <u_{P+2}, r4>
//   nxt[0] = rho3^2, nxt[1] = rho4^2 (the next pair's rho1^2, rho2^2)
//   hist_alpha[P+1], hist_alpha[P+2], hist_beta[P+1] = rho3, hist_beta[P+2] = rho4
//   host slots of the two iterations (alpha, beta^2, ||w||^2 before, after) and, for each, its gate value: the largest
//   coefficient of the iteration's raw vector relative to that vector.
__device__ __forceinline__ double pair_tri_row(const double* __restrict__ ha, const double* __restrict__ hb,
                                               const double* __restrict__ lambda, const double* v, int i, int reals, int L, int m,
                                               double alpha_last) {
  // entry i of the image of E = sum v_col (vector col) under the operator, expressed in the same columns: lambda_col v for a
  // locked eigenvector, row j of (T v) for the first m Lanczos vectors behind them; alpha_{m-1} may not be recorded yet
  const int col = i / reals;
  if (col < L) return lambda[col] * v[i];
  const int j = col - L;
  double t = (j == m - 1 ? alpha_last : ha[j]) * v[i];
  if (j >= 1) t = fma(hb[j - 1], v[i - reals], t);
  if (j + 1 < m) t = fma(hb[j], v[i + reals], t);
  return t;
}
__global__ __launch_bounds__(256) void pair_fold_kernel(const double* __restrict__ m, int P, int L, int reals,
                                                        const double* __restrict__ lambda,
                                                        const double* __restrict__ p4, const double* __restrict__ g2,
                                                        const double* __restrict__ gam, const double* __restrict__ rho2sq,
                                                        const double* __restrict__ n3sq_p, const double* __restrict__ e1p,
                                                        const double* __restrict__ e2p, double* __restrict__ rec3,
                                                        double* __restrict__ rec4, double* __restrict__ nxt,
                                                        double* __restrict__ hist_alpha, double* __restrict__ hist_beta,
                                                        double* __restrict__ scratch, double* __restrict__ host_a,
                                                        double* __restrict__ host_b, double* __restrict__ gate_a,
                                                        double* __restrict__ gate_b) {
  __shared__ double red[4];
  __shared__ double sh[8];
  const int tid = threadIdx.x;
  const int K = L + P;  // stored columns: L locked eigenvectors, then u_0 .. u_{P-1}
  const int RP = reals * K, M = reals * (K + 2);
  const double* tail = m + 2 * RP;
  const double n3sq = n3sq_p[0], n4sq = tail[5 * reals];
  // ---- g3, g4; |g3|^2, |g4|^2, g3^H g4, largest coefficients
  double s33 = 0.0, s44 = 0.0, s34r = 0.0, s34i = 0.0, mx3 = 0.0, mx4 = 0.0;
  for (int i = tid; i < M; i += 256) {
    double a, b;
    if (i < RP) {
      a = m[i];
      b = m[RP + i] - p4[i];
    } else {
      a = tail[i - RP];                 // <u_P, r3>, <u_{P+1}, r3>
      b = tail[2 * reals + (i - RP)];   // <u_P, r4>, <u_{P+1}, r4>
    }
    rec3[i] = a;
    rec4[i] = b;
    s33 = fma(a, a, s33);
    s44 = fma(b, b, s44);
    mx3 = fmax(mx3, fabs(a));
    mx4 = fmax(mx4, fabs(b));
  }
  __syncthreads();
  for (int j = tid; j < K + 2; j += 256) {  // conj(g3) . g4
    if (reals == 2) {
      const double ar = rec3[2 * j], ai = rec3[2 * j + 1], br = rec4[2 * j], bi = rec4[2 * j + 1];
      s34r += ar * br + ai * bi;
      s34i += ar * bi - ai * br;
    } else {
      s34r += rec3[j] * rec4[j];
    }
  }
  const double t33 = block_sum(s33, red);
  if (tid == 0) sh[0] = t33;
  const double t44 = block_sum(s44, red);
  if (tid == 0) sh[1] = t44;
  const double t34r = block_sum(s34r, red);
  if (tid == 0) sh[2] = t34r;
  const double t34i = block_sum(s34i, red);
  if (tid == 0) sh[3] = t34i;
  // block maxima (sums of non-negative numbers are not maxima: fold with fmax through LDS)
  __syncthreads();
  {
    double v3 = mx3, v4 = mx4;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      v3 = fmax(v3, __shfl_down(v3, d, 64));
      v4 = fmax(v4, __shfl_down(v4, d, 64));
    }
    __shared__ double mxs[2][4];
    if ((tid & 63) == 0) {
      mxs[0][tid >> 6] = v3;
      mxs[1][tid >> 6] = v4;
    }
    __syncthreads();
    if (tid == 0) {
      sh[4] = fmax(fmax(mxs[0][0], mxs[0][1]), fmax(mxs[0][2], mxs[0][3]));
      sh[5] = fmax(fmax(mxs[1][0], mxs[1][1]), fmax(mxs[1][2], mxs[1][3]));
    }
  }
  __syncthreads();
  // ---- quadratic terms through the recorded tridiagonal
  //   alpha_{P+1}: v = [g2 / rho2; gam / rho2] over u_0 .. u_P     (alpha_0 .. alpha_P, beta_0 .. beta_{P-1} recorded)
  const double rho2 = sqrt(*rho2sq), i2 = 1.0 / rho2;
  double* v = scratch;  // reals * (K + 1)
  for (int i = tid; i < reals * (K + 1); i += 256) v[i] = (i < RP ? g2[i] : gam[i - RP]) * i2;
  __syncthreads();
  double qa = 0.0;
  for (int i = tid; i < reals * (K + 1); i += 256)
    qa = fma(v[i], pair_tri_row(hist_alpha, hist_beta, lambda, v, i, reals, L, P + 1, hist_alpha[P]), qa);
  const double quad_a = block_sum(qa, red);
  if (tid == 0) {
    const double alpha_q = *e1p - 2.0 * gam[0] - quad_a;   // gam[0] = Re <u_P, r2>
    sh[6] = alpha_q;
    hist_alpha[P + 1] = alpha_q;
  }
  __syncthreads();
  //   alpha_{P+2}: <r3, A r3> = rho3^2 alpha + 2 rho3^2 Re <u_{P+1}, r3> + <E, A E>, E = sum g3_j u_j over u_0 .. u_{P+1}
  double qb = 0.0;
  for (int i = tid; i < M; i += 256) qb = fma(rec3[i], pair_tri_row(hist_alpha, hist_beta, lambda, rec3, i, reals, L, P + 2, sh[6]), qb);
  const double quad_b = block_sum(qb, red);
  if (tid == 0) {
    double rho3sq = n3sq - sh[0];
    rho3sq = rho3sq > 0.0 ? rho3sq : 0.0;
    const double rho3 = sqrt(rho3sq), i3 = rho3 > 0.0 ? 1.0 / rho3 : 0.0;
    const double gre = (tail[4 * reals] - sh[2]) * i3;                      // gam' = (<r3, r4> - g3^H g4) / rho3
    const double gim = reals == 2 ? (tail[4 * reals + 1] - sh[3]) * i3 : 0.0;
    double rho4sq = n4sq - sh[1] - (gre * gre + gim * gim);
    rho4sq = rho4sq > 0.0 ? rho4sq : 0.0;
    const double alpha_n = rho3sq > 0.0 ? (*e2p * n3sq - 2.0 * rho3sq * rec3[reals * (K + 1)] - quad_b) / rho3sq : 0.0;
    rec4[M] = gre;
    if (reals == 2) rec4[M + 1] = gim;
    nxt[0] = rho3sq;
    nxt[1] = rho4sq;
    hist_alpha[P + 2] = alpha_n;
    hist_beta[P + 1] = rho3;
    hist_beta[P + 2] = sqrt(rho4sq);
    // the largest coefficient of each raw vector relative to the vector: what the host's gate (kPairGate) looks at.  r3's decides
    // whether the SECOND iteration of this pair stands (its operator input was r3), r4's whether the next pair may build on it.
    const double gate3 = n3sq > 0.0 ? sh[4] / sqrt(n3sq) : 1.0;
    const double gate4 = n4sq > 0.0 ? fmax(sh[5], sqrt(gre * gre + gim * gim)) / sqrt(n4sq) : 1.0;
    host_a[0] = sh[6];
    host_a[1] = rho3sq;
    host_a[2] = n3sq;
    host_a[3] = rho3sq;
    *gate_a = gate3;
    host_b[0] = alpha_n;
    host_b[1] = rho4sq;
    host_b[2] = n4sq;
    host_b[3] = rho4sq;
    *gate_b = gate4;
  }
}
void launch_pair_fold(const double* m, int P, int L, int reals, const double* lambda, const double* p4, const double* g2, const double* gam,
                      const double* rho2sq, const double* n3sq, const double* e1, const double* e2, double* rec3, double* rec4,
                      double* nxt, double* hist_alpha, double* hist_beta, double* scratch, double* host_a, double* host_b,
                      double* gate_a, double* gate_b, hipStream_t s, hipEvent_t stop) {
  LL_LAUNCH_STOP(stop, pair_fold_kernel, dim3(1), dim3(256), 0, s, m, P, L, reals, lambda, p4, g2, gam, rho2sq, n3sq, e1, e2, rec3, rec4, nxt,
                 hist_alpha, hist_beta, scratch, host_a, host_b, gate_a, gate_b);
  LL_HIP(hipGetLastError());
}
#define LL_INST_PAIR(T)                                                                                                          \
  template int launch_pair_three_term<T>(int64_t, T*, const T*, const T*, double*, const double*, int, const double*,           \
                                         const double*, double*, bool, hipStream_t);                                             \
  template int launch_pair_sweep<T>(int64_t, const std::vector<BasisSegs<T>>&, int, const T*, const T*, const T*, T*, T*, T*, T*, \
                                    const double*, const double*, const double*, const double*, const double*, const double*,    \
                                    const double*, const double*, double*, int, hipStream_t, const T* const*, bool);              \
  template void launch_fill_ptrs<T>(const T**, int, int, const T*, int64_t, hipStream_t);
LL_INST_PAIR(double) LL_INST_PAIR(zc) LL_INST_PAIR(float) LL_INST_PAIR(cf)

// ================================================================= small-vector Gram-Schmidt kernels (vectors < 4 MiB)
// With few strips the streaming kernels above are a latency / instruction chain: ONE wave walks all k basis vectors of
// its strip (n = 1e4, k = 100: 28 us for 8 MB that the chip reads in under 7 us, tools/small_strip_probe.hip).  Here a
// workgroup is four waves on the SAME strip of 64 lanes x 16 B (n = 1e4 doubles: 79 workgroups instead of 5); the trips
// of kSmallJB basis vectors are dealt round-robin to the waves, so each wave walks a quarter of the basis:
//   multi-dot : every basis vector belongs to exactly one wave -> no cross-wave sums; the kSmallJB (x2) per-lane
//               partial products of a trip are transposed through a per-wave LDS tile and each column is summed by
//               four lanes (16 reads + 2 quad shuffles instead of 6 dependent shuffle steps per vector);
//   multi-axpy: every wave accumulates its share of sum_j h_j u_j, wave 0 adds the four shares in a fixed order,
//               updates w and accumulates ||w||^2.
// All sums have a fixed order: bit-reproducible like the streaming kernels (the two geometries differ from each other
// in the last bits, each is deterministic).
constexpr int kSmallJB = 8;
constexpr int kSmallTileRow = 65;  // doubles per row of the transpose tile (64 lanes + 1: conflict-free columns)

template <typename T> struct small_geom {
  static constexpr int EPT = (int)(16 / sizeof(T));  // 16 B per lane: 2 double / cf, 1 zc, 4 float
  static constexpr int ELEMS = 64 * EPT;
};

template <typename T>
__device__ __forceinline__ void load_small(const T* __restrict__ v, int64_t i0, int64_t n, T (&r)[small_geom<T>::EPT]) {
  constexpr int EPT = small_geom<T>::EPT;
  if (i0 + EPT <= n) {
    const uint4 c = *reinterpret_cast<const uint4*>(v + i0);
    __builtin_memcpy(&r[0], &c, sizeof(c));
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = (i0 + e < n) ? v[i0 + e] : zero<T>();
  }
}
template <typename T>
__device__ __forceinline__ void store_small(T* __restrict__ v, int64_t i0, int64_t n, const T (&r)[small_geom<T>::EPT]) {
  constexpr int EPT = small_geom<T>::EPT;
  if (i0 + EPT <= n) {
    uint4 c;
    __builtin_memcpy(&c, &r[0], sizeof(c));
    *reinterpret_cast<uint4*>(v + i0) = c;
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (i0 + e < n) v[i0 + e] = r[e];
  }
}
// LDS traffic between the lanes of ONE wave: the hardware executes a wave's LDS instructions in order; these keep the
// compiler from moving accesses across the hand-over point.
__device__ __forceinline__ void wave_lds_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mdot_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs, ThreeTerm<T> tt,
                                                            NormRefs pred, int predicated, double* __restrict__ partials,
                                                            int ncols) {
  constexpr int EPT = small_geom<T>::EPT;
  constexpr int ELEMS = small_geom<T>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  constexpr int NA = kSmallJB * R;  // accumulators per trip: 8 or 16
  extern __shared__ double lds[];   // [ncols] column sums of the workgroup, then one [16][65] transpose tile per wave
  if (predicated && !second_pass_due(pred)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cols = lds;
  double* tile = lds + ((ncols + 15) & ~15) + wave * (16 * kSmallTileRow);
  for (int i = tid; i < ncols; i += kBlock) cols[i] = 0.0;
  __syncthreads();

  double alpha = 0.0, beta = 0.0;
  const bool do_tt = tt.u_cur != nullptr;
  if (do_tt) {
    if (tt.alpha_partials) {  // deferred alpha (ThreeTerm)
      __shared__ double fold_scratch[5];
      alpha = fold_partials_all(tt.alpha_partials, tt.alpha_nparts, fold_scratch);
      if (blockIdx.x == 0 && tid == 0) *tt.alpha_out = alpha;
    } else {
      alpha = *tt.alpha;
    }
    if (tt.u_prev) beta = sqrt(final_norm2(tt.prev));
  }
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {  // same trip count for every wave of the workgroup
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    T wr[EPT];
    load_small<T>(w, i0, n, wr);
    if (do_tt) {  // every wave forms the same three-term strip; wave 0 stores it once all four have read w
      T uc[EPT];
      load_small<T>(tt.u_cur, i0, n, uc);
      if (tt.u_prev) {
        T up[EPT];
        load_small<T>(tt.u_prev, i0, n, up);
#pragma unroll
        for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, up[e])), rmul(alpha, uc[e]));
      } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, uc[e]));
      }
      __syncthreads();
      if (wave == 0) store_small<T>(w, i0, n, wr);
    }
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_small<T>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b) {
          acc_t<T> acc = zero<acc_t<T>>();
          if (b < nv) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) cfma_acc(acc, ur[b][e], wr[e]);
          }
          if constexpr (scalar_traits<T>::is_complex) {
            tile[(2 * b) * kSmallTileRow + lane] = acc.re;
            tile[(2 * b + 1) * kSmallTileRow + lane] = acc.im;
          } else {
            tile[b * kSmallTileRow + lane] = acc;
          }
        }
        wave_lds_handover();
        // column i of the tile (16 slots, NA of them used) is summed by the four lanes 4i .. 4i+3, 16 entries each
        const int i = lane >> 2, q = lane & 3;
        double sum = 0.0;
        if (i < nv * R) {
          const double* row = tile + i * kSmallTileRow + q * 16;
#pragma unroll
          for (int t = 0; t < 16; ++t) sum += row[t];
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if (q == 0 && i < nv * R) cols[col0 + R * j + i] += sum;  // this column belongs to this wave alone
        wave_lds_handover();
        (void)NA;
      }
      col0 += R * cnt;
    }
    if (wave == 0) {
      double nn = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) nn += abs2(wr[e]);
      nn = wave_sum(nn);
      if (lane == 0) cols[ncols - 1] += nn;
    }
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock) out[i] = cols[i];
}

// dst[j] = sum_b partials[b * ncols + j], j < ncols, formed by the WHOLE workgroup in exactly the order of
// reduce_cols_kernel (16 columns x 16 row lanes per pass, four chains per lane, rows folded 0..15): the fold of the
// multi-dot's partials without its launch, for grids small enough that every workgroup can afford to redo it.
__device__ __forceinline__ void fold_cols_into_lds(const double* __restrict__ partials, int nparts, int ncols, double* dst) {
  __shared__ double sm[16][17];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  for (int j0 = 0; j0 < ncols; j0 += 16) {
    const int j = j0 + cx;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (j < ncols) {
      int b = ry;
      for (; b + 48 < nparts; b += 64) {
        a0 += partials[(size_t)b * ncols + j];
        a1 += partials[(size_t)(b + 16) * ncols + j];
        a2 += partials[(size_t)(b + 32) * ncols + j];
        a3 += partials[(size_t)(b + 48) * ncols + j];
      }
      for (; b < nparts; b += 16) a0 += partials[(size_t)b * ncols + j];
    }
    __syncthreads();  // the previous pass has been read out
    sm[ry][cx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ry == 0 && j < ncols) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += sm[r][cx];
      dst[j] = t;
    }
  }
  __syncthreads();
}

// FOLD: h is not given; the kernel folds the multi-dot's partials `mp` ([mparts][R*nb + 1]: coefficients, then ||w||^2)
// itself — every workgroup, same order — and workgroup 0 stores the coefficients to h_out and ||w||^2 to *c0_out.
template <typename T, bool FOLD>
__global__ __launch_bounds__(kBlock) void maxpy_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs,
                                                             const double* __restrict__ h, int nb, NormRefs pred,
                                                             int predicated, double* __restrict__ partials,
                                                             const double* __restrict__ mp, int mparts,
                                                             double* __restrict__ h_out, double* __restrict__ c0_out) {
  constexpr int EPT = small_geom<T>::EPT;
  constexpr int ELEMS = small_geom<T>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  extern __shared__ double lds[];  // [R*nb (+1)] coefficients, then the four waves' shares [4][64][EPT*R]
  if (predicated && !second_pass_due(pred)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (FOLD) {
    fold_cols_into_lds(mp, mparts, R * nb + 1, lds);
    if (blockIdx.x == 0) {
      for (int i = tid; i < R * nb; i += kBlock) h_out[i] = lds[i];
      if (tid == 0 && c0_out) *c0_out = lds[R * nb];
    }
  } else {
    for (int i = tid; i < R * nb; i += kBlock) lds[i] = h[i];
  }
  double* share = lds + ((R * nb + 1 + 15) & ~15);
  __syncthreads();
  double nn = 0.0;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    acc_t<T> delta[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) delta[e] = zero<acc_t<T>>();
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_small<T>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) {
            const double* hc = lds + col0 + R * (j + b);
            acc_t<T> hj;
            if constexpr (scalar_traits<T>::is_complex) hj = zc{hc[0], hc[1]};
            else hj = hc[0];
#pragma unroll
            for (int e = 0; e < EPT; ++e) fma_acc(delta[e], hj, to_acc(ur[b][e]));
          }
      }
      col0 += R * cnt;
    }
    double* mine = share + ((size_t)wave * 64 + lane) * (EPT * R);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if constexpr (scalar_traits<T>::is_complex) {
        mine[2 * e] = delta[e].re;
        mine[2 * e + 1] = delta[e].im;
      } else {
        mine[e] = delta[e];
      }
    }
    __syncthreads();
    if (wave == 0) {
      T wr[EPT];
      load_small<T>(w, i0, n, wr);
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        acc_t<T> tot;
        const double* s0 = share + ((size_t)0 * 64 + lane) * (EPT * R);
        const double* s1 = share + ((size_t)1 * 64 + lane) * (EPT * R);
        const double* s2 = share + ((size_t)2 * 64 + lane) * (EPT * R);
        const double* s3 = share + ((size_t)3 * 64 + lane) * (EPT * R);
        if constexpr (scalar_traits<T>::is_complex)
          tot = zc{(s0[2 * e] + s1[2 * e]) + (s2[2 * e] + s3[2 * e]), (s0[2 * e + 1] + s1[2 * e + 1]) + (s2[2 * e + 1] + s3[2 * e + 1])};
        else
          tot = (s0[e] + s1[e]) + (s2[e] + s3[e]);
        wr[e] = narrow<T>(sub(to_acc(wr[e]), tot));
      }
      store_small<T>(w, i0, n, wr);
#pragma unroll
      for (int e = 0; e < EPT; ++e) nn += abs2(wr[e]);
    }
    __syncthreads();  // the shares are rewritten by the next strip
  }
  if (wave == 0) {
    const double tot = wave_sum(nn);
    if (lane == 0) partials[blockIdx.x] = tot;
  }
}


int small_lagged_lds_doubles(int ncols, int ept_times_reals) {
  return ((ncols + 15) & ~15) + 4 * 16 * kSmallTileRow + 2 * kBlock * ept_times_reals;
}
// One-sweep Gram-Schmidt (lagged_kernel's algebra, see there) in the SMALL-VECTOR geometry: four waves share a strip of
// 64 lanes x 16 B and split the basis between them (trips of kSmallJB vectors dealt round-robin).  Every wave takes the
// coefficients <u_j, wr> of its vectors (LDS-transposed column sums, as in mdot_small_kernel) and accumulates its share
// of sum g_j u_j (late update of u_{k-1}) and of sum d_j u_j (compensation of w); wave 0 adds the four shares in a fixed
// order (as in maxpy_small_kernel), finishes u_{k-1} and w, and takes the last coefficient and ||w||^2.
template <typename T>
__global__ __launch_bounds__(kBlock) void lagged_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs, int nb,
                                                              Lagged<T> lg, const double* __restrict__ g,
                                                              const double* __restrict__ t, ThreeTerm<T> tt,
                                                              double* __restrict__ partials) {
  constexpr int EPT = small_geom<T>::EPT;
  constexpr int ELEMS = small_geom<T>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = R * (nb + 1) + 1;
  extern __shared__ double lds[];  // [ncols] column sums, one [16][65] tile per wave, the waves' shares of the two updates
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cols = lds;
  double* tile = lds + ((ncols + 15) & ~15) + wave * (16 * kSmallTileRow);
  double* share_u = lds + ((ncols + 15) & ~15) + 4 * (16 * kSmallTileRow);
  double* share_w = share_u + (size_t)kBlock * EPT * R;
  for (int i = tid; i < ncols; i += kBlock) cols[i] = 0.0;
  double alpha;
  if (tt.alpha_partials) {
    __shared__ double fold_scratch[5];
    alpha = fold_partials_all(tt.alpha_partials, tt.alpha_nparts, fold_scratch);
    if (blockIdx.x == 0 && tid == 0) *tt.alpha_out = alpha;  // as measured; lagged_fold_kernel corrects it in place
  } else {
    alpha = *tt.alpha;
  }
  alpha = lagged_alpha(alpha, g[R * (nb - 1)], t[R * (nb + 1)]);
  const double beta = sqrt(*lg.beta2), s = 1.0 / beta;
  const double as = alpha * s;
  acc_t<T> dlast;
  if constexpr (scalar_traits<T>::is_complex) dlast = zc{t[R * nb], t[R * nb + 1]};
  else dlast = t[R * nb];
  __syncthreads();

  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {  // same trip count for every wave of the workgroup
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    T wr[EPT], rr[EPT];
    load_small<T>(w, i0, n, wr);
    load_small<T>(lg.r, i0, n, rr);
    if (tt.u_prev) {
      T up[EPT];
      load_small<T>(tt.u_prev, i0, n, up);
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, up[e])), rmul(alpha, rmul(s, rr[e])));
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, rmul(s, rr[e])));
    }
    acc_t<T> du[EPT], dw[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      du[e] = zero<acc_t<T>>();
      dw[e] = zero<acc_t<T>>();
    }
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_small<T>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b) {
          acc_t<T> acc = zero<acc_t<T>>();
          if (b < nv) {
            const double* gc = g + col0 + R * (j + b);
            const double* tc = t + col0 + R * (j + b);
            acc_t<T> gj, dj;
            if constexpr (scalar_traits<T>::is_complex) {
              gj = zc{gc[0], gc[1]};
              dj = zc{fma(-as, gj.re, tc[0]), fma(-as, gj.im, tc[1])};
            } else {
              gj = gc[0];
              dj = fma(-as, gj, tc[0]);
            }
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
              cfma_acc(acc, ur[b][e], wr[e]);
              fma_acc(du[e], gj, to_acc(ur[b][e]));
              fma_acc(dw[e], dj, to_acc(ur[b][e]));
            }
          }
          if constexpr (scalar_traits<T>::is_complex) {
            tile[(2 * b) * kSmallTileRow + lane] = acc.re;
            tile[(2 * b + 1) * kSmallTileRow + lane] = acc.im;
          } else {
            tile[b * kSmallTileRow + lane] = acc;
          }
        }
        wave_lds_handover();
        const int i = lane >> 2, q = lane & 3;
        double sum = 0.0;
        if (i < nv * R) {
          const double* row = tile + i * kSmallTileRow + q * 16;
#pragma unroll
          for (int tt2 = 0; tt2 < 16; ++tt2) sum += row[tt2];
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if (q == 0 && i < nv * R) cols[col0 + R * j + i] += sum;  // this column belongs to this wave alone
        wave_lds_handover();
      }
      col0 += R * cnt;
    }
    double* mu = share_u + ((size_t)wave * 64 + lane) * (EPT * R);
    double* mw = share_w + ((size_t)wave * 64 + lane) * (EPT * R);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if constexpr (scalar_traits<T>::is_complex) {
        mu[2 * e] = du[e].re;
        mu[2 * e + 1] = du[e].im;
        mw[2 * e] = dw[e].re;
        mw[2 * e + 1] = dw[e].im;
      } else {
        mu[e] = du[e];
        mw[e] = dw[e];
      }
    }
    __syncthreads();
    if (wave == 0) {
      T uc[EPT], wp[EPT];
      acc_t<T> last = zero<acc_t<T>>();
      double nn = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        acc_t<T> su, sw;
        auto at = [&](const double* base, int wv, int idx) { return base[((size_t)wv * 64 + lane) * (EPT * R) + idx]; };
        if constexpr (scalar_traits<T>::is_complex) {
          su = zc{(at(share_u, 0, 2 * e) + at(share_u, 1, 2 * e)) + (at(share_u, 2, 2 * e) + at(share_u, 3, 2 * e)),
                  (at(share_u, 0, 2 * e + 1) + at(share_u, 1, 2 * e + 1)) + (at(share_u, 2, 2 * e + 1) + at(share_u, 3, 2 * e + 1))};
          sw = zc{(at(share_w, 0, 2 * e) + at(share_w, 1, 2 * e)) + (at(share_w, 2, 2 * e) + at(share_w, 3, 2 * e)),
                  (at(share_w, 0, 2 * e + 1) + at(share_w, 1, 2 * e + 1)) + (at(share_w, 2, 2 * e + 1) + at(share_w, 3, 2 * e + 1))};
        } else {
          su = (at(share_u, 0, e) + at(share_u, 1, e)) + (at(share_u, 2, e) + at(share_u, 3, e));
          sw = (at(share_w, 0, e) + at(share_w, 1, e)) + (at(share_w, 2, e) + at(share_w, 3, e));
        }
        uc[e] = rmul(s, narrow<T>(sub(to_acc(rr[e]), su)));
        wp[e] = narrow<T>(sub(to_acc(wr[e]), sw));
        fnma_acc(wp[e], dlast, uc[e]);
        cfma_acc(last, uc[e], wp[e]);
        nn += abs2(wp[e]);
      }
      store_small<T>(lg.u_out, i0, n, uc);
      store_small<T>(w, i0, n, wp);
      if constexpr (scalar_traits<T>::is_complex) {
        const double lr = wave_sum(last.re), li = wave_sum(last.im);
        if (lane == 0) {
          cols[R * nb] += lr;
          cols[R * nb + 1] += li;
        }
      } else {
        const double lr = wave_sum(last);
        if (lane == 0) cols[R * nb] += lr;
      }
      nn = wave_sum(nn);
      if (lane == 0) cols[ncols - 1] += nn;
    }
    __syncthreads();  // the shares are rewritten by the next strip
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock) out[i] = cols[i];
}

// The pair sweep (pair_sweep_kernel's algebra, see there) in the SMALL-VECTOR geometry — vectors of 320 KiB .. 1 MiB, where the
// reference's users live (n = 4e4 .. 1.3e5 doubles): four waves share a strip of 64 lanes x 16 B and split the stored vectors
// between them (trips of kSmallJB vectors dealt round-robin).  Every wave takes the measured coefficients <u_j, r3>, <u_j, r4 raw>
// of its vectors (LDS-transposed column sums, as in mdot_small_kernel) and accumulates its shares of the three updates
// sum g1_j u_j, sum g2_j u_j (late updates of u_P, u_{P+1}) and sum p4_j u_j (compensation of the next operator input); wave 0
// adds the four shares in a fixed order, finishes the three strips and takes the in-strip dots.  One launch (no split: the
// launcher refuses more columns than the LDS holds and the loop keeps the one-sweep form there).  Partial columns in the layout
// of pair_sweep_kernel: [m3: R P][m4: R P][<u_P,r3>][<u_{P+1},r3>][<u_P,r4>][<u_{P+1},r4>][<r3,r4>] (R each) [|r4|^2].
int small_pair_lds_doubles(int ncols, int ept_times_reals) {
  return ((ncols + 15) & ~15) + 4 * 16 * kSmallTileRow + 3 * kBlock * ept_times_reals;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void pair_small_kernel(int64_t n, BasisSegs<T> segs, int P, const T* r1, const T* __restrict__ r2,
                                                            const T* __restrict__ r3, T* __restrict__ r4, T* uP_out,
                                                            T* __restrict__ uQ_out, const double* __restrict__ g1,
                                                            const double* __restrict__ g2, const double* __restrict__ gam,
                                                            const double* __restrict__ p4, const double* __restrict__ rho1sq,
                                                            const double* __restrict__ rho2sq, const double* __restrict__ e2,
                                                            const double* __restrict__ n3sq, double* __restrict__ partials) {
  // (r1 may alias uP_out: entering the pair form, u_{k-2} is already complete and is rewritten with zero coefficients)
  constexpr int EPT = small_geom<T>::EPT;
  constexpr int ELEMS = small_geom<T>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = 2 * R * P + 5 * R + 1;
  extern __shared__ double lds[];  // [ncols] column sums, one [16][65] tile per wave, the waves' shares of the three updates
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cols = lds;
  double* tile = lds + ((ncols + 15) & ~15) + wave * (16 * kSmallTileRow);
  double* share1 = lds + ((ncols + 15) & ~15) + 4 * (16 * kSmallTileRow);
  double* share2 = share1 + (size_t)kBlock * EPT * R;
  double* share4 = share2 + (size_t)kBlock * EPT * R;
  for (int i = tid; i < ncols; i += kBlock) cols[i] = 0.0;
  const double s1 = 1.0 / sqrt(*rho1sq), s2 = 1.0 / sqrt(*rho2sq);
  const double n3 = sqrt(*n3sq);
  const double ca = *e2 / n3, cb = n3 * s2;
  acc_t<T> gm;
  if constexpr (scalar_traits<T>::is_complex) gm = zc{gam[0], gam[1]};
  else gm = gam[0];
  double* tail = cols + 2 * R * P;
  __syncthreads();

  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {  // same trip count for every wave of the workgroup
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    T a1[EPT], a2[EPT], b3[EPT], b4r[EPT];
    load_small<T>(r1, i0, n, a1);
    load_small<T>(r2, i0, n, a2);
    load_small<T>(r3, i0, n, b3);
    load_small<T>(r4, i0, n, b4r);
#pragma unroll
    for (int e = 0; e < EPT; ++e) b4r[e] = sub(sub(b4r[e], rmul(ca, b3[e])), rmul(cb, a2[e]));
    acc_t<T> d1[EPT], d2[EPT], d4[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) d1[e] = d2[e] = d4[e] = zero<acc_t<T>>();
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_small<T>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
        acc_t<T> s3[kSmallJB], s4[kSmallJB];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b) {
          s3[b] = zero<acc_t<T>>();
          s4[b] = zero<acc_t<T>>();
          if (b < nv) {
            const int c = col0 + R * (j + b);
            acc_t<T> c1, c2, c4;
            if constexpr (scalar_traits<T>::is_complex) {
              c1 = zc{g1[c], g1[c + 1]};
              c2 = zc{g2[c], g2[c + 1]};
              c4 = zc{p4[c], p4[c + 1]};
            } else {
              c1 = g1[c];
              c2 = g2[c];
              c4 = p4[c];
            }
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
              cfma_acc(s3[b], ur[b][e], b3[e]);
              cfma_acc(s4[b], ur[b][e], b4r[e]);
              fma_acc(d1[e], c1, to_acc(ur[b][e]));
              fma_acc(d2[e], c2, to_acc(ur[b][e]));
              fma_acc(d4[e], c4, to_acc(ur[b][e]));
            }
          }
        }
        // the trip's column sums through the wave's transpose tile (16 rows): <u_j, r3> first, then <u_j, r4 raw>
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
          for (int b = 0; b < kSmallJB; ++b) {
            const acc_t<T> v = which == 0 ? s3[b] : s4[b];
            if constexpr (scalar_traits<T>::is_complex) {
              tile[(2 * b) * kSmallTileRow + lane] = v.re;
              tile[(2 * b + 1) * kSmallTileRow + lane] = v.im;
            } else {
              tile[b * kSmallTileRow + lane] = v;
            }
          }
          wave_lds_handover();
          const int i = lane >> 2, q = lane & 3;
          double sum = 0.0;
          if (i < nv * R) {
            const double* row = tile + i * kSmallTileRow + q * 16;
#pragma unroll
            for (int t2 = 0; t2 < 16; ++t2) sum += row[t2];
          }
          sum += __shfl_xor(sum, 1, 64);
          sum += __shfl_xor(sum, 2, 64);
          if (q == 0 && i < nv * R) cols[which * R * P + col0 + R * j + i] += sum;  // this column belongs to this wave alone
          wave_lds_handover();
        }
      }
      col0 += R * cnt;
    }
    double* m1 = share1 + ((size_t)wave * 64 + lane) * (EPT * R);
    double* m2 = share2 + ((size_t)wave * 64 + lane) * (EPT * R);
    double* m4 = share4 + ((size_t)wave * 64 + lane) * (EPT * R);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if constexpr (scalar_traits<T>::is_complex) {
        m1[2 * e] = d1[e].re;
        m1[2 * e + 1] = d1[e].im;
        m2[2 * e] = d2[e].re;
        m2[2 * e + 1] = d2[e].im;
        m4[2 * e] = d4[e].re;
        m4[2 * e + 1] = d4[e].im;
      } else {
        m1[e] = d1[e];
        m2[e] = d2[e];
        m4[e] = d4[e];
      }
    }
    __syncthreads();
    if (wave == 0) {
      T u1[EPT], u2[EPT], b4[EPT];
      acc_t<T> t3p = zero<acc_t<T>>(), t3q = zero<acc_t<T>>(), t4p = zero<acc_t<T>>(), t4q = zero<acc_t<T>>(),
               d34 = zero<acc_t<T>>();
      double nn = 0.0;
      auto total = [&](const double* base, int idx) {
        auto at = [&](int wv) { return base[((size_t)wv * 64 + lane) * (EPT * R) + idx]; };
        return (at(0) + at(1)) + (at(2) + at(3));
      };
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        acc_t<T> t1, t2, t4;
        if constexpr (scalar_traits<T>::is_complex) {
          t1 = zc{total(share1, 2 * e), total(share1, 2 * e + 1)};
          t2 = zc{total(share2, 2 * e), total(share2, 2 * e + 1)};
          t4 = zc{total(share4, 2 * e), total(share4, 2 * e + 1)};
        } else {
          t1 = total(share1, e);
          t2 = total(share2, e);
          t4 = total(share4, e);
        }
        u1[e] = rmul(s1, narrow<T>(sub(to_acc(a1[e]), t1)));
        T h2 = narrow<T>(sub(to_acc(a2[e]), t2));
        fnma_acc(h2, gm, u1[e]);
        u2[e] = rmul(s2, h2);
        b4[e] = narrow<T>(sub(to_acc(b4r[e]), t4));
        cfma_acc(t3p, u1[e], b3[e]);
        cfma_acc(t3q, u2[e], b3[e]);
        cfma_acc(t4p, u1[e], b4[e]);
        cfma_acc(t4q, u2[e], b4[e]);
        cfma_acc(d34, b3[e], b4[e]);
        nn += abs2(b4[e]);
      }
      store_small<T>(uP_out, i0, n, u1);
      store_small<T>(uQ_out, i0, n, u2);
      store_small<T>(r4, i0, n, b4);
      const acc_t<T> sums[5] = {wave_sum(t3p), wave_sum(t3q), wave_sum(t4p), wave_sum(t4q), wave_sum(d34)};
      nn = wave_sum(nn);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 5; ++c) {
          if constexpr (scalar_traits<T>::is_complex) {
            tail[2 * c] += sums[c].re;
            tail[2 * c + 1] += sums[c].im;
          } else {
            tail[c] += sums[c];
          }
        }
        tail[5 * R] += nn;
      }
    }
    __syncthreads();  // the shares are rewritten by the next strip
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock) out[i] = cols[i];
}
template <typename T> bool pair_small_fits(int P) {
  constexpr int R = scalar_traits<T>::reals;
  return (size_t)small_pair_lds_doubles(2 * R * P + 5 * R + 1, (int)(16 / sizeof(T)) * R) * sizeof(double) <= (size_t)64 * 1024;
}
template bool pair_small_fits<double>(int);
template bool pair_small_fits<zc>(int);
template bool pair_small_fits<float>(int);
template bool pair_small_fits<cf>(int);
// false: more columns than one workgroup's LDS holds in this geometry (nothing was launched)
template <typename T>
bool launch_pair_sweep_small(int64_t n, const BasisSegs<T>& segs, int P, const T* r1, const T* r2, const T* r3, T* r4, T* uP_out,
                             T* uQ_out, const double* g1, const double* g2, const double* gam, const double* p4, const double* rho1sq,
                             const double* rho2sq, const double* e2, const double* n3sq, double* partials, int* grid_out,
                             hipStream_t s) {
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = 2 * R * P + 5 * R + 1;
  const size_t lds_bytes = (size_t)small_pair_lds_doubles(ncols, (int)(16 / sizeof(T)) * R) * sizeof(double);
  if (!pair_small_fits<T>(P)) return false;  // (64 KiB, the default limit: no opt-in needed; P <= ~1240 real columns)
  const int grid = strip_grid(n, (int)(64 * (16 / sizeof(T))));
  hipLaunchKernelGGL((pair_small_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, segs, P, r1, r2, r3, r4, uP_out, uQ_out, g1, g2,
                     gam, p4, rho1sq, rho2sq, e2, n3sq, partials);
  LL_HIP(hipGetLastError());
  *grid_out = grid;
  return true;
}
#define LL_INST_PAIR_SMALL(T)                                                                                                    \
  template bool launch_pair_sweep_small<T>(int64_t, const BasisSegs<T>&, int, const T*, const T*, const T*, T*, T*, T*,         \
                                           const double*, const double*, const double*, const double*, const double*,          \
                                           const double*, const double*, const double*, double*, int*, hipStream_t);
LL_INST_PAIR_SMALL(double) LL_INST_PAIR_SMALL(zc) LL_INST_PAIR_SMALL(float) LL_INST_PAIR_SMALL(cf)

template <typename T>
int launch_mdot(int64_t n, T* w, const BasisSegs<T>& segs, const ThreeTerm<T>& tt, const NormRefs* pred,
                double* partials, int64_t small_bytes, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  const int ncols = scalar_traits<T>::reals * nb + 1;
  const NormRefs pr = pred ? *pred : NormRefs{nullptr, nullptr, nullptr, 1};
  if (blas_small(n, sizeof(T), small_bytes)) {
    const int grid = strip_grid(n, small_geom<T>::ELEMS);
    const size_t lds_bytes = ((size_t)((ncols + 15) & ~15) + 4 * 16 * kSmallTileRow) * sizeof(double);
    hipLaunchKernelGGL((mdot_small_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, tt, pr, pred ? 1 : 0,
                       partials, ncols);
    LL_HIP(hipGetLastError());
    return grid;
  }
  const int grid = strip_grid(n, strip<T>::ELEMS);
  const size_t lds_bytes = (size_t)4 * ncols * sizeof(double);
  // wave sums of the streaming geometry: the 4 (8) sums of a trip are formed with the transposing reduction (+0.5-1.3 %
  // at n >= 1e6 against one full wave sum per vector, measured in round 2)
  hipLaunchKernelGGL((mdot_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, tt, pr, pred ? 1 : 0, partials,
                     ncols);
  LL_HIP(hipGetLastError());
  return grid;
}
template int launch_mdot<double>(int64_t, double*, const BasisSegs<double>&, const ThreeTerm<double>&, const NormRefs*, double*, int64_t, hipStream_t);
template int launch_mdot<zc>(int64_t, zc*, const BasisSegs<zc>&, const ThreeTerm<zc>&, const NormRefs*, double*, int64_t, hipStream_t);
template int launch_mdot<float>(int64_t, float*, const BasisSegs<float>&, const ThreeTerm<float>&, const NormRefs*, double*, int64_t, hipStream_t);
template int launch_mdot<cf>(int64_t, cf*, const BasisSegs<cf>&, const ThreeTerm<cf>&, const NormRefs*, double*, int64_t, hipStream_t);

// ================================================================= a5/a6 (update half) + a7: multi-axpy
// w -= sum_j h_j u_j in one pass (w strip in registers, coefficients broadcast from LDS), then ||w||^2 of the
// result is accumulated while the strip is still in registers (fuses LA:56-60 at LL:262 into the same sweep).
template <typename T>
__global__ __launch_bounds__(kBlock) void maxpy_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs,
                                                       const double* __restrict__ h, int nb, NormRefs pred,
                                                       int predicated, double* __restrict__ partials) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  constexpr int JB = kJB;
  constexpr int R = scalar_traits<T>::reals;
  extern __shared__ double lds[];  // [R*nb] coefficients, then 4 doubles of reduction scratch
  if (predicated && !second_pass_due(pred)) return;
  const int tid = threadIdx.x;
  for (int i = tid; i < R * nb; i += kBlock) lds[i] = h[i];
  __syncthreads();
  double* red = lds + R * nb;
  double nn = 0.0;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  // Strips are walked in DESCENDING order: the multi-dot that ran just before walked them ascending, so the basis
  // strips it touched last are the ones most likely still in the Infinity Cache.
  for (int64_t sidx0 = blockIdx.x; sidx0 < nstrips; sidx0 += gridDim.x) {
    const int64_t sidx = nstrips - 1 - sidx0;
    const int64_t base = sidx * ELEMS;
    T wr[EPT];
    load_strip<T>(w, base, n, wr);
    int col = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      int j = 0;
      for (; j + JB <= cnt; j += JB, col += R * JB) maxpy_trip<T, JB>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, lds + col);
      if (j + 2 <= cnt) { maxpy_trip<T, 2>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, lds + col); j += 2; col += R * 2; }
      if (j < cnt) { maxpy_trip<T, 1>(ub + (int64_t)j * segs.ld, segs.ld, base, n, wr, lds + col); j += 1; col += R; }
    }
    store_strip<T>(w, base, n, wr);
#pragma unroll
    for (int e = 0; e < EPT; ++e) nn += abs2(wr[e]);
  }
  double tot = block_sum(nn, red);
  if (tid == 0) partials[blockIdx.x] = tot;
}

template <typename T>
int launch_maxpy(int64_t n, T* w, const BasisSegs<T>& segs, const double* h, const NormRefs* pred, double* partials,
                 int64_t small_bytes, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  const NormRefs pr = pred ? *pred : NormRefs{nullptr, nullptr, nullptr, 1};
  if (blas_small(n, sizeof(T), small_bytes)) {
    constexpr int R = scalar_traits<T>::reals;
    const int grid = strip_grid(n, small_geom<T>::ELEMS);
    const size_t lds_bytes = ((size_t)((R * nb + 1 + 15) & ~15) + (size_t)kBlock * small_geom<T>::EPT * R) * sizeof(double);
    hipLaunchKernelGGL((maxpy_small_kernel<T, false>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, h, nb, pr,
                       pred ? 1 : 0, partials, nullptr, 0, nullptr, nullptr);
    LL_HIP(hipGetLastError());
    return grid;
  }
  const int grid = strip_grid(n, strip<T>::ELEMS);
  const size_t lds_bytes = ((size_t)scalar_traits<T>::reals * nb + 4) * sizeof(double);
  hipLaunchKernelGGL((maxpy_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, h, nb, pr, pred ? 1 : 0,
                     partials);
  LL_HIP(hipGetLastError());
  return grid;
}
// The multi-axpy that folds the multi-dot's partials itself (small-vector geometry only): true when the fused kernel was
// launched — the caller then skips launch_reduce_cols.  Worth it while every workgroup's redundant fold (mparts * ncols
// loads) stays well below the ~10 us a separate fold launch costs in a launch-bound loop.
template <typename T>
bool launch_maxpy_folding(int64_t n, T* w, const BasisSegs<T>& segs, const double* mdot_partials, int mparts, double* h_out,
                          double* c0_out, double* partials, int64_t small_bytes, int* grid_out, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  constexpr int R = scalar_traits<T>::reals;
  if (!blas_small(n, sizeof(T), small_bytes) || (long long)mparts * (R * nb + 1) > 32768) return false;
  const int grid = strip_grid(n, small_geom<T>::ELEMS);
  const size_t lds_bytes = ((size_t)((R * nb + 1 + 15) & ~15) + (size_t)kBlock * small_geom<T>::EPT * R) * sizeof(double);
  hipLaunchKernelGGL((maxpy_small_kernel<T, true>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, nullptr, nb,
                     NormRefs{nullptr, nullptr, nullptr, 1}, 0, partials, mdot_partials, mparts, h_out, c0_out);
  LL_HIP(hipGetLastError());
  *grid_out = grid;
  return true;
}
#define LL_INST_MAXPY_FOLD(T)                                                                                          \
  template bool launch_maxpy_folding<T>(int64_t, T*, const BasisSegs<T>&, const double*, int, double*, double*, double*, \
                                        int64_t, int*, hipStream_t);
LL_INST_MAXPY_FOLD(double) LL_INST_MAXPY_FOLD(zc) LL_INST_MAXPY_FOLD(float) LL_INST_MAXPY_FOLD(cf)

template int launch_maxpy<double>(int64_t, double*, const BasisSegs<double>&, const double*, const NormRefs*, double*, int64_t, hipStream_t);
template int launch_maxpy<zc>(int64_t, zc*, const BasisSegs<zc>&, const double*, const NormRefs*, double*, int64_t, hipStream_t);
template int launch_maxpy<float>(int64_t, float*, const BasisSegs<float>&, const double*, const NormRefs*, double*, int64_t, hipStream_t);
template int launch_maxpy<cf>(int64_t, cf*, const BasisSegs<cf>&, const double*, const NormRefs*, double*, int64_t, hipStream_t);

// ================================================================= deterministic fold of workgroup partials
// out[j] = sum_b partials[b*ncols + j].  32 columns x 8 row-groups per workgroup; every column is folded in a
// fixed order, so results are bit-reproducible run to run (no float atomics anywhere in the library).
__global__ __launch_bounds__(256) void reduce_cols_kernel(const double* __restrict__ partials, int nparts, int ncols,
                                                          double* __restrict__ out, double* __restrict__ last_out) {
  __shared__ double sm[16][17];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;  // 16 columns (128 B per partial row) x 16 row lanes
  const int j = blockIdx.x * 16 + cx;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (j < ncols) {
    int b = ry;
    for (; b + 48 < nparts; b += 64) {  // four independent chains per lane
      a0 += partials[(size_t)b * ncols + j];
      a1 += partials[(size_t)(b + 16) * ncols + j];
      a2 += partials[(size_t)(b + 32) * ncols + j];
      a3 += partials[(size_t)(b + 48) * ncols + j];
    }
    for (; b < nparts; b += 16) a0 += partials[(size_t)b * ncols + j];
  }
  sm[ry][cx] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (ry == 0 && j < ncols) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += sm[r][cx];
    if (j == ncols - 1 && last_out) *last_out = t;
    else out[j] = t;
  }
}
// single column: one workgroup, 256 lanes
__global__ __launch_bounds__(256) void reduce_one_kernel(const double* __restrict__ partials, int nparts,
                                                         double* __restrict__ out) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nparts; b += 256) acc += partials[b];
  double tot = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = tot;
}
// The fold of the post-update norm and the publish step in one launch (single-GPU whole-loop drivers): out[0] = sum of
// the partials = ||w||^2 after the Gram-Schmidt pass, and the four per-iteration scalars (alpha, that norm, ||w||^2
// before the pass, the norm again) go straight to the pinned host slot.
__global__ __launch_bounds__(256) void reduce_publish_kernel(const double* __restrict__ partials, int nparts,
                                                             double* __restrict__ out, const double* __restrict__ alpha,
                                                             const double* __restrict__ c0, double* __restrict__ host) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nparts; b += 256) acc += partials[b];
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    out[0] = tot;
    host[0] = alpha ? *alpha : 0.0;
    host[1] = tot;
    host[2] = c0 ? *c0 : 0.0;
    host[3] = tot;
  }
}
void launch_reduce_publish(const double* partials, int nparts, double* out, const double* alpha, const double* c0,
                           double* host_mapped, hipStream_t s) {
  hipLaunchKernelGGL(reduce_publish_kernel, dim3(1), dim3(256), 0, s, partials, nparts, out, alpha, c0, host_mapped);
  LL_HIP(hipGetLastError());
}
// last_out (nullable): destination of the LAST column (the ||w||^2 column of mdot) instead of out[ncols-1].
void launch_reduce_cols(const double* partials, int nparts, int ncols, double* out, double* last_out, hipStream_t s) {
  if (ncols == 1) {
    hipLaunchKernelGGL(reduce_one_kernel, dim3(1), dim3(256), 0, s, partials, nparts, last_out ? last_out : out);
  } else {
    hipLaunchKernelGGL(reduce_cols_kernel, dim3((ncols + 15) / 16), dim3(256), 0, s, partials, nparts, ncols, out,
                       last_out);
  }
  LL_HIP(hipGetLastError());
}
// Sharded contexts: ||w - U h||^2 = ||w||^2 - sum |h_j|^2 for an orthonormal U (Pythagoras), from values every rank
// already holds after the one all-reduce of (h, ||w||^2) — no second all-reduce for the norm.  Fixed summation order,
// identical inputs on all ranks => identical bits on all ranks.
__global__ __launch_bounds__(256) void derive_norm_kernel(const double* __restrict__ c0_src, const double* __restrict__ h,
                                                          int count, double* __restrict__ c0, double* __restrict__ c1,
                                                          const double* __restrict__ alpha, double* __restrict__ host) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) acc = fma(h[i], h[i], acc);
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const double before = *c0_src;
    double v = before - tot;
    v = v > 0.0 ? v : 0.0;
    *c0 = before;  // the copy of ||w||^2 out of the all-reduced buffer and ...
    *c1 = v;
    if (host) {    // ... the publish step ride along (two launches per iteration less on sharded contexts)
      host[0] = alpha ? *alpha : 0.0;
      host[1] = v;
      host[2] = before;
      host[3] = v;
    }
  }
}
void launch_derive_norm(const double* c0_src, const double* h, int count, double* c0, double* c1, const double* alpha,
                        double* host_mapped, hipStream_t s) {
  hipLaunchKernelGGL(derive_norm_kernel, dim3(1), dim3(256), 0, s, c0_src, h, count, c0, c1, alpha, host_mapped);
  LL_HIP(hipGetLastError());
}
__global__ void set_scalar_kernel(double* dst, double v) { *dst = v; }
void launch_set_scalar(double* dst, double v, hipStream_t s) {
  hipLaunchKernelGGL(set_scalar_kernel, dim3(1), dim3(1), 0, s, dst, v);
  LL_HIP(hipGetLastError());
}
__global__ void copy_scalar_kernel(double* dst, const double* src) { *dst = *src; }
void launch_copy_scalar(double* dst, const double* src, hipStream_t s) {
  hipLaunchKernelGGL(copy_scalar_kernel, dim3(1), dim3(1), 0, s, dst, src);
  LL_HIP(hipGetLastError());
}

// ================================================================= a8: scale, plain three-term, dot, offset+dot
template <typename T>
__global__ __launch_bounds__(kBlock) void scale_kernel(int64_t n, T* __restrict__ v, double a, NormRefs norms,
                                                       int use_norms) {
  constexpr int EPT = strip<T>::EPT;
  const double f = use_norms ? 1.0 / sqrt(final_norm2(norms)) : a;  // T(1)/norm, LA:77-80
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    T r[EPT];
    load_strip<T>(v, base, n, r);
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = rmul(f, r[e]);
    store_strip<T>(v, base, n, r);
  }
}
template <typename T> void launch_scale(int64_t n, T* v, double a, const NormRefs* norms, hipStream_t s) {
  const NormRefs nr = norms ? *norms : NormRefs{nullptr, nullptr, nullptr, 0};
  hipLaunchKernelGGL((scale_kernel<T>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, v, a, nr,
                     norms ? 1 : 0);
  LL_HIP(hipGetLastError());
}
template void launch_scale<double>(int64_t, double*, double, const NormRefs*, hipStream_t);
template void launch_scale<zc>(int64_t, zc*, double, const NormRefs*, hipStream_t);
template void launch_scale<float>(int64_t, float*, double, const NormRefs*, hipStream_t);
template void launch_scale<cf>(int64_t, cf*, double, const NormRefs*, hipStream_t);

// a8 fused with the fold of the post-pass norm and the publish step (see launch_scale_publish in ll_internal.hpp)
template <typename T>
__global__ __launch_bounds__(kBlock) void scale_publish_kernel(int64_t n, T* __restrict__ v,
                                                               const double* __restrict__ partials, int nparts,
                                                               double* __restrict__ out, const double* __restrict__ alpha,
                                                               const double* __restrict__ c0, double* __restrict__ host,
                                                               const T* __restrict__ src) {
  constexpr int EPT = strip<T>::EPT;
  __shared__ double fold_scratch[5];
  const double tot = fold_partials_all(partials, nparts, fold_scratch);  // the order of reduce_publish_kernel
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = tot;
    host[0] = alpha ? *alpha : 0.0;
    host[1] = tot;
    host[2] = c0 ? *c0 : 0.0;
    host[3] = tot;
  }
  const double f = 1.0 / sqrt(tot);  // T(1)/norm, LA:77-80
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    T r[EPT];
    load_strip<T>(src ? src : v, base, n, r);
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = rmul(f, r[e]);
    store_strip<T>(v, base, n, r);
  }
}
// Sharded contexts: a8 fused with derive_norm_kernel — every workgroup forms ||w'||^2 = ||w||^2 - sum |h_j|^2 from the
// all-reduced coefficients (same fixed order as derive_norm_kernel, identical bits on all workgroups and ranks), scales by
// 1/||w'||; workgroup 0 stores c0 / c1 and the iteration's four scalars to the pinned host slot.
template <typename T>
__global__ __launch_bounds__(kBlock) void scale_derive_kernel(int64_t n, T* __restrict__ v, const double* __restrict__ c0_src,
                                                              const double* __restrict__ h, int count, double* __restrict__ c0,
                                                              double* __restrict__ c1, const double* __restrict__ alpha,
                                                              double* __restrict__ host) {
  constexpr int EPT = strip<T>::EPT;
  __shared__ double red[5];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += kBlock) acc = fma(h[i], h[i], acc);
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const double before = *c0_src;
    double val = before - tot;
    val = val > 0.0 ? val : 0.0;
    red[4] = val;
    if (blockIdx.x == 0) {
      *c0 = before;
      *c1 = val;
      if (host) {
        host[0] = alpha ? *alpha : 0.0;
        host[1] = val;
        host[2] = before;
        host[3] = val;
      }
    }
  }
  __syncthreads();
  const double f = 1.0 / sqrt(red[4]);
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    T r[EPT];
    load_strip<T>(v, base, n, r);
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = rmul(f, r[e]);
    store_strip<T>(v, base, n, r);
  }
}
template <typename T>
void launch_scale_derive(int64_t n, T* v, const double* c0_src, const double* h, int count, double* c0, double* c1,
                         const double* alpha, double* host_mapped, hipStream_t s) {
  hipLaunchKernelGGL((scale_derive_kernel<T>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, v, c0_src, h, count,
                     c0, c1, alpha, host_mapped);
  LL_HIP(hipGetLastError());
}
#define LL_INST_SCALE_DERIVE(T) \
  template void launch_scale_derive<T>(int64_t, T*, const double*, const double*, int, double*, double*, const double*, double*, hipStream_t);
LL_INST_SCALE_DERIVE(double) LL_INST_SCALE_DERIVE(zc) LL_INST_SCALE_DERIVE(float) LL_INST_SCALE_DERIVE(cf)

template <typename T>
int launch_scale_publish(int64_t n, T* v, const double* partials, int nparts, double* out, const double* alpha,
                         const double* c0, double* host_mapped, hipStream_t s, const T* src) {
  const int grid = strip_grid(n, strip<T>::ELEMS);
  hipLaunchKernelGGL((scale_publish_kernel<T>), dim3(grid), dim3(kBlock), 0, s, n, v, partials, nparts, out, alpha, c0,
                     host_mapped, src);
  LL_HIP(hipGetLastError());
  return grid;
}
template int launch_scale_publish<double>(int64_t, double*, const double*, int, double*, const double*, const double*, double*, hipStream_t, const double*);
template int launch_scale_publish<zc>(int64_t, zc*, const double*, int, double*, const double*, const double*, double*, hipStream_t, const zc*);
template int launch_scale_publish<float>(int64_t, float*, const double*, int, double*, const double*, const double*, double*, hipStream_t, const float*);
template int launch_scale_publish<cf>(int64_t, cf*, const double*, int, double*, const double*, const double*, double*, hipStream_t, const cf*);

template <typename T>
__global__ __launch_bounds__(kBlock) void three_term_kernel(int64_t n, T* __restrict__ w, const T* __restrict__ up,
                                                            const T* __restrict__ uc, double beta, double alpha) {
  constexpr int EPT = strip<T>::EPT;
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    T wr[EPT], c[EPT];
    load_strip<T>(w, base, n, wr);
    load_strip<T>(uc, base, n, c);
    if (up) {
      T p[EPT];
      load_strip<T>(up, base, n, p);
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, p[e])), rmul(alpha, c[e]));
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, c[e]));
    }
    store_strip<T>(w, base, n, wr);
  }
}
template <typename T>
void launch_three_term(int64_t n, T* w, const T* u_prev, const T* u_cur, double beta, double alpha, hipStream_t s) {
  hipLaunchKernelGGL((three_term_kernel<T>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, w, u_prev,
                     u_cur, beta, alpha);
  LL_HIP(hipGetLastError());
}
template void launch_three_term<double>(int64_t, double*, const double*, const double*, double, double, hipStream_t);
template void launch_three_term<zc>(int64_t, zc*, const zc*, const zc*, double, double, hipStream_t);
template void launch_three_term<float>(int64_t, float*, const float*, const float*, double, double, hipStream_t);
template void launch_three_term<cf>(int64_t, cf*, const cf*, const cf*, double, double, hipStream_t);

template <typename T>
__global__ __launch_bounds__(kBlock) void dot_kernel(int64_t n, const T* __restrict__ a, const T* __restrict__ b,
                                                     double* __restrict__ partials) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int R = scalar_traits<T>::reals;
  __shared__ double red[4];
  acc_t<T> acc = zero<acc_t<T>>();
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    T x[EPT], y[EPT];
    load_strip<T>(a, base, n, x);
    load_strip<T>(b, base, n, y);
#pragma unroll
    for (int e = 0; e < EPT; ++e) cfma_acc(acc, x[e], y[e]);
  }
  if constexpr (scalar_traits<T>::is_complex) {
    double re = block_sum(acc.re, red);
    double im = block_sum(acc.im, red);
    if (threadIdx.x == 0) {
      partials[(size_t)blockIdx.x * R] = re;
      partials[(size_t)blockIdx.x * R + 1] = im;
    }
  } else {
    double v = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = v;
  }
}
template <typename T> int launch_dot(int64_t n, const T* a, const T* b, double* partials, hipStream_t s) {
  const int grid = strip_grid(n, strip<T>::ELEMS);
  hipLaunchKernelGGL((dot_kernel<T>), dim3(grid), dim3(kBlock), 0, s, n, a, b, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template int launch_dot<double>(int64_t, const double*, const double*, double*, hipStream_t);
template int launch_dot<zc>(int64_t, const zc*, const zc*, double*, hipStream_t);
template int launch_dot<float>(int64_t, const float*, const float*, double*, hipStream_t);
template int launch_dot<cf>(int64_t, const cf*, const cf*, double*, hipStream_t);

// y += offset*x ; Re<x,y> partials — the a2/a3 post-pass for callback operators (CSR fuses it into the SpMV).
template <typename T>
__global__ __launch_bounds__(kBlock) void offset_dot_kernel(int64_t n, const T* __restrict__ x, T* __restrict__ y,
                                                            double offset, double* __restrict__ partials) {
  constexpr int EPT = strip<T>::EPT;
  __shared__ double red[4];
  double acc = 0.0;
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    T xr[EPT], yr[EPT];
    load_strip<T>(x, base, n, xr);
    load_strip<T>(y, base, n, yr);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      yr[e] = add(yr[e], rmul(offset, xr[e]));
      acc += re_cmul(xr[e], yr[e]);
    }
    store_strip<T>(y, base, n, yr);
  }
  double tot = block_sum(acc, red);
  if (threadIdx.x == 0 && partials) partials[blockIdx.x] = tot;
}
template <typename T>
int launch_offset_dot(int64_t n, const T* x, T* y, double offset, double* dot_partials, hipStream_t s) {
  const int grid = strip_grid(n, strip<T>::ELEMS);
  hipLaunchKernelGGL((offset_dot_kernel<T>), dim3(grid), dim3(kBlock), 0, s, n, x, y, offset, dot_partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template int launch_offset_dot<double>(int64_t, const double*, double*, double, double*, hipStream_t);
template int launch_offset_dot<zc>(int64_t, const zc*, zc*, double, double*, hipStream_t);
template int launch_offset_dot<float>(int64_t, const float*, float*, double, double*, hipStream_t);
template int launch_offset_dot<cf>(int64_t, const cf*, cf*, double, double*, hipStream_t);

// ================================================================= a1/a2/a3: dense row block (sample1's operator)
// One wavefront per row: the row streams in with coalesced loads, x comes from L2, the 64 partial sums fold with
// shuffles; offset, y write and the alpha partial are fused like in the CSR kernels.  Bound by the matrix stream
// (sizeof(T) * n_local * n bytes per apply).
// Column ranges [a0, a1) and [b0, b1) of every row are multiplied (the second may be empty); x element of column j is
// xf[j - xshift].  part: 0 = whole rows; 1 = the rank's own columns, y = A_own x + offset x (under the all-gather, no dot
// product yet); 2 = the other ranks' columns, y += A_rem x, then Re<x, y> (sharded contexts, Engine::apply).
template <typename T>
__global__ __launch_bounds__(kBlock) void dense_mv_kernel(long long nrows, long long ncols, const T* __restrict__ a,
                                                          const T* __restrict__ xf, const T* __restrict__ xl,
                                                          T* __restrict__ y, double offset,
                                                          double* __restrict__ dot_partials, int vec, ScaleIn<T> sc,
                                                          long long a0, long long a1, long long b0, long long b1,
                                                          long long xshift, int part) {
  __shared__ double red[5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn)
  for (long long row = (long long)blockIdx.x * 4 + wave; row < nrows; row += (long long)gridDim.x * 4) {
    const T* __restrict__ ar = a + row * ncols;
    acc_t<T> acc = zero<acc_t<T>>();
    for (int rng = 0; rng < 2; ++rng) {
      const long long j0 = rng == 0 ? a0 : b0, j1 = rng == 0 ? a1 : b1;
      if (vec) {  // 16-byte loads: V elements per lane per trip (range bounds, ncols and xshift multiples of V, bases 16-byte aligned)
        constexpr int V = (int)(16 / sizeof(T)) > 0 ? (int)(16 / sizeof(T)) : 1;
#pragma unroll 4
        for (long long j = j0 + (long long)lane * V; j < j1; j += 64 * V) {
          T av[V], xv[V];
          load_chunk<T, V>(ar + j, av);
          load_chunk<T, V>(xf + (j - xshift), xv);
#pragma unroll
          for (int e = 0; e < V; ++e) fma_acc(acc, av[e], xv[e]);
        }
      } else {
#pragma unroll 4
        for (long long j = j0 + lane; j < j1; j += 64) fma_acc(acc, ar[j], xf[j - xshift]);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      const T xi = rmul(sfac, xl[row]);
      if (sc.u_out) sc.u_out[row] = xi;
      const T yi = part == 2 ? add(y[row], narrow<T>(scale_acc(sfac, acc))) : add(narrow<T>(scale_acc(sfac, acc)), rmul(offset, xi));
      y[row] = yi;
      if (part != 1) dot_acc += re_cmul(xi, yi);
    }
  }
  if (dot_partials) {
    const double tot = block_sum(dot_acc, red);
    if (threadIdx.x == 0) dot_partials[blockIdx.x] = tot;
  }
}
template <typename T>
int launch_dense_mv(const ll_operator& op, const T* x_full, const T* x_local, T* y, double offset, double* dot_partials,
                    hipStream_t s, const ScaleIn<T>* scp, int part) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  const long long want = (op.n_local + 3) / 4;
  const int grid = (int)std::max<long long>(1, std::min<long long>(kMaxGrid, want));
  constexpr long long V = (long long)(16 / sizeof(T)) > 0 ? (long long)(16 / sizeof(T)) : 1;
  long long a0 = 0, a1 = op.n, b0 = 0, b1 = 0, xshift = 0;
  if (part == 1) {  // x_full = the local shard
    a0 = op.row_begin;
    a1 = op.row_begin + op.n_local;
    xshift = op.row_begin;
  } else if (part == 2) {  // x_full = the gathered vector (global order: equal shard strides)
    a1 = op.row_begin;
    b0 = op.row_begin + op.n_local;
    b1 = op.n;
  }
  const bool aligned = op.n % V == 0 && a0 % V == 0 && a1 % V == 0 && b0 % V == 0 && b1 % V == 0 && xshift % V == 0;
  const int vec = aligned && (reinterpret_cast<uintptr_t>(x_full) & 15) == 0 ? 1 : 0;  // rows then start 16-B aligned
  hipLaunchKernelGGL((dense_mv_kernel<T>), dim3(grid), dim3(kBlock), 0, s, (long long)op.n_local, (long long)op.n,
                     (const T*)op.dense.get(), x_full, x_local, y, offset, part == 1 ? nullptr : dot_partials, vec, sc, a0, a1, b0, b1,
                     xshift, part);
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_DENSE(T) \
  template int launch_dense_mv<T>(const ll_operator&, const T*, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*, int);
LL_INST_DENSE(double) LL_INST_DENSE(zc) LL_INST_DENSE(float) LL_INST_DENSE(cf)

// ================================================================= a1/a2/a3: matrix-free lattice operator
// (A x)(r) = (diag + onsite[r]) x(r) + sum_d ( hop[d] x(r + e_d) + conj(hop[d]) x(r - e_d) ), open or periodic per
// dimension (sample3_dynamic.cpp:17-22, T1:265-273, T2:113-121, BASELINE config 2).  Nothing but x, y (and onsite)
// moves: the neighbour reads of one site hit lines that the neighbouring lanes / the previous lattice rows already
// pulled into L1/L2, so HBM sees one read of x and one write of y.  Terms are added in ascending column order of
// the equivalent matrix row (lower neighbours slowest dimension first, the diagonal, upper neighbours fastest
// first), the order of a CSR row with sorted columns.
struct StencilGeom {
  int ndim;
  int periodic[3];
  long long dims[3];
  long long stride[3];
  double diag;
  double hop_re[3], hop_im[3];
  // Peierls phases: the bond from site r to r + e_d carries hop[d] * exp(i * sum_e grad[d][e] * c_e(r)) (c = lattice
  // coordinates of the bond's LOWER site r); the reverse direction carries the conjugate.  has_phase[d]: any grad != 0.
  double grad[3][3];
  int has_phase[3];
  long long halo;
  long long row_begin, n_local;
};
__device__ __forceinline__ double hop_value(const StencilGeom& g, int d, bool conj, double phase, double*) {
  return g.hop_re[d];
}
__device__ __forceinline__ float hop_value(const StencilGeom& g, int d, bool conj, double phase, float*) {
  return (float)g.hop_re[d];
}
__device__ __forceinline__ zc hop_value(const StencilGeom& g, int d, bool conj, double phase, zc*) {
  double re = g.hop_re[d], im = g.hop_im[d];
  if (g.has_phase[d]) {
    double sn, cs;
    sincos(phase, &sn, &cs);
    const double r2 = re * cs - im * sn, i2 = re * sn + im * cs;
    re = r2;
    im = i2;
  }
  return zc{re, conj ? -im : im};
}
__device__ __forceinline__ cf hop_value(const StencilGeom& g, int d, bool conj, double phase, cf*) {
  const zc h = hop_value(g, d, conj, phase, (zc*)nullptr);
  return cf{(float)h.re, (float)h.im};
}
// phase of the bond whose lower site has the coordinates c
__device__ __forceinline__ double bond_phase(const StencilGeom& g, int d, const long long (&c)[3]) {
  return g.grad[d][0] * (double)c[0] + g.grad[d][1] * (double)c[1] + g.grad[d][2] * (double)c[2];
}

template <typename T, typename IDX>
__global__ __launch_bounds__(kBlock) void stencil_kernel(StencilGeom g, const T* __restrict__ xl,
                                                         const T* __restrict__ lo, const T* __restrict__ hi,
                                                         const typename scalar_traits<T>::real* __restrict__ onsite,
                                                         T* __restrict__ y, double offset,
                                                         double* __restrict__ dot_partials, ScaleIn<T> sc) {
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn): the sites hold w, u = sfac * w
  const long long nl = g.n_local, H = g.halo;
  auto fetch = [&](long long j) -> T { return j < 0 ? lo[H + j] : (j >= nl ? hi[j - nl] : xl[j]); };
  for (long long li = (long long)blockIdx.x * kBlock + threadIdx.x; li < nl; li += (long long)gridDim.x * kBlock) {
    // lattice coordinates of the site (IDX = 32-bit when the whole lattice fits, else 64-bit)
    IDX rem = (IDX)(g.row_begin + li);
    long long c[3] = {0, 0, 0};
#pragma unroll
    for (int d = 2; d >= 0; --d) {
      if (d < g.ndim) {
        const IDX dim = (IDX)g.dims[d];
        const IDX q = rem / dim;
        c[d] = (long long)(rem - q * dim);
        rem = q;
      }
    }
    acc_t<T> acc = zero<acc_t<T>>();
    // lower neighbours, slowest dimension first
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < g.ndim) {
        long long off = 0;
        bool have = true;
        if (c[d] > 0) off = -g.stride[d];
        else if (g.periodic[d]) off = d == 0 ? -g.stride[0] : (g.dims[d] - 1) * g.stride[d];  // dim 0 wraps on the ring
        else have = false;
        // the bond's lower site is the neighbour: one step down in dimension d (dims[d]-1 steps up across the wrap)
        if (have) {
          const double ph = g.has_phase[d] ? bond_phase(g, d, c) - g.grad[d][d] * (c[d] > 0 ? 1.0 : -(double)(g.dims[d] - 1)) : 0.0;
          fma_acc(acc, hop_value(g, d, true, ph, (T*)nullptr), fetch(li + off));
        }
      }
    }
    const T xi = xl[li];
    fma_real(acc, g.diag + (onsite ? (double)onsite[li] : 0.0), xi);
    // upper neighbours, fastest dimension first
#pragma unroll
    for (int d = 2; d >= 0; --d) {
      if (d < g.ndim) {
        long long off = 0;
        bool have = true;
        if (c[d] + 1 < g.dims[d]) off = g.stride[d];
        else if (g.periodic[d]) off = d == 0 ? g.stride[0] : -(g.dims[d] - 1) * g.stride[d];
        else have = false;
        if (have) fma_acc(acc, hop_value(g, d, false, g.has_phase[d] ? bond_phase(g, d, c) : 0.0, (T*)nullptr), fetch(li + off));
      }
    }
    const T xs = rmul(sfac, xi);
    if (sc.u_out) sc.u_out[li] = xs;
    const T yi = add(narrow<T>(scale_acc(sfac, acc)), rmul(offset, xs));
    y[li] = yi;
    dot_acc += re_cmul(xs, yi);
  }
  if (dot_partials) {
    const double tot = block_sum(dot_acc, red);
    if (threadIdx.x == 0) dot_partials[blockIdx.x] = tot;
  }
}
// Vectorised form: every lane owns V consecutive sites of one lattice row (V * sizeof(T) = 32 bytes), so the
// coordinate arithmetic is paid once per V sites, the centre / slow-dimension neighbours / on-site terms / results
// move as 16-byte pieces and only the two fast-dimension end neighbours are scalar loads.  Needs the fastest
// dimension, the shard start and the shard length to be multiples of V (then no chunk straddles a lattice row or a
// shard / halo boundary); same accumulation order per site as stencil_kernel, so both give identical bits.
template <typename T, typename IDX, int V>
__global__ __launch_bounds__(kBlock) void stencil_vec_kernel(StencilGeom g, const T* __restrict__ xl,
                                                             const T* __restrict__ lo, const T* __restrict__ hi,
                                                             const typename scalar_traits<T>::real* __restrict__ onsite,
                                                             T* __restrict__ y, double offset,
                                                             double* __restrict__ dot_partials, ScaleIn<T> sc) {
  typedef typename scalar_traits<T>::real R;
  __shared__ double red[5];
  double dot_acc = 0.0;
  const double sfac = scale_in_factor<T>(sc, red);  // deferred normalisation (ScaleIn)
  const long long nl = g.n_local, H = g.halo;
  const int last = g.ndim - 1;
  const long long dl = g.dims[last];
  auto fetch = [&](long long j) -> T { return j < 0 ? lo[H + j] : (j >= nl ? hi[j - nl] : xl[j]); };
  auto chunk_ptr = [&](long long j) -> const T* { return j < 0 ? lo + (H + j) : (j >= nl ? hi + (j - nl) : xl + j); };
  const long long nchunks = nl / V;
  for (long long ch = (long long)blockIdx.x * kBlock + threadIdx.x; ch < nchunks; ch += (long long)gridDim.x * kBlock) {
    const long long li = ch * V;
    IDX rem = (IDX)(g.row_begin + li);
    long long c[3] = {0, 0, 0};
#pragma unroll
    for (int d = 2; d >= 0; --d) {
      if (d < g.ndim) {
        const IDX dim = (IDX)g.dims[d];
        const IDX q = rem / dim;
        c[d] = (long long)(rem - q * dim);
        rem = q;
      }
    }
    T ctr[V];
    load_chunk<T, V>(xl + li, ctr);
    // Peierls phase of site e's upward / downward bond in dimension d: the scalar kernel's expressions, site by site
    auto upper_phase = [&](int d, int e) -> double {
      if (!g.has_phase[d]) return 0.0;
      long long ce[3] = {c[0], c[1], c[2]};
      ce[last] += e;
      return bond_phase(g, d, ce);
    };
    auto lower_phase = [&](int d, int e) -> double {
      if (!g.has_phase[d]) return 0.0;
      long long ce[3] = {c[0], c[1], c[2]};
      ce[last] += e;
      return bond_phase(g, d, ce) - g.grad[d][d] * (ce[d] > 0 ? 1.0 : -(double)(g.dims[d] - 1));
    };
    acc_t<T> acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = zero<acc_t<T>>();
    // lower neighbours, slowest dimension first; the fastest dimension comes last and is a shift by one site
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < last) {
        long long off = 0;
        bool have = true;
        if (c[d] > 0) off = -g.stride[d];
        else if (g.periodic[d]) off = d == 0 ? -g.stride[0] : (g.dims[d] - 1) * g.stride[d];
        else have = false;
        if (have) {
          T nb[V];
          load_chunk<T, V>(chunk_ptr(li + off), nb);
          // the phase is evaluated per site with the scalar kernel's expression (identical bits); it is the same for
          // the whole chunk unless it depends on the fastest coordinate
          const bool varies = g.has_phase[d] && g.grad[d][last] != 0.0;
          const T hv = hop_value(g, d, true, lower_phase(d, 0), (T*)nullptr);
#pragma unroll
          for (int e = 0; e < V; ++e)
            fma_acc(acc[e], varies && e > 0 ? hop_value(g, d, true, lower_phase(d, e), (T*)nullptr) : hv, nb[e]);
        }
      } else if (d == last) {
        // fastest dimension: site e's lower neighbour is site e-1 of the chunk
        const bool varies = g.has_phase[d] && g.grad[d][d] != 0.0;
        bool have = true;
        T left = zero<T>();
        if (c[last] > 0) left = fetch(li - 1);
        else if (g.periodic[last]) left = fetch(last == 0 ? li - 1 : li + (dl - 1));  // dimension 0 wraps on the ring
        else have = false;
        if (have) fma_acc(acc[0], hop_value(g, d, true, lower_phase(d, 0), (T*)nullptr), left);
        const T hv = hop_value(g, d, true, lower_phase(d, 1), (T*)nullptr);
#pragma unroll
        for (int e = 1; e < V; ++e)
          fma_acc(acc[e], varies && e > 1 ? hop_value(g, d, true, lower_phase(d, e), (T*)nullptr) : hv, ctr[e - 1]);
      }
    }
    if (onsite) {
      R os[V];
      load_chunk<R, V>(onsite + li, os);
#pragma unroll
      for (int e = 0; e < V; ++e) fma_real(acc[e], g.diag + (double)os[e], ctr[e]);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) fma_real(acc[e], g.diag, ctr[e]);
    }
    // upper neighbours, fastest dimension first
    {
      const bool varies = g.has_phase[last] && g.grad[last][last] != 0.0;
      const T hv = hop_value(g, last, false, upper_phase(last, 0), (T*)nullptr);
#pragma unroll
      for (int e = 0; e + 1 < V; ++e)
        fma_acc(acc[e], varies && e > 0 ? hop_value(g, last, false, upper_phase(last, e), (T*)nullptr) : hv, ctr[e + 1]);
      bool have = true;
      T right = zero<T>();
      if (c[last] + V < dl) right = fetch(li + V);
      else if (g.periodic[last]) right = fetch(last == 0 ? li + V : li + V - dl);
      else have = false;
      if (have) fma_acc(acc[V - 1], varies ? hop_value(g, last, false, upper_phase(last, V - 1), (T*)nullptr) : hv, right);
    }
#pragma unroll
    for (int d = 2; d >= 0; --d) {
      if (d < last) {
        long long off = 0;
        bool have = true;
        if (c[d] + 1 < g.dims[d]) off = g.stride[d];
        else if (g.periodic[d]) off = d == 0 ? g.stride[0] : -(g.dims[d] - 1) * g.stride[d];
        else have = false;
        if (have) {
          T nb[V];
          load_chunk<T, V>(chunk_ptr(li + off), nb);
          const bool varies = g.has_phase[d] && g.grad[d][last] != 0.0;
          const T hv = hop_value(g, d, false, upper_phase(d, 0), (T*)nullptr);
#pragma unroll
          for (int e = 0; e < V; ++e)
            fma_acc(acc[e], varies && e > 0 ? hop_value(g, d, false, upper_phase(d, e), (T*)nullptr) : hv, nb[e]);
        }
      }
    }
    T out[V], us[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      us[e] = rmul(sfac, ctr[e]);
      out[e] = add(narrow<T>(scale_acc(sfac, acc[e])), rmul(offset, us[e]));
      dot_acc += re_cmul(us[e], out[e]);
    }
    if (sc.u_out) store_chunk<T, V>(sc.u_out + li, us);
    store_chunk<T, V>(y + li, out);
  }
  if (dot_partials) {
    const double tot = block_sum(dot_acc, red);
    if (threadIdx.x == 0) dot_partials[blockIdx.x] = tot;
  }
}

template <typename T>
int launch_stencil(const ll_operator& op, const T* x_local, const T* halo_lo, const T* halo_hi, T* y, double offset,
                   double* dot_partials, hipStream_t s, const ScaleIn<T>* scp) {
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  StencilGeom g;
  g.ndim = op.st.ndim;
  for (int d = 0; d < 3; ++d) {
    g.periodic[d] = d < g.ndim ? op.st.periodic[d] : 0;
    g.dims[d] = d < g.ndim ? op.st.dims[d] : 1;
    g.stride[d] = d < g.ndim ? op.st_stride[d] : 0;
    g.hop_re[d] = op.st.hop_re[d];
    g.hop_im[d] = op.st.hop_im[d];
    g.has_phase[d] = 0;
    for (int e = 0; e < 3; ++e) {
      g.grad[d][e] = (d < g.ndim && e < g.ndim) ? op.st.phase_grad[d][e] : 0.0;
      if (g.grad[d][e] != 0.0) g.has_phase[d] = 1;
    }
  }
  g.diag = op.st.diag;
  g.halo = op.st_halo;
  g.row_begin = op.row_begin;
  g.n_local = op.n_local;
  typedef typename scalar_traits<T>::real R;
  constexpr int V = (int)(32 / sizeof(T));
  const bool allow_vec = op.ctx == nullptr || op.ctx->tune.stencil_vec;
  auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool ptrs_ok = aligned16(x_local) && aligned16(y) && (g.ndim == 1 || (aligned16(halo_lo) && aligned16(halo_hi)));
  if (allow_vec && ptrs_ok && op.n_local >= V && g.dims[g.ndim - 1] % V == 0 && op.row_begin % V == 0 &&
      op.n_local % V == 0) {
    const long long chunks = op.n_local / V;
    const int vgrid = (int)std::max<long long>(1, std::min<long long>(kMaxGrid, (chunks + kBlock - 1) / kBlock));
    if (op.n < ((long long)1 << 31))
      hipLaunchKernelGGL((stencil_vec_kernel<T, unsigned, V>), dim3(vgrid), dim3(kBlock), 0, s, g, x_local, halo_lo,
                         halo_hi, (const R*)op.onsite.get(), y, offset, dot_partials, sc);
    else
      hipLaunchKernelGGL((stencil_vec_kernel<T, unsigned long long, V>), dim3(vgrid), dim3(kBlock), 0, s, g, x_local,
                         halo_lo, halo_hi, (const R*)op.onsite.get(), y, offset, dot_partials, sc);
    LL_HIP(hipGetLastError());
    return vgrid;
  }
  const long long want = (op.n_local + kBlock - 1) / kBlock;
  const int grid = (int)std::max<long long>(1, std::min<long long>(kMaxGrid, want));
  if (op.n < ((long long)1 << 31))
    hipLaunchKernelGGL((stencil_kernel<T, unsigned>), dim3(grid), dim3(kBlock), 0, s, g, x_local, halo_lo, halo_hi,
                       (const R*)op.onsite.get(), y, offset, dot_partials, sc);
  else
    hipLaunchKernelGGL((stencil_kernel<T, unsigned long long>), dim3(grid), dim3(kBlock), 0, s, g, x_local, halo_lo,
                       halo_hi, (const R*)op.onsite.get(), y, offset, dot_partials, sc);
  LL_HIP(hipGetLastError());
  return grid;
}
#define LL_INST_STENCIL(T) \
  template int launch_stencil<T>(const ll_operator&, const T*, const T*, const T*, T*, double, double*, hipStream_t, \
                                 const ScaleIn<T>*);
LL_INST_STENCIL(double) LL_INST_STENCIL(zc) LL_INST_STENCIL(float) LL_INST_STENCIL(cf)

// ================================================================= a9/a10: tall-skinny GEMV over the basis
// out_r = sum_k coeff[r*m + k] u_k for r < NOUT in one pass over the basis: every basis strip is read once and
// feeds all NOUT accumulators (the reference re-reads the basis per root, LL:51-57).  Vectors are visited in
// DESCENDING k like the reference (LL:53).  The coefficients and the accumulators are acc_t<T> (double / complex double
// for every type: the float sums are carried in double like every reduction of the library), the coefficients staged in
// LDS.  part (ld_part): the partial sums of the launches over the other basis groups — load_part: start from part;
// out == nullptr: leave the sum in part for the next launch; otherwise round it to T once into out.
template <typename T> __device__ __forceinline__ void load_acc_strip(const acc_t<T>* __restrict__ p, int64_t base, int64_t n,
                                                                     acc_t<T> (&r)[strip<T>::EPT]) {
  if constexpr (std::is_same<acc_t<T>, T>::value) {
    load_strip<T>(p, base, n, r);
  } else {
    const int64_t i0 = base + (int64_t)threadIdx.x * strip<T>::EPT;
#pragma unroll
    for (int e = 0; e < strip<T>::EPT; ++e) r[e] = (i0 + e < n) ? p[i0 + e] : zero<acc_t<T>>();
  }
}
template <typename T> __device__ __forceinline__ void store_acc_strip(acc_t<T>* __restrict__ p, int64_t base, int64_t n,
                                                                      const acc_t<T> (&r)[strip<T>::EPT]) {
  if constexpr (std::is_same<acc_t<T>, T>::value) {
    store_strip<T>(p, base, n, r);
  } else {
    const int64_t i0 = base + (int64_t)threadIdx.x * strip<T>::EPT;
#pragma unroll
    for (int e = 0; e < strip<T>::EPT; ++e)
      if (i0 + e < n) p[i0 + e] = r[e];
  }
}
template <typename T, int NOUT>
__global__ __launch_bounds__(kBlock) void gemv_basis_kernel(int64_t n, BasisSegs<T> segs, int kofs, int m_total,
                                                            const acc_t<T>* __restrict__ coeff, acc_t<T>* part, int64_t ld_part,
                                                            int load_part, T* out, int64_t ld_out) {
  typedef acc_t<T> A;
  constexpr int EPT = strip<T>::EPT;
  extern __shared__ double lds_raw[];
  A* cs = reinterpret_cast<A*>(lds_raw);  // [NOUT][nb]
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  for (int i = threadIdx.x; i < NOUT * nb; i += kBlock) {
    const int r = i / nb, k = i - r * nb;
    cs[i] = coeff[(size_t)r * m_total + kofs + k];
  }
  __syncthreads();
  const int64_t nstrips = (n + strip<T>::ELEMS - 1) / strip<T>::ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * strip<T>::ELEMS;
    A acc[NOUT][EPT];
#pragma unroll
    for (int r = 0; r < NOUT; ++r) {
      if (load_part) load_acc_strip<T>(part + (int64_t)r * ld_part, base, n, acc[r]);
      else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) acc[r][e] = zero<A>();
      }
    }
    int col = nb;
    for (int sg = segs.nseg - 1; sg >= 0; --sg) {
      const T* ub = segs.base[sg];
      for (int j = segs.count[sg] - 1; j >= 0; --j) {
        --col;
        T ur[EPT];
        load_strip<T>(ub + (int64_t)j * segs.ld, base, n, ur);
#pragma unroll
        for (int r = 0; r < NOUT; ++r) {
          const A c = cs[r * nb + col];
#pragma unroll
          for (int e = 0; e < EPT; ++e) fma_acc(acc[r][e], c, to_acc(ur[e]));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NOUT; ++r) {
      if (out == nullptr) {
        store_acc_strip<T>(part + (int64_t)r * ld_part, base, n, acc[r]);
      } else {
        T o[EPT];
#pragma unroll
        for (int e = 0; e < EPT; ++e) o[e] = narrow<T>(acc[r][e]);
        store_strip<T>(out + (int64_t)r * ld_out, base, n, o);
      }
    }
  }
}

template <typename T, int NOUT>
static void gemv_launch_n(int64_t n, const BasisSegs<T>& segs, int kofs, int m_total, const acc_t<T>* coeff, acc_t<T>* part,
                          int64_t ld_part, int load_part, T* out, int64_t ld_out, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  const size_t lds_bytes = (size_t)NOUT * nb * sizeof(acc_t<T>);
  hipLaunchKernelGGL((gemv_basis_kernel<T, NOUT>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), lds_bytes, s,
                     n, segs, kofs, m_total, coeff, part, ld_part, load_part, out, ld_out);
  LL_HIP(hipGetLastError());
}

// segs[0..nlaunch) cover vectors 0..m_total-1 in order; launches run from the last group to the first so that the
// overall accumulation order is k = m-1 .. 0.  Between launches the partial sums stay in acc_t<T>: in out itself where that is
// the same type (double, complex double), in scratch (nout x n values of acc_t<T>, needed when nlaunch > 1) for float types.
template <typename T>
void launch_gemv_basis(int64_t n, int64_t m_total, const BasisSegs<T>* segs, int nlaunch, int nout, const acc_t<T>* coeff,
                       T* out, int64_t ld_out, acc_t<T>* scratch, hipStream_t s) {
  std::vector<int> kofs(nlaunch);
  int k = 0;
  for (int i = 0; i < nlaunch; ++i) {
    kofs[i] = k;
    for (int g = 0; g < segs[i].nseg; ++g) k += segs[i].count[g];
  }
  constexpr bool same = std::is_same<acc_t<T>, T>::value;
  for (int r0 = 0; r0 < nout; r0 += 4) {  // up to 4 outputs per pass (register budget: 4*EPT accumulators)
    const int nr = nout - r0 < 4 ? nout - r0 : 4;
    for (int i = nlaunch - 1; i >= 0; --i) {
      const int load = (i != nlaunch - 1);
      const acc_t<T>* c = coeff + (size_t)r0 * m_total;
      T* o = out + (int64_t)r0 * ld_out;
      acc_t<T>* part = same ? reinterpret_cast<acc_t<T>*>(o) : (scratch ? scratch + (int64_t)r0 * n : nullptr);
      const int64_t ld_part = same ? ld_out : n;
      T* dst = (same || i == 0) ? o : nullptr;  // float types: the last launch rounds once into out
      LL_REQUIRE(part != nullptr || nlaunch == 1, "gemv_basis: scratch missing");
      switch (nr) {
        case 1: gemv_launch_n<T, 1>(n, segs[i], kofs[i], (int)m_total, c, part, ld_part, load, dst, ld_out, s); break;
        case 2: gemv_launch_n<T, 2>(n, segs[i], kofs[i], (int)m_total, c, part, ld_part, load, dst, ld_out, s); break;
        case 3: gemv_launch_n<T, 3>(n, segs[i], kofs[i], (int)m_total, c, part, ld_part, load, dst, ld_out, s); break;
        default: gemv_launch_n<T, 4>(n, segs[i], kofs[i], (int)m_total, c, part, ld_part, load, dst, ld_out, s); break;
      }
    }
  }
}
#define LL_INST_GEMV(T) \
  template void launch_gemv_basis<T>(int64_t, int64_t, const BasisSegs<T>*, int, int, const acc_t<T>*, T*, int64_t, acc_t<T>*, hipStream_t);
LL_INST_GEMV(double) LL_INST_GEMV(zc) LL_INST_GEMV(float) LL_INST_GEMV(cf)

// ================================================================= tiny scalar kernels
__global__ void accumulate_h_kernel(double* h_acc, const double* h_add, int count, NormRefs pred, int predicated) {
  if (predicated && !second_pass_due(pred)) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) h_acc[i] += h_add[i];
}
void launch_accumulate_h(double* h_acc, const double* h_add, int count, const NormRefs* pred, hipStream_t s) {
  const NormRefs pr = pred ? *pred : NormRefs{nullptr, nullptr, nullptr, 1};
  hipLaunchKernelGGL(accumulate_h_kernel, dim3((count + 255) / 256), dim3(256), 0, s, h_acc, h_add, count, pr,
                     pred ? 1 : 0);
  LL_HIP(hipGetLastError());
}
// The only per-iteration device->host traffic of the Lanczos loop: four doubles stored straight into pinned,
// device-mapped host memory (no DMA copy on the critical path).
__global__ void publish_kernel(double* out, const double* alpha, NormRefs norms) {
  out[0] = alpha ? *alpha : 0.0;
  out[1] = final_norm2(norms);
  out[2] = *norms.c0;
  out[3] = *norms.c1;
}
void launch_publish(double* out_mapped, const double* alpha, const NormRefs& norms, hipStream_t s) {
  hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(1), 0, s, out_mapped, alpha, norms);
  LL_HIP(hipGetLastError());
}

// ================================================================= streaming ceilings of the device at hand (ll_bandwidth_probe)
// SURVEY 8d "Bound": the roofline fraction is also reported against a MEASURED ceiling taken in the same process: a read-only
// stream (sum of a buffer) and a copy (read + write), 16-byte accesses per lane, U loads in flight per lane.
template <int U> __global__ __launch_bounds__(256) void bw_read_kernel(const double2* __restrict__ a, size_t n2, double* out) {
  double acc = 0.0;
  const size_t stride = (size_t)gridDim.x * 256 * U;
  for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n2; i += stride) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = i + (size_t)u * 256 < n2 ? a[i + (size_t)u * 256] : double2{0, 0};
#pragma unroll
    for (int u = 0; u < U; ++u) acc += v[u].x + v[u].y;
  }
  if (acc == 1.2345e-300) out[0] = acc;  // keeps the loads alive
}
template <int U> __global__ __launch_bounds__(256) void bw_copy_kernel(const double2* __restrict__ a, double2* __restrict__ b, size_t n2) {
  const size_t stride = (size_t)gridDim.x * 256 * U;
  for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n2; i += stride) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = i + (size_t)u * 256 < n2 ? a[i + (size_t)u * 256] : double2{0, 0};
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + (size_t)u * 256 < n2) b[i + (size_t)u * 256] = v[u];
  }
}
void launch_bw_read(const void* a, size_t bytes, double* out, int grid, hipStream_t s) {
  hipLaunchKernelGGL(bw_read_kernel<8>, dim3(grid), dim3(256), 0, s, (const double2*)a, bytes / sizeof(double2), out);
  LL_HIP(hipGetLastError());
}
void launch_bw_copy(const void* a, void* b, size_t bytes, int grid, hipStream_t s) {
  hipLaunchKernelGGL(bw_copy_kernel<4>, dim3(grid), dim3(256), 0, s, (const double2*)a, (double2*)b, bytes / sizeof(double2));
  LL_HIP(hipGetLastError());
}

}  // namespace ll
