// The operator kernels that need no image of their own: the CSR-stream SpMV with the column split of a sharded CSR image, the
// dense row block and the matrix-free lattice stencil (beside spmv_pb.hip, spmv_tiled.hip, spmv_sym.hip and pauli.hip).
//
// All are HBM-bandwidth bound (SpMV 0.15 flop/B); offset, the write of y and the alpha partial are fused into the
// one pass over the operator.  Reference rows:
//   a1/a2/a3  spmv_stream / dense_mv / stencil   mv_mul (LL:243, EX:108) + offset update (LL:244-246) + alpha dot (LL:248, EX:110)
#include <algorithm>

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
  const int grid = spmv_grid(ntiles, sizeof(T));
  const ScaleIn<T> sc = scp ? *scp : ScaleIn<T>{};
  // (the kernel that publishes an iteration's scalars may complete that iteration's event itself: ll_context::stop_next)
  hipEvent_t stop = part != 1 ? take_stop(op.ctx) : nullptr;
  for_row_ptr_type(im.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    LL_LAUNCH_STOP(stop, (spmv_stream<T, RP>), dim3(grid), dim3(kBlock), 0, s, ntiles, im.tiles.get(), (const RP*)im.row_ptr.get(),
                   im.col.get(), (const T*)im.val.get(), x_full, x_local, y, offset, part == 1 ? nullptr : dot_partials, sc, part);
  });
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
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((csr_count_own_kernel<RP>), dim3(grid), dim3(256), 0, s, (long long)op.n_local, c0, c1,
                       (const RP*)a.row_ptr.get(), a.col.get(), own_cnt);
  });
  LL_HIP(hipGetLastError());
}
template <typename T> void launch_csr_split(const ll_operator& op, const CsrImage& own, const CsrImage& rem, hipStream_t s) {
  const int grid = (int)std::max<long long>(1, std::min<long long>(kMaxGrid, (op.n_local + 255) / 256));
  const long long c0 = op.row_begin, c1 = op.row_begin + op.n_local;
  const CsrImage& a = op.csr;
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((csr_split_kernel<T, RP>), dim3(grid), dim3(256), 0, s, (long long)op.n_local, c0, c1,
                       (const RP*)a.row_ptr.get(), a.col.get(), (const T*)a.val.get(), (const RP*)own.row_ptr.get(),
                       (const RP*)rem.row_ptr.get(), own.col.get(), (T*)own.val.get(), rem.col.get(), (T*)rem.val.get());
  });
  LL_HIP(hipGetLastError());
}
#define LL_INST_SPMV(T)                                                                                                       \
  template int launch_spmv<T>(const ll_operator&, const T*, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*, int); \
  template void launch_csr_count_own<T>(const ll_operator&, int32_t*, hipStream_t);                                            \
  template void launch_csr_split<T>(const ll_operator&, const CsrImage&, const CsrImage&, hipStream_t);
LL_FOR_EACH_SCALAR(LL_INST_SPMV)

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
LL_FOR_EACH_SCALAR(LL_INST_DENSE)

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
LL_FOR_EACH_SCALAR(LL_INST_STENCIL)

}  // namespace ll
