// Device-side construction of the two SpMV images that are built from an operator's CSR arrays: the propagation-blocked image
// (kernels: spmv_pb.hip) and the 2-D tiled image (kernel: spmv_tiled.hip), and the check of the CSR arrays themselves.
// Every number of a layout comes from spmv_plan.hpp (host arithmetic, tested on the CPU); a builder here is the sequence
// plan -> count launch -> read-back -> layout -> allocate and upload -> scatter launches -> move the image into the operator.
#include <algorithm>
#include <vector>

#include "dev_helpers.hpp"
#include "ll_internal.hpp"
#include "spmv_shared.hpp"

namespace ll {

// ================================================================= build kernels
// exponent of every local row's absolute sum: sum_j |a_ij| < 2^rexp[i]  (32767: the row holds Inf / NaN)
template <typename T, typename RP>
__global__ __launch_bounds__(256) void pb_rowexp_kernel(long long n_local, const RP* __restrict__ rp,
                                                        const T* __restrict__ va, int16_t* __restrict__ rexp) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_local; i += (long long)gridDim.x * 256) {
    double s = 0.0;
    for (long long p = (long long)rp[i]; p < (long long)rp[i + 1]; ++p) s += abs1(va[p]);
    int e = -1100;
    if (s > 0.0 && isfinite(s)) (void)frexp(s, &e);
    else if (!(s == 0.0)) e = 32767;
    rexp[i] = (int16_t)e;
  }
}

// Pass 1: entries per (column block, row block).  One workgroup per row block, LDS histogram over the column blocks.
template <typename RP>
__global__ __launch_bounds__(256) void pb_count_kernel(PbColMap m, int ncb, int nrb, int rb_rows, long long n_local,
                                                       const RP* __restrict__ rp, const int32_t* __restrict__ ci,
                                                       int32_t* __restrict__ cnt /* [ncb][nrb] */,
                                                       const uint32_t* __restrict__ skip = nullptr) {
  extern __shared__ int hist[];
  const int r = blockIdx.x;
  for (int i = threadIdx.x; i < ncb; i += 256) hist[i] = 0;
  __syncthreads();
  const long long i0 = (long long)r * rb_rows, i1 = min(n_local, i0 + rb_rows);
  const long long p0 = (long long)rp[i0], p1 = (long long)rp[i1];
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    if (skip != nullptr && ((skip[p >> 5] >> (p & 31)) & 1u)) continue;  // the row's diagonal entry: kept outside the image
    int local;
    atomicAdd(&hist[pb_block_of(m, ci[p], &local)], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ncb; i += 256) cnt[(size_t)i * nrb + r] = hist[i];
}

// Pass 2: scatter.  ONE wavefront per row block walks the block's entries in CSR order, 64 at a time; entries of the
// chunk that fall into the same segment get consecutive slots in lane order (ballot ranking), so the position of
// every entry is a pure function of the matrix: the image — hence the summation order of phase 2 — is identical
// from build to build.  Inside a segment both orders agree (row-major, original order within a row).
// TILED (the 2-D tiled image, tl_build_device below): ONE order — the segments of a row block are consecutive (segq is laid out row
// block by row block, segdest is not used) — the two 16-bit local indices of an entry are packed into one 32-bit word
// (pcol is that array, prow is not used) and the value is stored PRE-SCALED by 2^-er_i (rexp: exponent of the row's
// absolute sum), an exact operation that takes the per-row exponent out of the kernel's inner loop.
template <typename T, typename RP, bool TILED = false>
__global__ __launch_bounds__(64) void pb_scatter_kernel(PbColMap m, int ncb, int nrb, int rb_rows, long long n_local,
                                                        const RP* __restrict__ rp, const int32_t* __restrict__ ci,
                                                        const T* __restrict__ va, const int64_t* __restrict__ segq,
                                                        const int64_t* __restrict__ segdest, T* __restrict__ pval,
                                                        uint16_t* __restrict__ pcol, uint16_t* __restrict__ prow,
                                                        const int16_t* __restrict__ rexp = nullptr,
                                                        const uint32_t* __restrict__ skip = nullptr) {
  extern __shared__ int fill[];  // [ncb]
  const int r = blockIdx.x, lane = threadIdx.x;
  for (int i = lane; i < ncb; i += 64) fill[i] = 0;
  __syncthreads();
  const long long i0 = (long long)r * rb_rows, i1 = min(n_local, i0 + rb_rows);
  const long long p0 = (long long)rp[i0], p1 = (long long)rp[i1];
  long long row_hint = i0;  // row of the chunk's first entry (monotone over the chunks)
  for (long long base = p0; base < p1; base += 64) {
    const long long p = base + lane;
    const bool in_range = p < p1;
    const bool valid = in_range && !(skip != nullptr && ((skip[p >> 5] >> (p & 31)) & 1u));  // (the diagonal entry stays outside)
    // row of entry p: the last row i with rp[i] <= p (binary search from the hint; rows of a chunk are few)
    long long lo = row_hint, hi = i1 - 1;
    if (in_range) {
      while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if ((long long)rp[mid] <= p) lo = mid; else hi = mid - 1;
      }
    }
    const long long rowi = lo;
    row_hint = __shfl(rowi, 0, 64);
    int local = 0;
    const int key = valid ? pb_block_of(m, ci[p], &local) : -1;
    int off = 0;
    unsigned long long todo = __ballot(valid);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int k = __shfl(key, leader, 64);
      const unsigned long long same = __ballot(valid && key == k);
      if (valid && key == k) off = fill[k] + __popcll(same & ((1ull << lane) - 1ull));
      __syncthreads();  // single wave: orders the LDS read above before the update below
      if (lane == leader) fill[k] += __popcll(same);
      __syncthreads();
      todo &= ~same;
    }
    if (valid) {
      const long long q = segq[(size_t)key * (nrb + 1) + r] + off;
      if constexpr (TILED) {
        const int er = rexp[rowi];
        pval[q] = (er == 32767 || er <= -1100) ? va[p] : scale_pow2(va[p], -er);  // (rows with Inf / NaN, empty rows: as is)
        reinterpret_cast<uint32_t*>(pcol)[q] = (uint32_t)local | ((uint32_t)(rowi - i0) << 16);
      } else {
        const long long qd = segdest[(size_t)key * nrb + r] + off;
        pval[q] = va[p];
        pcol[q] = (uint16_t)local;
        prow[qd] = (uint16_t)(rowi - i0);
      }
    }
  }
}

// The first diagonal entry of every local row leaves the image: it is the one entry whose x element the row's own epilogue
// holds anyway (offset term, alpha), so its product needs no trip through the product buffer — 28 bytes of traffic per row
// saved for 8 (the diag array), 1/15 of config 3's entries.  diag[i] = a_ii (0 when the row stores none), skip: one bit
// per CSR entry, set for the entries taken out (read by the count and scatter kernels).  Further diagonal duplicates of a
// row stay in the streams.
template <typename T, typename RP>
__global__ __launch_bounds__(256) void pb_diag_kernel(long long n_local, long long row_begin, const RP* __restrict__ rp,
                                                      const int32_t* __restrict__ ci, const T* __restrict__ va,
                                                      T* __restrict__ diag, uint32_t* __restrict__ skip) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_local; i += (long long)gridDim.x * 256) {
    T d = zero<T>();
    const long long g = row_begin + i;
    for (long long p = (long long)rp[i]; p < (long long)rp[i + 1]; ++p)
      if ((long long)ci[p] == g) {
        d = va[p];
        atomicOr(&skip[p >> 5], 1u << (p & 31));
        break;
      }
    diag[i] = d;
  }
}

// max_i sum_j |a_ij| over the local rows and the column range check, on the device (inputs may never have been on
// the host).  out[0] = max row sum, out[1] = number of out-of-range columns.
template <typename T, typename RP>
__global__ __launch_bounds__(256) void csr_check_kernel(long long n_local, long long n_cols, const RP* __restrict__ rp,
                                                        const int32_t* __restrict__ ci, const T* __restrict__ va,
                                                        double* __restrict__ part_max, unsigned long long* __restrict__ bad) {
  __shared__ double red[4];
  double mx = 0.0;
  unsigned long long nbad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_local; i += (long long)gridDim.x * 256) {
    double rs = 0.0;
    for (long long p = (long long)rp[i]; p < (long long)rp[i + 1]; ++p) {
      rs += sqrt(abs2(va[p]));
      const int c = ci[p];
      if (c < 0 || c >= n_cols) ++nbad;
    }
    mx = fmax(mx, rs);
  }
  // fold: max over the workgroup (wave shuffles + LDS), count via one atomic per lane that saw a bad column
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mx = fmax(mx, __shfl_down(mx, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) part_max[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  if (nbad) atomicAdd(bad, nbad);
}

// ================================================================= builders
namespace {
// grid of the kernels that walk the local rows with a grid stride
int row_grid(int64_t nr) { return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, (nr + 255) / 256)); }

// a host table of a plan -> a device array of the image (asynchronous: the caller synchronises before the table goes out of scope)
template <typename E> void upload_table(ll_context* ctx, DevArray<E>& dst, const std::vector<E>& v, const char* what) {
  dst = ctx->dev_alloc<E>(v.size(), what);
  LL_HIP(hipMemcpyAsync(dst.get(), v.data(), v.size() * sizeof(E), hipMemcpyHostToDevice, ctx->stream));
}

// the inputs of the planners (spmv_plan.hpp) for an operator of storage type T
template <typename T> PlanShape plan_shape(const ll_operator* op) {
  const ll_context* ctx = op->ctx;
  PlanShape sh;
  sh.elem_bytes = sizeof(T);
  sh.acc_bytes = sizeof(acc_t<T>);
  sh.n = op->n;
  sh.n_local = op->n_local;
  sh.row_begin = op->row_begin;
  sh.nranks = ctx->nranks;
  sh.shard = ctx->nranks > 1 ? op->n_shard : op->n;
  sh.rank = ctx->comm != nullptr ? ctx->rank : 0;
  // test hook: treat the rank's own columns like everybody else's (every x slice is read from the gathered buffer), so
  // that a 1-rank RCCL communicator exercises the gather -> remote-block dependency of the overlapped path
  if (ctx->comm != nullptr && ctx->tune.pb_test_all_remote) sh.rank = -1;
  return sh;
}
PlanTuning plan_tuning(const Tuning& t) {
  PlanTuning p;
  p.pb_block = t.pb_block;
  p.pb_row_block = t.pb_row_block;
  p.pb_col_block = t.pb_col_block;
  p.gather_chunks = t.gather_chunks;
  p.pb_pad = t.pb_pad;
  p.tl_walk_modulo = t.tl_walk_modulo;
  return p;
}
PlanLimits plan_limits() {
  PlanLimits lim;
  lim.cus = kCUs;
  return lim;
}

// entries per (column block, row block) of the map m, counted on the device into d_cnt [ncb][nrb] and read back
std::vector<int32_t> count_segments(const ll_operator* op, const PbColMap& m, int64_t ncb, int64_t nrb, int64_t rb_rows,
                                    const uint32_t* skip, const DevArray<int32_t>& d_cnt) {
  const CsrImage& a = op->csr;
  hipStream_t s = op->ctx->stream;
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((pb_count_kernel<RP>), dim3((int)nrb), dim3(256), (size_t)ncb * sizeof(int), s, m, (int)ncb, (int)nrb,
                       (int)rb_rows, (long long)op->n_local, (const RP*)a.row_ptr.get(), a.col.get(), d_cnt.get(), skip);
  });
  LL_HIP(hipGetLastError());
  std::vector<int32_t> cnt((size_t)ncb * nrb);
  LL_HIP(hipMemcpyAsync(cnt.data(), d_cnt.get(), cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LL_HIP(hipStreamSynchronize(s));
  return cnt;
}

// exponents of the local rows' absolute sums into rexp
template <typename T> void launch_rowexp(const ll_operator* op, int16_t* rexp) {
  const CsrImage& a = op->csr;
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((pb_rowexp_kernel<T, RP>), dim3(row_grid(op->n_local)), dim3(256), 0, op->ctx->stream, (long long)op->n_local,
                       (const RP*)a.row_ptr.get(), (const T*)a.val.get(), rexp);
  });
  LL_HIP(hipGetLastError());
}
}  // namespace

template <typename T> void csr_check_device(ll_operator* op) {
  const long long nr = op->n_local;
  const int grid = row_grid(nr);
  const DevArray<double> d_part = op->ctx->dev_alloc<double>((size_t)grid, "row-sum partials");
  const DevArray<unsigned long long> d_bad = op->ctx->dev_alloc<unsigned long long>(1, "column check");
  hipStream_t s = op->ctx->stream;
  const CsrImage& a = op->csr;
  LL_HIP(hipMemsetAsync(d_bad.get(), 0, sizeof(unsigned long long), s));
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((csr_check_kernel<T, RP>), dim3(grid), dim3(256), 0, s, nr, (long long)op->n, (const RP*)a.row_ptr.get(),
                       a.col.get(), (const T*)a.val.get(), d_part.get(), d_bad.get());
  });
  LL_HIP(hipGetLastError());
  std::vector<double> part((size_t)grid);
  unsigned long long bad = 0;
  LL_HIP(hipMemcpyAsync(part.data(), d_part.get(), (size_t)grid * sizeof(double), hipMemcpyDeviceToHost, s));
  LL_HIP(hipMemcpyAsync(&bad, d_bad.get(), sizeof(bad), hipMemcpyDeviceToHost, s));
  LL_HIP(hipStreamSynchronize(s));
  LL_REQUIRE(bad == 0, "column index out of range");
  double mx = 0.0;
  for (double v : part) mx = std::max(mx, v);
  op->inf_norm = mx;
}

// Block geometry + tables on the host (spmv_plan.hpp, O(ncb * nrb)), entry placement on the device.  Returns false when the
// image cannot be built for this shape (segment tables too large, or the LDS budget cannot hold a slice and its tables):
// the operator then keeps CSR-stream.  The image goes to op->pb only when it is complete.
template <typename T> bool pb_build_device(ll_operator* op, int phase2) {
  ll_context* ctx = op->ctx;
  const CsrImage& a = op->csr;
  const Tuning& tune = ctx->tune;
  hipStream_t s = ctx->stream;
  const int64_t nr = op->n_local;
  PbGeometry g;
  if (!pb_plan_geometry(plan_shape<T>(op), plan_tuning(tune), plan_limits(), &g)) return false;
  PbImage im;

  // ---- the diagonal leaves the image (pb_diag_kernel): one bit per CSR entry marks what the passes below skip
  DevArray<uint32_t> d_skip;
  if (tune.pb_diag && nr > 0 && op->nnz > 0) {
    const size_t words = ((size_t)op->nnz + 31) / 32 + 1;
    d_skip = ctx->dev_alloc<uint32_t>(words, "diagonal marks");
    im.diag = ctx->dev_alloc<T>(std::max<size_t>((size_t)nr, 2), "diagonal of the PB image");
    LL_HIP(hipMemsetAsync(d_skip.get(), 0, words * sizeof(uint32_t), s));
    for_row_ptr_type(a.rp64, [&](auto rp_tag) {
      using RP = decltype(rp_tag);
      hipLaunchKernelGGL((pb_diag_kernel<T, RP>), dim3(row_grid(nr)), dim3(256), 0, s, (long long)nr, (long long)op->row_begin,
                         (const RP*)a.row_ptr.get(), a.col.get(), (const T*)a.val.get(), (T*)im.diag.get(), d_skip.get());
    });
    LL_HIP(hipGetLastError());
  }
  // ---- pass 1 on the device: segment sizes; the two segment orders from them
  const DevArray<int32_t> d_cnt = ctx->dev_alloc<int32_t>((size_t)g.ncb * g.nrb, "segment counts");
  const PbSegments sg = pb_plan_segments(count_segments(op, g.map, g.ncb, g.nrb, g.rb_rows, d_skip.get(), d_cnt), g.ncb, g.nrb, g.pad);
  im.ncb = (int)g.ncb;
  im.nrb = (int)g.nrb;
  im.cb_cols = g.cb_cols;
  im.rb_rows = (int)g.rb_rows;
  im.own_count = g.own_total;
  im.entries = sg.entries;
  im.xpre = tune.pb_xpre;
  im.threads1 = tune.pb_threads1 > 0 ? tune.pb_threads1 : (std::max(1, ctx->nranks) > 1 ? 512 : kPbThreads);
  im.gather = g.gather;
  std::copy(g.chunk_first, g.chunk_first + kMaxGatherChunks, im.chunk_first);
  std::copy(g.chunk_count, g.chunk_count + kMaxGatherChunks, im.chunk_count);
  // Phase 2 form, fixed per operator at creation (LL_PB_PHASE2).  Default "fixed": order-independent fixed-point sums
  // (integer LDS adds, all waves at once) — bit-reproducible for every launch, kernel geometry and partition, and 2-5 %
  // faster than the wave-ordered form (profiles/r02_spmv_variants_run10_fixed_default.jsonl).  "ordered": floating-
  // point adds, the 16 waves in turn (barriers) — reproducible and component-wise accurate; "atomic": floating-point
  // adds in arrival order (not reproducible; A/B timing reference).
  // The caller resolves it from the accuracy request and the environment (operators.cpp image_forms).
  im.phase2 = phase2;
  upload_table(ctx, im.segq, sg.segq, "propagation-blocking tables");
  upload_table(ctx, im.segdest, sg.segdest, "propagation-blocking tables");
  upload_table(ctx, im.rptr, sg.rptr, "propagation-blocking tables");
  upload_table(ctx, im.xoff, g.xoff, "propagation-blocking tables");
  upload_table(ctx, im.ncols, g.ncols, "propagation-blocking tables");
  // 16 entries behind the image: the dump quad of phase 1 and the clamped reads of an empty last block
  const size_t cap = (size_t)sg.entries + 16;
  const PbArena ar = pb_plan_arena(cap, sizeof(T));
  im.arena = ctx->dev_alloc<void>(ar.total, "propagation-blocked image (values, indices, product buffer)");
  im.arena_bytes = ar.total;
  im.arena_static_bytes = ar.o_prod;  // everything in front of the product buffer is the matrix (copied on re-placement)
  char* base = (char*)im.arena.get();
  im.val = base + ar.o_val;
  im.col = (uint16_t*)(base + ar.o_col);
  im.row = (uint16_t*)(base + ar.o_row);
  im.prod = base + ar.o_prod;
  ctx->test_fill_if_set((T*)im.val, cap);   // (test hook: the two streams of T inside the untyped arena; the indices are never filled)
  ctx->test_fill_if_set((T*)im.prod, cap);
  LL_HIP(hipMemsetAsync(im.val, 0, cap * sizeof(T), s));  // padding entries: value 0, local indices 0
  LL_HIP(hipMemsetAsync(im.col, 0, cap * sizeof(uint16_t), s));
  LL_HIP(hipMemsetAsync(im.row, 0, cap * sizeof(uint16_t), s));
  // ---- pass 2 on the device: place the entries
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((pb_scatter_kernel<T, RP>), dim3((int)g.nrb), dim3(64), (size_t)g.ncb * sizeof(int), s, g.map, (int)g.ncb,
                       (int)g.nrb, (int)g.rb_rows, (long long)nr, (const RP*)a.row_ptr.get(), a.col.get(), (const T*)a.val.get(),
                       im.segq.get(), im.segdest.get(), (T*)im.val, im.col, im.row, nullptr, d_skip.get());
  });
  LL_HIP(hipGetLastError());
  // Fixed-point sums need per-row exponents of the absolute row sums and per-block maxima of |x|.  They are built for EVERY
  // image whose row block leaves room for them (2 bytes per row; the CSR arrays they come from may be released after creation),
  // so that ll_op_set_accuracy can move the operator between the two accuracy classes later.
  const bool fixed_fits = pb_fixed_fits(g.rb_rows, sizeof(acc_t<T>), kPbLdsCap);
  if (im.phase2 == LL_PB_FIXED)
    LL_REQUIRE(fixed_fits, "LL_PB_PHASE2=fixed: row block too large for the LDS (lower the tuning key pb_row_block)");
  if (fixed_fits) {
    im.rexp = ctx->dev_alloc<int16_t>(std::max<size_t>((size_t)nr, 8), "row exponents");
    im.blockmax = ctx->dev_alloc<double>((size_t)g.ncb, "x slice maxima");
    LL_HIP(hipMemsetAsync(im.blockmax.get(), 0, (size_t)g.ncb * sizeof(double), s));
    launch_rowexp<T>(op, im.rexp.get());
  }
  LL_HIP(hipStreamSynchronize(s));  // the host tables above go out of scope
  op->pb = std::move(im);
  return true;
}

// Build the tiled image on the device from the operator's CSR arrays.  false: the matrix is not eligible — its row
// blocks touch too many column tiles (re-staging x would cost more than the matrix stream itself: matrices without
// column locality, which keep PB) or the shape does not fit the tables — and nothing stays allocated.  The image goes to op->tl
// only when it is complete (the caller sets tl.ordered).
template <typename T> bool tl_build_device(ll_operator* op) {
  ll_context* ctx = op->ctx;
  const CsrImage& a = op->csr;
  hipStream_t s = ctx->stream;
  const int64_t nr = op->n_local;
  if (nr <= 0 || op->nnz <= 0 || ctx->nranks > kXmaxParts) return false;
  const PlanShape sh = plan_shape<T>(op);
  TlGeometry g;
  if (!tl_plan_geometry(sh, plan_tuning(ctx->tune), plan_limits(), &g)) return false;
  // ---- entries per (column tile, row block); the tile list from them
  const DevArray<int32_t> d_cnt = ctx->dev_alloc<int32_t>((size_t)g.ncb * g.nrb, "tile counts");
  const TlTiles t = tl_plan_tiles(count_segments(op, g.map, g.ncb, g.nrb, g.rb_rows, nullptr, d_cnt), g, sh, op->nnz,
                                  ctx->tune.tl_walk_modulo);
  if (t.ntiles == 0 || !(t.eligible || ctx->tune.tl_force)) return false;
  if (t.ntiles > 0x7ffffff0) return false;
  TiledImage im;
  im.nrb = (int)g.nrb;
  im.rb_rows = (int)g.rb_rows;
  im.ncb = (int)g.ncb;
  im.entries = t.entries;
  im.tiles = t.ntiles;
  im.n_interior = t.n_interior;
  DevArray<int64_t> d_segq;
  upload_table(ctx, im.first, t.tfirst, "tiled-image tables");
  upload_table(ctx, im.col, t.tcol, "tiled-image tables");
  upload_table(ctx, im.quad, t.tquad, "tiled-image tables");
  upload_table(ctx, d_segq, t.segq, "tiled-image tables");
  if (!t.rbmap.empty()) upload_table(ctx, im.rbmap, t.rbmap, "tiled-image tables");
  const size_t cap = (size_t)t.entries + 16;  // one quad behind the image: clamped reads of lanes beyond the end
  im.val = ctx->dev_alloc<T>(cap, "tiled image (values)");
  im.idx = ctx->dev_alloc<uint32_t>(cap, "tiled image (local indices)");
  im.rexp = ctx->dev_alloc<int16_t>(std::max<size_t>((size_t)nr, 8), "row exponents");
  // [0, parts): what the kernel folds; [parts, 2 parts): the own shard's partial maxima; [2 parts]: the own shard's maximum
  im.xmax = ctx->dev_alloc<double>((size_t)(2 * kXmaxParts + 8), "x maxima");
  LL_HIP(hipMemsetAsync(im.val.get(), 0, cap * sizeof(T), s));  // padding entries: value 0, local indices 0
  LL_HIP(hipMemsetAsync(im.idx.get(), 0, cap * sizeof(uint32_t), s));
  LL_HIP(hipMemsetAsync(im.xmax.get(), 0, (size_t)(2 * kXmaxParts + 8) * sizeof(double), s));
  launch_rowexp<T>(op, im.rexp.get());
  for_row_ptr_type(a.rp64, [&](auto rp_tag) {
    using RP = decltype(rp_tag);
    hipLaunchKernelGGL((pb_scatter_kernel<T, RP, true>), dim3((int)g.nrb), dim3(64), (size_t)g.ncb * sizeof(int), s, g.map, (int)g.ncb,
                       (int)g.nrb, (int)g.rb_rows, (long long)nr, (const RP*)a.row_ptr.get(), a.col.get(), (const T*)a.val.get(),
                       d_segq.get(), nullptr, (T*)im.val.get(), reinterpret_cast<uint16_t*>(im.idx.get()), nullptr, im.rexp.get());
  });
  LL_HIP(hipGetLastError());
  LL_HIP(hipStreamSynchronize(s));  // the host tables above go out of scope
  op->tl = std::move(im);
  return true;
}

#define LL_INST_IMAGE_BUILD(T)                          \
  template bool pb_build_device<T>(ll_operator*, int);  \
  template bool tl_build_device<T>(ll_operator*);       \
  template void csr_check_device<T>(ll_operator*);
LL_FOR_EACH_SCALAR(LL_INST_IMAGE_BUILD)

}  // namespace ll
