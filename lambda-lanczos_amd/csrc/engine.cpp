// Engine<T>: one operator application (exchange step + one path per image), Gram-Schmidt against a list of basis runs and the
// GEMV over the basis, with the slab storage of the Krylov basis (Basis<T>, RunList<T>).  The whole-loop drivers that call it
// are lanczos_run.cpp and expo_run.cpp (loop machinery: lanczos_loop.hpp).
#include "engine.hpp"
#include "trace.hpp"

#include <algorithm>
#include <cmath>
#include <string>

namespace ll {

// ================================================================= Basis / RunList
template <typename T> Basis<T>::~Basis() {
  // slabs go back to the context's cache: the next run() on this context reuses them instead of paying
  // hipMalloc/hipFree of tens of GB per call (ll_ctx_release_cache or ll_ctx_destroy frees them)
  const size_t bytes = (size_t)chunk_vecs * (size_t)ld * sizeof(T);
  for (T* p : chunks) ctx->cache_put((void*)p, bytes);
}
template <typename T> void Basis<T>::init(ll_context* c, int64_t n_local_, int64_t ld_, int64_t chunk_vecs_) {
  ctx = c;
  n_local = n_local_;
  ld = ld_;
  chunk_vecs = chunk_vecs_;
}
template <typename T> T* Basis<T>::vec(int64_t k) {
  const int64_t ci = k / chunk_vecs;
  while ((int64_t)chunks.size() <= ci) {
    T* p = nullptr;
    const size_t bytes = (size_t)chunk_vecs * (size_t)ld * sizeof(T);
    for (size_t i = 0; i < ctx->slab_cache.size(); ++i)
      if (ctx->slab_cache[i].second == bytes) {
        p = (T*)ctx->slab_cache[i].first;
        ctx->slab_cache.erase(ctx->slab_cache.begin() + (long)i);
        break;
      }
    if (p) {
      ctx->test_fill_if_set(p, (size_t)chunk_vecs * (size_t)ld);
      chunks.push_back(p);
      continue;
    }
    // (a 4 GiB hipMalloc was measured at 0.3-0.5 ms on every box of round 5: allocating the next slab ahead of need on a helper
    // thread changed nothing and was removed again — what does stall the loop is a hipFREE, see LoopState::begin_pass)
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e != hipSuccess && !ctx->slab_cache.empty()) {  // make room: drop cached slabs of other shapes and retry
      (void)hipGetLastError();
      for (auto& c : ctx->slab_cache) (void)hipFree(c.first);
      ctx->slab_cache.clear();
      e = hipMalloc((void**)&p, bytes);
    }
    if (e != hipSuccess) {
      set_error("out of device memory growing the Krylov basis to " + std::to_string((chunks.size() + 1) * chunk_vecs) +
                " vectors of " + std::to_string(ld * sizeof(T)) + " bytes: " + hipGetErrorString(e));
      throw Failure{LL_ERR_ALLOC};
    }
    ctx->test_fill_if_set(p, (size_t)chunk_vecs * (size_t)ld);
    chunks.push_back(p);
  }
  return chunks[ci] + (k % chunk_vecs) * ld;
}

template <typename T> std::vector<BasisSegs<T>> RunList<T>::groups(int max_vecs) const {
  std::vector<BasisSegs<T>> out;
  BasisSegs<T> cur;
  cur.nseg = 0;
  cur.ld = ld;
  int cur_vecs = 0;
  auto flush = [&]() {
    if (cur.nseg > 0) out.push_back(cur);
    cur.nseg = 0;
    cur_vecs = 0;
  };
  for (auto& r : runs) {
    const T* base = r.first;
    int left = r.second;
    while (left > 0) {
      if (cur.nseg == kMaxSegs || cur_vecs == max_vecs) flush();
      const int take = std::min(left, max_vecs - cur_vecs);
      cur.base[cur.nseg] = base;
      cur.count[cur.nseg] = take;
      ++cur.nseg;
      cur_vecs += take;
      base += (int64_t)take * ld;
      left -= take;
    }
  }
  flush();
  return out;
}

// ================================================================= Engine
template <typename T> void Engine<T>::all_reduce(double* d, size_t count) {
  if (ctx->comm == nullptr) return;
  if (ctx->profiling) {
    hipEvent_t a, b;
    LL_HIP(hipEventCreate(&a));
    LL_HIP(hipEventCreate(&b));
    LL_HIP(hipEventRecord(a, ctx->stream));
    comm_allreduce_sum(ctx->comm, d, count, ctx->stream);
    LL_HIP(hipEventRecord(b, ctx->stream));
    ctx->ev_allreduce.emplace_back(a, b);
  } else {
    comm_allreduce_sum(ctx->comm, d, count, ctx->stream);
  }
}
template <typename T> void Engine<T>::comm_timer_begin(hipStream_t cs) {
  if (!ctx->profiling) return;
  hipEvent_t a, b;
  LL_HIP(hipEventCreate(&a));
  LL_HIP(hipEventCreate(&b));
  ctx->ev_gather.emplace_back(a, b);
  LL_HIP(hipEventRecord(a, cs));
}
template <typename T> void Engine<T>::comm_timer_end(hipStream_t cs) {
  if (!ctx->profiling) return;
  LL_HIP(hipEventRecord(ctx->ev_gather.back().second, cs));
}

template <typename T> void Engine<T>::fetch(const double* d, double* host, size_t count) {
  LL_HIP(hipMemcpyAsync(host, d, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LL_HIP(hipStreamSynchronize(ctx->stream));
}

// Exchange step: every rank needs the whole x for its row block.
template <typename T>
typename Engine<T>::Gathered Engine<T>::gather_x(const T* x_local, bool x_padded, bool own_first) {
  hipStream_t s = ctx->stream;
  // Every rank sends n_shard elements (equal strides); the last shard can be shorter.  Basis vectors are padded to the
  // stride (x_padded); a caller-provided shard of exactly n_local elements is copied into a padded send buffer first (the
  // tail of the gathered buffer beyond n is never referenced by a matrix entry).
  const int P = ctx->nranks;
  const size_t shard_bytes = (size_t)op->n_shard * sizeof(T);
  ctx->ensure_xfull(shard_bytes * (size_t)(P + 1));
  T* gathered = (T*)ctx->xfull.get();
  const T* send = x_local;
  if (!x_padded && op->n_local < op->n_shard) {
    T* pad = (T*)((char*)ctx->xfull.get() + shard_bytes * (size_t)P);
    LL_HIP(hipMemsetAsync(pad, 0, shard_bytes, s));
    LL_HIP(hipMemcpyAsync(pad, x_local, (size_t)op->n_local * sizeof(T), hipMemcpyDeviceToDevice, s));
    send = pad;
  }
  // PB: the gather is cut into chunks (op->pb.gather) laid out chunk-major; every other kernel needs global order
  const bool pb = op->kind == ll_operator::CSR && op->spmv_kind == LL_SPMV_PB;
  GatherPlan plan = pb ? op->pb.gather : GatherPlan();
  if (!pb) plan.len[0] = op->n_shard;
  const bool overlap = own_first && ctx->tune.comm_overlap && ctx->comm_stream != nullptr;
  hipStream_t cs = overlap ? ctx->comm_stream : s;
  // tiled, fixed-point class: the grid's scale needs max |x| over the WHOLE vector before the first launch — every rank's own
  // maximum (two small kernels) travels in an 8-byte all-gather in front of the vector's
  const bool tl_max = op->kind == ll_operator::CSR && op->spmv_kind == LL_SPMV_TILED && !op->tl.ordered;
  if (tl_max) launch_tl_xmax_local<T>(*op, send, s);
  comm_timer_begin(cs);
  if (overlap) {
    LL_HIP(hipEventRecord(ctx->ev_x_ready, s));  // everything enqueued so far (x final, previous readers of the
    LL_HIP(hipStreamWaitEvent(cs, ctx->ev_x_ready, 0));  // gathered buffer done) precedes the gather
  }
  if (tl_max) {
    comm_allgather(ctx->comm, op->tl.xmax.get() + tl_xmax_local_slot(), op->tl.xmax.get(), sizeof(double), cs);
    if (overlap) LL_HIP(hipEventRecord(ctx->ev_xmax, cs));
  }
  for (int c = 0; c < plan.nchunks; ++c) {
    comm_allgather(ctx->comm, send + plan.start[c], gathered + (int64_t)P * plan.start[c], (size_t)plan.len[c] * sizeof(T), cs);
    if (overlap) LL_HIP(hipEventRecord(ctx->ev_chunk[c], cs));
  }
  comm_timer_end(cs);
  return Gathered{send, gathered, overlap, overlap && tl_max ? ctx->ev_xmax : nullptr, ctx->ev_chunk, plan.nchunks};
}

template <typename T>
void Engine<T>::apply(const T* x_local, T* y, double offset, double* d_alpha, bool x_padded, DeferredAlpha* defer,
                      const ScaleIn<T>* sc, const double* xnorm2) {
  TraceRange trace("ll::apply (mv_mul + offset + alpha)");
  const InputCaps caps = input_caps();
  LL_REQUIRE(sc == nullptr || caps.defer, "internal: this operator cannot normalise its input on the fly");
  LL_REQUIRE(xnorm2 == nullptr || ((caps.norm2 || caps.scale_in) && sc == nullptr), "internal: this operator cannot scale its input");
  const ScaleIn<T> from_norm{xnorm2, 1};  // the norm as a one-element list of "partials" (nothing published)
  if (xnorm2 && caps.scale_in) sc = &from_norm;
  ctx->ensure_alpha_partials(std::max<size_t>(kMaxSpmvGrid, (size_t)std::max({op->pb.nrb, op->tl.nrb, op->sym.nrb})));
  double* const dotp = d_alpha ? ctx->alpha_partials.get() : nullptr;
  // dense row block: split by column range without a second image, but only when the shard's column range starts and
  // ends on 16-byte pieces of the rows (with an unaligned boundary both parts would take the scalar path of
  // dense_mv_kernel, and gather-then-multiply, which vectorises whole rows, is faster)
  constexpr int64_t V = (int64_t)(16 / sizeof(T)) > 0 ? (int64_t)(16 / sizeof(T)) : 1;
  const bool dense_split_ok = op->n % V == 0 && op->row_begin % V == 0 && (op->row_begin + op->n_local) % V == 0;
  int nparts;
  if (op->kind == ll_operator::STENCIL) nparts = apply_lattice(x_local, y, offset, dotp, sc);
  else if (op->is_pauli())  // a sum of Pauli strings, whole or on a block: single GPU only (creation refuses sharded contexts)
    nparts = launch_pauli_op<T>(*op, x_local, y, offset, dotp, ctx->stream, sc);
  else if (op->kind == ll_operator::DENSE)
    nparts = apply_rows(&launch_dense_mv<T>, ctx->tune.csr_split && dense_split_ok, x_local, x_padded, y, offset, dotp, sc);
  else if (op->kind != ll_operator::CSR) nparts = apply_callback(x_local, y, offset, dotp);
  else if (op->spmv_kind == LL_SPMV_PB) nparts = apply_pb(x_local, x_padded, y, offset, dotp, xnorm2);
  else if (op->spmv_kind == LL_SPMV_TILED) nparts = apply_tiled(x_local, x_padded, y, offset, dotp, xnorm2);
  else if (op->spmv_kind == LL_SPMV_SYM)  // one-triangle image: single GPU only (creation refuses sharded contexts)
    nparts = launch_spmv_sym<T>(*op, x_local, y, offset, dotp, ctx->stream, xnorm2);
  else {  // CSR-stream: the column-split image (operators.cpp build_csr_split) on sharded contexts
    LL_REQUIRE((ctx->comm != nullptr && op->csr_split()) || op->csr.col || op->nnz == 0,
               "this operator kept only its column-split image (created on a sharded context) and needs that communicator");
    nparts = apply_rows(&launch_spmv<T>, op->csr_split(), x_local, x_padded, y, offset, dotp, sc);
  }
  if (d_alpha) {
    if (defer && ctx->comm == nullptr) {  // the caller's multi-dot folds them
      defer->partials = dotp;
      defer->nparts = nparts;
    } else {
      launch_reduce_cols(dotp, nparts, 1, d_alpha, nullptr, ctx->stream);
      all_reduce(d_alpha, 1);
    }
  }
}

// CSR-stream and dense: the whole image, on the gathered vector when sharded.  split: the own-column product (no exchange
// needed) runs under the gather, the other ranks' columns are added when the gathered vector has arrived;
// LL_COMM_OVERLAP=0 issues the same two kernels behind the gather on one stream.
template <typename T>
int Engine<T>::apply_rows(RowLauncher launch, bool split, const T* x, bool x_padded, T* y, double offset, double* dotp,
                          const ScaleIn<T>* sc) {
  hipStream_t s = ctx->stream;
  if (ctx->comm == nullptr) return launch(*op, x, x, y, offset, dotp, s, sc, 0);
  const Gathered g = gather_x(x, x_padded, split);
  if (!split) return launch(*op, g.x_full, x, y, offset, dotp, s, sc, 0);
  launch(*op, x, x, y, offset, nullptr, s, sc, 1);
  wait(g.whole());
  return launch(*op, g.x_full, x, y, offset, dotp, s, sc, 2);
}

// Lattice: no all-gather — one hyperplane from each ring neighbour
template <typename T> int Engine<T>::apply_lattice(const T* x, T* y, double offset, double* dotp, const ScaleIn<T>* sc) {
  hipStream_t s = ctx->stream;
  const int64_t H = op->st_halo;
  if (ctx->comm == nullptr)  // the shard is the whole lattice: the ring neighbours are its own ends
    return launch_stencil<T>(*op, x, x + (n_local - H), x, y, offset, dotp, s, sc);
  const size_t hb = (size_t)H * sizeof(T);
  ctx->ensure_halo(2 * hb);
  T* rlo = (T*)ctx->halo.get();
  T* rhi = rlo + H;
  const bool ring = op->st.periodic[0] != 0;
  const int prev = ctx->rank > 0 ? ctx->rank - 1 : (ring ? ctx->nranks - 1 : -1);
  const int next = ctx->rank + 1 < ctx->nranks ? ctx->rank + 1 : (ring ? 0 : -1);
  comm_timer_begin(s);
  comm_halo_exchange(ctx->comm, x, rlo, prev, x + (n_local - H), rhi, next, hb, s);
  comm_timer_end(s);
  return launch_stencil<T>(*op, x, rlo, rhi, y, offset, dotp, s, sc);
}

// PB: one call, or the own-column blocks under the gather and every chunk's remote blocks when that chunk has arrived
template <typename T>
int Engine<T>::apply_pb(const T* x, bool x_padded, T* y, double offset, double* dotp, const double* xnorm2) {
  hipStream_t s = ctx->stream;
  if (ctx->comm == nullptr) return launch_spmv_pb<T>(*op, x, x, x, y, offset, dotp, s, xnorm2);
  const Gathered g = gather_x(x, x_padded, true);
  launch_pb_phase1<T>(*op, 0, op->pb.own_count, g.x_own, s, xnorm2);
  for (int c = 0; c < op->pb.gather.nchunks; ++c) {
    wait(g.chunk(c));
    launch_pb_phase1<T>(*op, op->pb.chunk_first[c], op->pb.chunk_count[c], g.x_full, s, xnorm2);
  }
  return launch_pb_phase2<T>(*op, x, y, offset, dotp, s, xnorm2);
}

// Tiled: one launch on the whole x, or two passes — the row blocks whose tiles are all own-column tiles run under the
// gather (x = the own shard), the others when the vector has arrived; LL_COMM_OVERLAP=0 issues the same two launches
// behind the gather on one stream
template <typename T>
int Engine<T>::apply_tiled(const T* x, bool x_padded, T* y, double offset, double* dotp, const double* xnorm2) {
  hipStream_t s = ctx->stream;
  if (ctx->comm == nullptr) return launch_spmv_tiled<T>(*op, x, y, offset, dotp, s, xnorm2);
  const Gathered g = gather_x(x, x_padded, true);
  const int P = ctx->nranks;
  wait(g.xmax);  // (fixed-point class: the scale of the grid)
  launch_spmv_tiled_pass<T>(*op, 0, g.x_own, op->row_begin, op->row_begin + op->n_shard, x, y, offset, dotp, s, xnorm2, P);
  wait(g.whole());
  return launch_spmv_tiled_pass<T>(*op, 1, g.x_full, 0, op->n, x, y, offset, dotp, s, xnorm2, P);
}

// LL_ITER_TRACE: what the user's code saw and returned (a stale or torn buffer shows here)
template <typename T> static void trace_callback(const std::string& path, const T* x, const void* h_in, const void* h_out, int64_t n) {
  FILE* f = std::fopen(path.c_str(), "a");
  if (!f) return;
  double sin2 = 0.0, sout2 = 0.0, dot = 0.0;
  const typename scalar_traits<T>::real* a = (const typename scalar_traits<T>::real*)h_in;
  const typename scalar_traits<T>::real* b = (const typename scalar_traits<T>::real*)h_out;
  for (int64_t i = 0; i < n * scalar_traits<T>::reals; ++i) {
    sin2 += (double)a[i] * a[i];
    sout2 += (double)b[i] * b[i];
    dot += (double)a[i] * b[i];
  }
  std::fprintf(f, "cb x=%p |in|^2=%.17g |out|^2=%.17g <in,out>=%.17g\n", (const void*)x, sin2, sout2, dot);
  std::fclose(f);
}

// Host and device callbacks, then offset and alpha partials in a kernel of their own
template <typename T> int Engine<T>::apply_callback(const T* x, T* y, double offset, double* dotp) {
  LL_REQUIRE(ctx->comm == nullptr, "callback operators are not supported on sharded contexts");
  hipStream_t s = ctx->stream;
  const size_t bytes = (size_t)n_local * sizeof(T);
  if (op->kind == ll_operator::HOST_CB) {
    // unmodified user code (LL:120-126): one D2H + one H2D of an n-vector per call
    // through the context's pinned callback buffers [in | out]: full-rate DMA, no pageable bounce copies
    char* h_in = (char*)ctx->ensure_cb_stage(2 * bytes);
    char* h_out = h_in + bytes;
    if (ctx->ev_cb) LL_HIP(hipEventSynchronize(ctx->ev_cb));  // the previous call's upload out of h_out has finished
    LL_HIP(hipMemcpyAsync(h_in, x, bytes, hipMemcpyDeviceToHost, s));
    std::memset(h_out, 0, bytes);  // "out" is zero-filled on entry (LL:242, EX:107); overlaps the copy above
    LL_HIP(hipStreamSynchronize(s));
    int rc = op->host_fn(h_in, h_out, n_local, op->user);
    if (rc != 0) {
      set_error("mv_mul host callback returned " + std::to_string(rc));
      throw Failure{LL_ERR_CALLBACK};
    }
    if (!ctx->tune.iter_trace.empty()) trace_callback(ctx->tune.iter_trace, x, h_in, h_out, n_local);
    // no second synchronisation: the next callback waits for this upload (ev_cb) before it reuses the buffer
    LL_HIP(hipMemcpyAsync(y, h_out, bytes, hipMemcpyHostToDevice, s));
    if (!ctx->ev_cb) LL_HIP(hipEventCreateWithFlags(&ctx->ev_cb, hipEventDisableTiming));
    LL_HIP(hipEventRecord(ctx->ev_cb, s));
  } else {
    LL_HIP(hipMemsetAsync(y, 0, bytes, s));
    int rc = op->dev_fn(x, y, n_local, (void*)s, op->user);
    if (rc != 0) {
      set_error("mv_mul device callback returned " + std::to_string(rc));
      throw Failure{LL_ERR_CALLBACK};
    }
  }
  return launch_offset_dot<T>(n_local, x, y, offset, dotp, s);
}

template <typename T> void Engine<T>::norm2_dev(const T* v, double* d_out) {
  ctx->ensure_partials((size_t)kMaxGrid * R);
  const int grid = launch_dot<T>(n_local, v, v, ctx->partials.get(), ctx->stream);
  ctx->ensure_h(4);
  if (R == 1) {
    launch_reduce_cols(ctx->partials.get(), grid, 1, d_out, nullptr, ctx->stream);
  } else {  // real part is column 0
    launch_reduce_cols(ctx->partials.get(), grid, R, ctx->h.get(), nullptr, ctx->stream);
    launch_copy_scalar(d_out, ctx->h.get(), ctx->stream);
  }
  all_reduce(d_out, 1);
}

template <typename T> void Engine<T>::dot_dev(const T* a, const T* b, double* d_out) {
  ctx->ensure_partials((size_t)kMaxGrid * R);
  const int grid = launch_dot<T>(n_local, a, b, ctx->partials.get(), ctx->stream);
  launch_reduce_cols(ctx->partials.get(), grid, R, d_out, nullptr, ctx->stream);
  all_reduce(d_out, R);
}

// ================================================================= Gram-Schmidt in two sweeps
// How a pass ends, given where the partial sums of ||w||^2 lie (c0: what is published as the norm before the pass, nullable)
// and what the loop asked for: a single GPU can leave the fold to the caller's normalisation kernel or publish from the fold;
// a communicator, or no request, takes the plain fold and the all-reduce.
template <typename T>
typename Engine<T>::PassEnding Engine<T>::close_pass(const double* partials, int nparts, const double* c0, double* c, const PassRequest* req) {
  const bool publishes = req && ctx->comm == nullptr;
  if (publishes && req->caller_normalises) return PartialsPending{partials, nparts, c0, c + 1};
  if (publishes) {
    launch_reduce_publish(partials, nparts, c + 1, req->alpha, c0, req->host, ctx->stream);
    return Published{};
  }
  launch_reduce_cols(partials, nparts, 1, c + 1, nullptr, ctx->stream);
  all_reduce(c + 1, 1);
  return Folded{};
}

// three-term update (if any) + ||w||^2 only
template <typename T>
typename Engine<T>::PassEnd Engine<T>::three_term_only(T* w, int64_t ld, const ThreeTerm<T>& tt, double* c, const PassRequest* req) {
  ctx->ensure_partials(kMaxGrid);
  const int grid = launch_mdot<T>(n_local, w, no_segs<T>(ld), tt, nullptr, ctx->partials.get(), ctx->tune.blas_small_bytes, ctx->stream);
  return PassEnd{plain_norm(c + 1), close_pass(ctx->partials.get(), grid, nullptr, c, req)};
}

// The reference's operation order (LA:132-144): for every basis vector h = <u,w>; w -= h u, strictly sequential.
template <typename T> NormRefs Engine<T>::mgs_sweep(T* w, const RunList<T>& runs, const ThreeTerm<T>& tt, double* c, double* h_total) {
  hipStream_t s = ctx->stream;
  double* h1 = ctx->h.get();
  ctx->ensure_partials((size_t)kMaxGrid * (R + 1));
  if (tt.u_cur) launch_mdot<T>(n_local, w, no_segs<T>(runs.ld), tt, nullptr, ctx->partials.get(), ctx->tune.blas_small_bytes, s);
  int grid = 0;
  for (const BasisSegs<T>& one : runs.groups(1)) {  // one vector per launch
    grid = launch_mdot<T>(n_local, w, one, ThreeTerm<T>::none(), nullptr, ctx->partials.get(), ctx->tune.blas_small_bytes, s);
    launch_reduce_cols(ctx->partials.get(), grid, R + 1, h1, S(kScalSpare), s);
    all_reduce(h1, R);
    grid = launch_maxpy<T>(n_local, w, one, h1, nullptr, ctx->partials.get(), ctx->tune.blas_small_bytes, s);
    h1 += R;
  }
  launch_reduce_cols(ctx->partials.get(), grid, 1, c + 1, nullptr, s);
  all_reduce(c + 1, 1);
  if (h_total) LL_HIP(hipMemcpyAsync(h_total, ctx->h.get(), (size_t)R * runs.total() * sizeof(double), hipMemcpyDeviceToDevice, s));
  return plain_norm(c + 1);
}

// pass 1: h = U^H w (+ fused three-term update and ||w||^2), then w -= U h (+ fused ||w||^2)
template <typename T>
typename Engine<T>::PassEnd Engine<T>::cgs_first_pass(T* w, const std::vector<BasisSegs<T>>& groups, int nb, const ThreeTerm<T>& tt,
                                                      double* c, bool derive, const PassRequest* req) {
  hipStream_t s = ctx->stream;
  const bool sharded = ctx->comm != nullptr;
  double* h1 = ctx->h.get();
  size_t max_cols = 1;
  for (auto& g : groups) max_cols = std::max(max_cols, (size_t)R * g.total() + 1);
  ctx->ensure_partials((size_t)kMaxGrid * max_cols);
  int off = 0, grid = 0;
  double* norm_partials = ctx->partials.get();  // where the multi-axpy leaves the partial sums of ||w'||^2
  bool folded_in_maxpy = false;
  for (size_t g = 0; g < groups.size(); ++g) {
    const int nbg = groups[g].total();
    const int mgrid = launch_mdot<T>(n_local, w, groups[g], g == 0 ? tt : ThreeTerm<T>::none(), nullptr, ctx->partials.get(),
                                     ctx->tune.blas_small_bytes, s);
    if (groups.size() == 1 && !sharded && ctx->tune.fuse_launches) {
      // small vectors, small grids: the multi-axpy folds the coefficients itself (one launch less per iteration)
      if (!ctx->norm_partials) ctx->norm_partials = ctx->dev_alloc<double>((size_t)kMaxGrid, "norm partials");
      folded_in_maxpy = launch_maxpy_folding<T>(n_local, w, groups[0], ctx->partials.get(), mgrid, h1, c, ctx->norm_partials.get(),
                                                ctx->tune.blas_small_bytes, &grid, s);
      if (folded_in_maxpy) norm_partials = ctx->norm_partials.get();
    }
    if (!folded_in_maxpy)
      launch_reduce_cols(ctx->partials.get(), mgrid, R * nbg + 1, h1 + R * off, (g + 1 == groups.size() && !sharded) ? c : nullptr, s);
    off += nbg;
  }
  if (sharded) {  // one all-reduce for all coefficients and the norm (latency-sized)
    all_reduce(h1, (size_t)R * nb + 1);
    if (!derive) launch_copy_scalar(c, h1 + R * nb, s);  // (derive: copied by the derive kernel after the update)
  }
  off = 0;
  for (size_t g = 0; g < groups.size() && !folded_in_maxpy; ++g) {
    grid = launch_maxpy<T>(n_local, w, groups[g], h1 + R * off, nullptr, ctx->partials.get(), ctx->tune.blas_small_bytes, s);
    off += groups[g].total();
  }
  const NormRefs refs{c, c + 1, c + 1, 0};  // final norm = c1
  if (!derive) return PassEnd{refs, close_pass(norm_partials, grid, c, c, req)};
  // ... inside the caller's normalisation kernel (launch_scale_derive), or in one small launch: norm + copy of ||w||^2 + (with a
  // request) the publish step
  if (req && req->caller_normalises) return PassEnd{refs, DerivePending{h1 + R * nb, h1, R * nb, c, c + 1}};
  launch_derive_norm(h1 + R * nb, h1, R * nb, c, c + 1, req ? req->alpha : nullptr, req ? req->host : nullptr, s);
  return PassEnd{refs, req ? PassEnding(Published{}) : PassEnding(Folded{})};
}

// pass 2: always (CGS2: pred null) or only when ||w|| dropped below ||w_before||/sqrt(2) (DGKS); decided on the device
template <typename T>
void Engine<T>::cgs_second_pass(T* w, const std::vector<BasisSegs<T>>& groups, int nb, const NormRefs* pred, double* c) {
  hipStream_t s = ctx->stream;
  double* h2 = ctx->h.get() + (R * nb + 2);
  int off = 0, grid = 0;
  for (auto& g : groups) {
    const int g2 = launch_mdot<T>(n_local, w, g, ThreeTerm<T>::none(), pred, ctx->partials.get(), ctx->tune.blas_small_bytes, s);
    launch_reduce_cols(ctx->partials.get(), g2, R * g.total() + 1, h2 + R * off, S(kScalSpare), s);
    off += g.total();
  }
  if (ctx->comm != nullptr) all_reduce(h2, (size_t)R * nb);
  off = 0;
  for (auto& g : groups) {
    grid = launch_maxpy<T>(n_local, w, g, h2 + R * off, pred, ctx->partials.get(), ctx->tune.blas_small_bytes, s);
    off += g.total();
  }
  launch_reduce_cols(ctx->partials.get(), grid, 1, c + 2, nullptr, s);
  all_reduce(c + 2, 1);
}

template <typename T>
NormRefs Engine<T>::orth(T* w, const RunList<T>& runs, int mode, const ThreeTerm<T>& tt, double* c, double* h_total) {
  TraceRange trace("ll::orth (three-term + Gram-Schmidt + norm)");
  const int nb = runs.total();
  ctx->ensure_h((size_t)2 * (R * nb + 2));  // the coefficients of pass 1, then those of pass 2
  if (nb == 0) return three_term_only(w, runs.ld, tt, c, nullptr).refs;
  if (mode == LL_ORTH_MGS) return mgs_sweep(w, runs, tt, c, h_total);
  const std::vector<BasisSegs<T>> groups = runs.groups(max_vecs_per_launch<T>());
  const NormRefs refs{c, c + 1, c + 2, mode == LL_ORTH_CGS2 ? 1 : 0, ctx->tune.dgks_threshold};
  const NormRefs* pred = mode == LL_ORTH_CGS2 ? nullptr : &refs;
  cgs_first_pass(w, groups, nb, tt, c, /* derive: never, the device's test of pass 2 compares measured norms */ false, nullptr);
  cgs_second_pass(w, groups, nb, pred, c);
  if (h_total) {
    LL_HIP(hipMemcpyAsync(h_total, ctx->h.get(), (size_t)R * nb * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    launch_accumulate_h(h_total, ctx->h.get() + (R * nb + 2), R * nb, pred, ctx->stream);
  }
  return refs;
}

template <typename T>
typename Engine<T>::PassEnd Engine<T>::orth_pass(T* w, const RunList<T>& runs, int mode, const ThreeTerm<T>& tt, double* c,
                                                 const PassRequest* req) {
  const int nb = runs.total();
  if (nb > 0 && mode != LL_ORTH_CGS_DGKS) return PassEnd{orth(w, runs, mode, tt, c, nullptr), Folded{}};
  TraceRange trace("ll::orth (three-term + Gram-Schmidt + norm)");
  ctx->ensure_h((size_t)2 * (R * nb + 2));
  if (nb == 0) return three_term_only(w, runs.ld, tt, c, req);
  // Sharded whole-loop passes: the norm after the pass follows from what the one all-reduce of the pass delivers
  // (||w'||^2 = ||w||^2 - sum |h_j|^2 for an orthonormal basis) — one all-reduce per iteration less.  Its relative error
  // is eps * ||w||^2 / ||w'||^2, i.e. a few eps whenever the DGKS test (evaluated on these two numbers) does not ask
  // for a second pass anyway.  LL_SHARDED_NORM=measured restores the reduced-and-all-reduced partial norms of maxpy.
  return cgs_first_pass(w, runs.groups(max_vecs_per_launch<T>()), nb, tt, c, ctx->comm != nullptr && !ctx->tune.sharded_norm_measured, req);
}

template <typename T> double Engine<T>::second_pass(T* u, const RunList<T>& runs) {
  const NormRefs r = orth_pass(u, runs, LL_ORTH_CGS_DGKS, ThreeTerm<T>::none(), S(kScalScratch), nullptr).refs;
  launch_scale<T>(n_local, u, 0.0, &r, ctx->stream);
  double shrink = 0.0;
  fetch(r.c1, &shrink, 1);
  return shrink;
}

template <typename T>
void Engine<T>::gemv(const RunList<T>& basis, int64_t m, int nout, const T* coeff_host, T* out, int64_t ld_out) {
  typedef acc_t<T> A;
  std::vector<A> wide((size_t)nout * m);
  for (size_t i = 0; i < wide.size(); ++i) {  // exact: every T is representable in acc_t<T>
    if constexpr (std::is_same<A, T>::value) wide[i] = coeff_host[i];
    else if constexpr (scalar_traits<T>::is_complex) wide[i] = A{(double)coeff_host[i].re, (double)coeff_host[i].im};
    else wide[i] = (double)coeff_host[i];
  }
  gemv_acc(basis, m, nout, wide.data(), out, ld_out);
}
template <typename T>
void Engine<T>::gemv_acc(const RunList<T>& basis, int64_t m, int nout, const acc_t<T>* coeff_host, T* out, int64_t ld_out) {
  TraceRange trace("ll::gemv_basis (Ritz vectors / exp output)");
  typedef acc_t<T> A;
  const std::vector<BasisSegs<T>> groups = basis.groups(512);
  ctx->ensure_coeff((size_t)nout * m * sizeof(A));
  LL_HIP(hipMemcpyAsync(ctx->coeff.get(), coeff_host, (size_t)nout * m * sizeof(A), hipMemcpyHostToDevice, ctx->stream));
  // float types over more than one basis group: the partial sums stay in double between the launches
  DevArray<double> scratch;
  if (!std::is_same<A, T>::value && groups.size() > 1)
    scratch = ctx->dev_alloc<double>((size_t)nout * n_local * scalar_traits<T>::reals, "gemv partial sums");
  launch_gemv_basis<T>(n_local, m, groups.data(), (int)groups.size(), nout, (const A*)ctx->coeff.get(), out, ld_out,
                       reinterpret_cast<A*>(scratch.get()), ctx->stream);
  LL_HIP(hipStreamSynchronize(ctx->stream));  // coeff_host may go away; d_coeff is reused; scratch is released after this
}

// Vectors per basis slab.  The reference's initial_vector_size (LL:181, default 200) only RESERVES the outer
// std::vector; its Lanczos vectors are allocated one by one.  Here a slab is one hipMalloc, so it is capped by BYTES
// (4 GiB, LL_SLAB_BYTES overrides): a run that converges after 30 iterations of an n = 1e8 problem must not need
// 200 vectors of HBM up front.  Slabs are appended on demand and cached in the context between runs.
int64_t pick_chunk_vecs(int64_t initial_vector_size, int64_t max_iteration, int64_t vec_bytes, int64_t cap_bytes) {
  int64_t want = initial_vector_size > 0 ? initial_vector_size : 200;
  want = std::min(want, max_iteration + 2);
  want = std::min(want, cap_bytes / std::max<int64_t>(vec_bytes, 1));
  return std::max<int64_t>(want, 4);
}

// Bytes of one Krylov-basis slab of a run with default parameters on this operator (initial_vector_size = 200, max_iteration = n):
// what operator creation sizes its spare placement candidates to, so that they can serve as the first basis slabs (operators.cpp).
int64_t default_slab_bytes(int64_t n, int64_t n_local, int64_t n_shard, int elem_bytes, const Tuning& tune) {
  const int64_t ld = round_up(std::max(n_local, n_shard), 256);
  const int64_t vec_bytes = ld * (int64_t)elem_bytes;
  return pick_chunk_vecs(200, std::max<int64_t>(n, 1), vec_bytes, tune.slab_bytes) * vec_bytes;
}

#define LL_INST_ENGINE(T)    \
  template struct Basis<T>;   \
  template struct RunList<T>; \
  template struct Engine<T>;
LL_FOR_EACH_SCALAR(LL_INST_ENGINE)

}  // namespace ll
