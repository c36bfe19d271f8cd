// Operator construction: the images of a CSR matrix (upload, SpMV tiles, the column split, the PB and tiled builds, their
// creation-time timing and the kernel choice), the one-triangle and COO forms, the dense, lattice, Pauli-string and callback operators, and the
// accuracy policy that gives every image its form.  The extern "C" entry points (capi.cpp, documented in include/lanczos_hip.h)
// call in here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace ll {
namespace {

inline double abs2_host(double v) { return v * v; }
inline double abs2_host(float v) { return (double)v * (double)v; }
inline double abs2_host(zc v) { return v.re * v.re + v.im * v.im; }
inline double abs2_host(cf v) { return (double)v.re * (double)v.re + (double)v.im * (double)v.im; }
// the device's abs1 / abs2 (dev_helpers.hpp) on the host, operation for operation (row exponents and norm of a stored triangle)
inline double abs1_host(double v) { return std::fabs(v); }
inline double abs1_host(float v) { return std::fabs((double)v); }
inline double abs1_host(zc v) { return std::fabs(v.re) + std::fabs(v.im); }
inline double abs1_host(cf v) { return std::fabs((double)v.re) + std::fabs((double)v.im); }
inline double abs2_fma_host(double v) { return v * v; }
inline double abs2_fma_host(float v) { return (double)v * (double)v; }
inline double abs2_fma_host(zc v) { return std::fma(v.re, v.re, v.im * v.im); }
inline double abs2_fma_host(cf v) { return std::fma((double)v.re, (double)v.re, (double)v.im * (double)v.im); }

// SpMV tiles: runs of whole rows with <= cap nonzeros and <= kBlock rows; a longer row is alone.
void build_tiles_cap(const int64_t* rp, int64_t nrows, int64_t cap, std::vector<int32_t>& tiles) {
  tiles.clear();
  tiles.push_back(0);
  int64_t r = 0;
  while (r < nrows) {
    int64_t r1 = r;
    while (r1 < nrows && (r1 - r) < kBlock && rp[r1 + 1] - rp[r] <= cap) ++r1;
    if (r1 == r) r1 = r + 1;
    tiles.push_back((int32_t)r1);
    r = r1;
  }
}
// The kernel walks the tiles with a persistent grid of at most `grid_cap` workgroups, every workgroup the same number of
// tiles +-1 (TileWalk).  With only a few tiles per workgroup that +-1 is a large share of the kernel: config 2 (4 880
// tiles of 1 024 nonzeros on 2 048 workgroups) runs three rounds of which the last is 38 % full.  So when fewer than
// eight rounds are needed the tile size is lowered until the tiles fill whole rounds: every workgroup then walks exactly
// `rounds` tiles, each a little shorter: config 2's SpMV 18.35 -> 17.37 us (54.5 -> 57.5 % of the roofline).  Only from three
// rounds up: a tile costs mostly latency, so with one or two rounds (config 5: 4 883 tiles on 4 096 workgroups) a few
// workgroups walking a second full tile are cheaper than all of them walking two shorter ones (25.0 -> 30.6 us when
// balanced; gpurun A/B of round 4).  (LL_SPMV_TILE_BALANCE=0: always kSpmvTileNnz.)
void build_tiles(const int64_t* rp, int64_t nrows, std::vector<int32_t>& tiles, int grid_cap = 0, bool balance = true) {
  build_tiles_cap(rp, nrows, kSpmvTileNnz, tiles);
  const int64_t nt = (int64_t)tiles.size() - 1;
  if (!balance || grid_cap <= 0 || nt <= grid_cap / 2 || nt >= 8 * (int64_t)grid_cap) return;
  const int64_t rounds = (nt + grid_cap - 1) / grid_cap;
  if (rounds < 3) return;
  const int64_t nnz = rp[nrows];
  // rows do not cut evenly: shrink the cap until the tile count fits rounds x grid (a few tries)
  for (double slack : {0.995, 0.97, 0.94, 0.90}) {
    const int64_t cap = std::max<int64_t>(64, std::min<int64_t>(kSpmvTileNnz, (int64_t)((double)nnz / ((double)rounds * grid_cap * slack)) + 1));
    std::vector<int32_t> t;
    build_tiles_cap(rp, nrows, cap, t);
    if ((int64_t)t.size() - 1 <= rounds * grid_cap) {
      tiles.swap(t);
      return;
    }
  }
}

// The index of a CSR image of nr rows from its host row offsets: the SpMV tiles, and the row offsets in 32 bit, or in 64 bit
// when im.rp64.
template <typename T>
void upload_csr_index(ll_context* ctx, CsrImage& im, const int64_t* rp, int64_t nr, const char* what_rp, const char* what_tiles) {
  std::vector<int32_t> tiles;
  build_tiles(rp, nr, tiles, sizeof(T) >= 16 ? kMaxSpmvGrid : kMaxGrid, ctx->tune.spmv_tile_balance);
  im.ntiles = (int)tiles.size() - 1;
  im.tiles = ctx->dev_alloc<int32_t>(tiles.size(), what_tiles);
  LL_HIP(hipMemcpy(im.tiles.get(), tiles.data(), tiles.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  if (im.rp64) {
    im.row_ptr = ctx->dev_alloc<int64_t>((size_t)nr + 1, what_rp);
    LL_HIP(hipMemcpy(im.row_ptr.get(), rp, (size_t)(nr + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  } else {
    std::vector<int32_t> rp32((size_t)nr + 1);
    for (int64_t i = 0; i <= nr; ++i) rp32[(size_t)i] = (int32_t)rp[i];
    im.row_ptr = ctx->dev_alloc<int32_t>((size_t)nr + 1, what_rp);
    LL_HIP(hipMemcpy(im.row_ptr.get(), rp32.data(), (size_t)(nr + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  }
}

// Sharded contexts that keep the CSR-stream kernel: split the image by column ownership so that the own-column product
// runs under the all-gather (the PB image has its own own / remote block ranges).  Built on the device from
// the CSR arrays (they may never have been on the host); one int32 per row crosses the bus for the prefix sums.
template <typename T> void build_csr_split(ll_operator* op) {
  ll_context* ctx = op->ctx;
  hipStream_t s = ctx->stream;
  const int64_t nr = op->n_local;
  const bool rp64 = op->csr.rp64;
  if (nr <= 0 || !op->csr.row_ptr) return;
  const DevArray<int32_t> d_cnt = ctx->dev_alloc<int32_t>((size_t)nr, "own-column counts");
  launch_csr_count_own<T>(*op, d_cnt.get(), s);
  std::vector<int32_t> cnt((size_t)nr);
  std::vector<int64_t> rp((size_t)nr + 1);
  LL_HIP(hipMemcpyAsync(cnt.data(), d_cnt.get(), (size_t)nr * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (rp64) {
    LL_HIP(hipMemcpyAsync(rp.data(), op->csr.row_ptr.get(), (size_t)(nr + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    LL_HIP(hipStreamSynchronize(s));
  } else {
    std::vector<int32_t> rp32((size_t)nr + 1);
    LL_HIP(hipMemcpyAsync(rp32.data(), op->csr.row_ptr.get(), (size_t)(nr + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LL_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i <= nr; ++i) rp[(size_t)i] = rp32[(size_t)i];
  }
  std::vector<int64_t> rp_own((size_t)nr + 1), rp_rem((size_t)nr + 1);
  rp_own[0] = rp_rem[0] = 0;
  for (int64_t i = 0; i < nr; ++i) {
    rp_own[(size_t)i + 1] = rp_own[(size_t)i] + cnt[(size_t)i];
    rp_rem[(size_t)i + 1] = rp_rem[(size_t)i] + (rp[(size_t)i + 1] - rp[(size_t)i] - cnt[(size_t)i]);
  }
  CsrImage own, rem;
  own.rp64 = rem.rp64 = rp64;
  upload_csr_index<T>(ctx, own, rp_own.data(), nr, "split row offsets", "split SpMV tiles");
  upload_csr_index<T>(ctx, rem, rp_rem.data(), nr, "split row offsets", "split SpMV tiles");
  const size_t n_own = (size_t)rp_own[(size_t)nr], n_rem = (size_t)rp_rem[(size_t)nr];
  own.col = ctx->dev_alloc<int32_t>(std::max<size_t>(n_own, 1), "own-column indices");
  own.val = ctx->dev_alloc<T>(std::max<size_t>(n_own, 1), "own-column values");
  rem.col = ctx->dev_alloc<int32_t>(std::max<size_t>(n_rem, 1), "remote-column indices");
  rem.val = ctx->dev_alloc<T>(std::max<size_t>(n_rem, 1), "remote-column values");
  launch_csr_split<T>(*op, own, rem, s);
  LL_HIP(hipStreamSynchronize(s));
  op->csr_own = std::move(own);
  op->csr_rem = std::move(rem);
}

// Drop the SpMV images that are NOT selected (LL_SPMV_KEEP_BOTH=1 keeps both for A/B timing).  CSR-stream needs the CSR image;
// the other kernels need none of it (the caller's borrowed arrays are just forgotten).
void release_unselected_image(ll_operator* op) {
  if (op->ctx->tune.keep_both) return;
  const int keep = op->spmv_kind;
  if (keep != LL_SPMV_CSR_STREAM) op->csr = CsrImage();
  if (keep != LL_SPMV_PB) op->pb = PbImage();
  if (keep != LL_SPMV_TILED) op->tl = TiledImage();
  if (keep != LL_SPMV_SYM) op->sym = SymImage();
}

// Creation-time timing of the operator's SpMV kernels (autotune, PB placement search): a zeroed x over every rank's padded
// shard, a y of the local rows, and min_ms(launch) = three launches behind events, the first a warm-up, the fastest of the
// other two in ms.
template <typename T> struct SpmvTimer {
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  hipStream_t s;
  DevArray<T> x, y;
  SpmvTimer(const ll_operator* op, const std::string& what) : s(op->ctx->stream) {
    ll_context* ctx = op->ctx;
    const size_t xn = (size_t)std::max<int64_t>(op->n, op->n_shard * std::max(1, ctx->nranks));
    x = ctx->dev_alloc<T>(xn, (what + " x").c_str());
    y = ctx->dev_alloc<T>((size_t)std::max<int64_t>(op->n_local, 1), (what + " y").c_str());
    LL_HIP(hipMemsetAsync(x.get(), 0, xn * sizeof(T), s));
    LL_HIP(hipEventCreate(&ev.e0));
    LL_HIP(hipEventCreate(&ev.e1));
  }
  template <typename F> double min_ms(F&& launch) {
    double best = 1e30;
    for (int rep = 0; rep < 3; ++rep) {
      LL_HIP(hipEventRecord(ev.e0, s));
      launch();
      LL_HIP(hipEventRecord(ev.e1, s));
      LL_HIP(hipEventSynchronize(ev.e1));
      float ms = 0.f;
      LL_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
      if (rep > 0) best = std::min(best, (double)ms);
    }
    return best;
  }
};

// Placement of the PB image.  The same image at another address runs up to 5-8 % faster or slower (round 2: "position
// noise"; round 3, bench.py spmv.ms_by_kernel: 0.922 ms for the operator created first, 0.845 ms for one created later, same
// process, same x / y) — which HBM stacks and channels the arena's physical pages land on is the draw of the allocation,
// fixed for its life.  So the draw is repeated: the image is copied (device to device, ~1 ms per GB) into fresh
// allocations, each is timed with the real kernels, the fastest is kept and the others are freed.  Purely local: no
// collective decision depends on it.  Returns the best time (ms).
template <typename T> double tune_pb_placement(ll_operator* op) {
  ll_context* ctx = op->ctx;
  hipStream_t s = ctx->stream;
  PbImage& pb = op->pb;
  if (!pb.present() || op->nnz < ((int64_t)1 << 22)) return -1.0;
  SpmvTimer<T> timer(op, "placement timing");
  T* const x = timer.x.get();
  auto time_pb = [&]() {
    return timer.min_ms([&] { launch_spmv_pb<T>(*op, x, x + op->row_begin, x + op->row_begin, timer.y.get(), 0.0, nullptr, s); });
  };
  // Every candidate stays allocated until all have been timed (an allocation freed at once would simply be handed out
  // again for the next one); then all but the fastest are freed.  cand[0] is the arena the image was built in.
  std::vector<DevArray<void>> cand;
  cand.push_back(std::move(pb.arena));
  size_t best_i = 0;
  std::vector<size_t> losers;  // in the order they lost
  double best = time_pb();
  if (ctx->tune.pb_placement_trace) std::fprintf(stderr, "[ll placement] draw 0 at %p: %.4f ms\n", cand[0].get(), best);
  // The candidates that lose are not returned to the device: sized like a Krylov-basis slab of a default run on this operator
  // (when that is at least the arena's size), they go into the context's slab cache and become the first basis slabs.  A process
  // that starts on a GPU another process has just left pays ~120 ms per fresh 4 GiB hipMalloc: config 3's
  // first run() to convergence needs seven slabs — the search has already paid for seven allocations.
  const size_t slab_hint = (size_t)default_slab_bytes(op->n, op->n_local, op->n_shard, op->elem_bytes, ctx->tune);
  const size_t cand_bytes = slab_hint >= pb.arena_bytes && slab_hint <= 2 * pb.arena_bytes ? slab_hint : pb.arena_bytes;
  // The image goes back to the best arena found so far — also when a copy or launch throws (LL_HIP) — and the other copies
  // are freed, or, after a completed search, cached.
  auto settle = [&](bool finished) {
    pb.rebase(cand[best_i].get());
    pb.arena = std::move(cand[best_i]);
    for (size_t i : losers) {
      // (at most eight slabs of that size are kept this way: a context on which many operators are created must not pile up
      // a placement search's worth of HBM per operator)
      size_t same = 0;
      for (auto& c : ctx->slab_cache) same += c.second == cand_bytes;
      if (finished && i != 0 && cand_bytes == slab_hint && same < 8) ctx->cache_put(cand[i].release(), cand_bytes);
    }
    cand.clear();  // frees the others
  };
  try {
    // candidates come from the context's allocator: under memory pressure it releases the cached Krylov slabs once before
    // giving up, so a large matrix is not silently left with fewer draws
    for (int t = 1; t < ctx->tune.pb_placements; ++t) {
      try {
        cand.push_back(ctx->dev_alloc<void>(cand_bytes, "PB placement candidate"));
      } catch (const Failure&) {  // no room for another copy: decide among what we have
        (void)hipGetLastError();
        break;
      }
      LL_HIP(hipMemcpyAsync(cand.back().get(), cand[best_i].get(), pb.arena_static_bytes, hipMemcpyDeviceToDevice, s));
      pb.rebase(cand.back().get());
      const double ms = time_pb();
      if (ctx->tune.pb_placement_trace)
        std::fprintf(stderr, "[ll placement] draw %d at %p: %.4f ms (best so far %.4f)\n", t, cand.back().get(), ms, best);
      if (ms < best) {
        best = ms;
        losers.push_back(best_i);  // the previous best becomes a loser
        best_i = cand.size() - 1;
      } else {
        losers.push_back(cand.size() - 1);
      }
      pb.rebase(cand[best_i].get());
    }
  } catch (...) {
    settle(false);
    throw;
  }
  settle(true);
  return best;
}

// Time both SpMV kernels on the device with the actual matrix and keep the faster one.  Sharded contexts decide on
// the SUM of the per-rank times, so every rank runs the same kernel (the exchange plan depends on it).  A kernel
// whose launch fails is simply not a candidate.
template <typename T> void autotune_spmv(ll_operator* op) {
  ll_context* ctx = op->ctx;
  hipStream_t s = ctx->stream;
  SpmvTimer<T> timer(op, "autotune");
  T* const x = timer.x.get();
  T* const y = timer.y.get();
  const DevArray<double> t = ctx->dev_alloc<double>(3, "autotune scalars");
  double t_kind[3] = {1e30, 1e30, 1e30};
  for (int kind : {LL_SPMV_CSR_STREAM, LL_SPMV_PB, LL_SPMV_TILED}) {
    if (kind == LL_SPMV_PB && !op->pb.present()) continue;     // image not built: not a candidate
    if (kind == LL_SPMV_TILED && !op->tl.present()) continue;
    try {
      t_kind[kind] = timer.min_ms([&] {
        if (kind == LL_SPMV_PB) launch_spmv_pb<T>(*op, x, x + op->row_begin, x + op->row_begin, y, 0.0, nullptr, s);
        else if (kind == LL_SPMV_TILED) launch_spmv_tiled<T>(*op, x, y, 0.0, nullptr, s);
        else launch_spmv<T>(*op, x, x + op->row_begin, y, 0.0, nullptr, s);
      });
    } catch (const Failure&) {  // e.g. a launch the device refuses: not a candidate, and not an error of the operator
      (void)hipGetLastError();
      t_kind[kind] = 1e30;
    }
  }
  for (int k = 0; k < 3; ++k) op->tune_ms[k] = t_kind[k] < 1e29 ? (float)t_kind[k] : -1.f;
  if (ctx->comm != nullptr) {
    LL_HIP(hipMemcpyAsync(t.get(), t_kind, 3 * sizeof(double), hipMemcpyHostToDevice, s));
    comm_allreduce_sum(ctx->comm, t.get(), 3, s);
    LL_HIP(hipMemcpyAsync(t_kind, t.get(), 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    LL_HIP(hipStreamSynchronize(s));
  }
  op->spmv_kind = LL_SPMV_CSR_STREAM;
  if (t_kind[LL_SPMV_PB] < t_kind[op->spmv_kind]) op->spmv_kind = LL_SPMV_PB;
  if (t_kind[LL_SPMV_TILED] < t_kind[op->spmv_kind]) op->spmv_kind = LL_SPMV_TILED;
}

// Sharded contexts take every image decision COLLECTIVELY (an empty shard, or a shard whose shape rules the image out, must
// not leave the ranks with different kernels: the exchange plan and the collectives issued depend on it): true when every
// rank says true.
bool all_ranks_agree(ll_context* ctx, bool mine) {
  if (ctx->comm == nullptr) return mine;
  const DevArray<double> d = ctx->dev_alloc<double>(1, "agreement flag");
  const double v = mine ? 0.0 : 1.0;
  double sum = 0.0;
  LL_HIP(hipMemcpyAsync(d.get(), &v, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  comm_allreduce_sum(ctx->comm, d.get(), 1, ctx->stream);
  LL_HIP(hipMemcpyAsync(&sum, d.get(), sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LL_HIP(hipStreamSynchronize(ctx->stream));
  return sum == 0.0;
}

// One optional image (PB or tiled): build it, and settle whether the operator has it.  A build that fails means "not built"
// where the operator stays usable without the image: on one GPU when it ran out of memory under auto selection (a matrix
// that fits as CSR alone keeps CSR-stream; asked for by name, the failure is the caller's), on a sharded context whatever
// the failure, so that every rank reaches the agreement below instead of leaving its peers waiting in it.  Any other
// failure propagates.  An image that some rank could not build is dropped by the ranks that have it.
template <typename Image, typename Build> bool build_optional_image(ll_context* ctx, bool auto_select, Image& im, Build&& build) {
  bool built = false;
  try {
    built = build();
  } catch (const Failure& f) {
    if (ctx->comm == nullptr && !(f.code == LL_ERR_ALLOC && auto_select)) throw;
    (void)hipGetLastError();
  }
  const bool ok = all_ranks_agree(ctx, built);
  if (built && !ok) im = Image();
  return ok;
}

// The header of every operator: kind, storage type, context and row range.  Sharded operators must use the ll_partition()
// row ranges (equal shard strides); a single-GPU operator is whole.
template <typename T>
std::unique_ptr<ll_operator> new_operator(ll_context* ctx, ll_operator::Kind kind, int64_t n, int64_t row_begin, int64_t n_local) {
  std::unique_ptr<ll_operator> op(new ll_operator);
  op->kind = kind;
  op->is_complex = scalar_traits<T>::is_complex;
  op->elem_bytes = (int)sizeof(T);
  op->ctx = ctx;
  op->n = n;
  op->n_local = n_local;
  op->row_begin = row_begin;
  if (ctx->nranks > 1) {
    op->n_shard = (n + ctx->nranks - 1) / ctx->nranks;
    LL_REQUIRE(row_begin == std::min<int64_t>(n, op->n_shard * ctx->rank) &&
                   n_local == std::min<int64_t>(n, op->n_shard * (ctx->rank + 1)) - row_begin,
               "sharded operators must use the ll_partition() row ranges");
  } else {
    op->n_shard = n;
    LL_REQUIRE(row_begin == 0 && n_local == n, "a single-GPU context needs the whole operator (row_begin 0, n_local == n)");
  }
  return op;
}

// The caller's ll_csr_options: a known accuracy class and a kernel up to max_kernel (LL_SPMV_TILED for full storage,
// LL_SPMV_SYM for one triangle)
void check_options(const ll_csr_options& o, int max_kernel) {
  LL_REQUIRE(o.accuracy >= LL_ACCURACY_DEFAULT && o.accuracy <= LL_ACCURACY_COMPONENTWISE, "ll_csr_options.accuracy");
  LL_REQUIRE(o.kernel >= -1 && o.kernel <= max_kernel, "ll_csr_options.kernel");
}

// The caller's row offsets on the host (device arrays are copied down into `copy`), checked: 0 first, never decreasing.
const int64_t* host_row_ptr(const int64_t* rp, int64_t nr, bool on_device, std::vector<int64_t>& copy) {
  if (on_device) {
    copy.resize((size_t)nr + 1);
    LL_HIP(hipMemcpy(copy.data(), rp, copy.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    rp = copy.data();
  }
  LL_REQUIRE(rp[0] == 0, "row_ptr must start at 0");
  for (int64_t i = 0; i < nr; ++i) LL_REQUIRE(rp[i + 1] >= rp[i], "row_ptr must be non-decreasing");
  return rp;
}

// ---------------------------------------------------------------- accuracy policy
// The form of every image for an accuracy request (LL_ACCURACY_*) and the form LL_PB_PHASE2 names (Tuning::pb_phase2, or the
// form a PB image has now).  Norm-wise: the fixed-point sums of every image.  Component-wise: floating-point sums — PB
// phase 2 wave-ordered, or in arrival order where LL_PB_PHASE2=atomic; the tiled kernel's waves in turn; no one-triangle
// kernel.  LL_ACCURACY_DEFAULT: the form LL_PB_PHASE2 names decides the class.
struct ImageForms {
  int pb_phase2;     // LL_PB_FIXED / _ORDERED / _ATOMIC
  bool tl_ordered;   // TiledImage::ordered
  bool sym_allowed;  // the one-triangle kernel sums in fixed point only
};
ImageForms image_forms(int accuracy, int pb_phase2) {
  const int phase2 = accuracy == LL_ACCURACY_COMPONENTWISE ? (pb_phase2 == LL_PB_ATOMIC ? LL_PB_ATOMIC : LL_PB_ORDERED)
                     : accuracy == LL_ACCURACY_NORMWISE    ? LL_PB_FIXED
                                                           : pb_phase2;
  const bool componentwise = phase2 != LL_PB_FIXED;
  return {phase2, componentwise, !componentwise};
}

}  // namespace

void set_op_accuracy(ll_operator* op, int accuracy) {
  LL_REQUIRE(op != nullptr && op->kind == ll_operator::CSR, "not a CSR operator");
  LL_REQUIRE(accuracy == LL_ACCURACY_NORMWISE || accuracy == LL_ACCURACY_COMPONENTWISE,
             "accuracy must be LL_ACCURACY_NORMWISE or LL_ACCURACY_COMPONENTWISE");
  // (a PB image's own form stands for the environment's: an atomic image stays atomic, a fixed one becomes ordered)
  const ImageForms f = image_forms(accuracy, op->pb.phase2);
  LL_REQUIRE(f.sym_allowed || op->spmv_kind != LL_SPMV_SYM,
             "the one-triangle kernel sums in fixed point only (norm-wise class): it has no component-wise form");
  if (op->tl.present()) op->tl.ordered = f.tl_ordered;  // the tiled image serves both classes
  if (!op->pb.present()) return;  // no PB image: CSR-stream is component-wise whatever is asked, the tiled kernel was set above
  LL_REQUIRE(f.pb_phase2 != LL_PB_FIXED || (op->pb.rexp && op->pb.blockmax),
             "this image was built without the row exponents of the fixed-point sums (row block too large for them)");
  op->pb.phase2 = f.pb_phase2;
}

int op_accuracy(const ll_operator* op) {
  const bool fixed = op->kind == ll_operator::CSR && ((op->spmv_kind == LL_SPMV_PB && op->pb.phase2 == LL_PB_FIXED) ||
                                                      (op->spmv_kind == LL_SPMV_TILED && !op->tl.ordered) ||
                                                      op->spmv_kind == LL_SPMV_SYM);
  return fixed ? LL_ACCURACY_NORMWISE : LL_ACCURACY_COMPONENTWISE;
}

// ---------------------------------------------------------------- creation
ll_csr_options csr_options_default(bool arrays_on_device) {
  ll_csr_options o;
  (void)ll_csr_options_default(&o);
  o.arrays_on_device = arrays_on_device ? 1 : 0;
  return o;
}

template <typename T>
void create_csr(ll_context* ctx, int64_t nr, int64_t nc, int64_t row_begin, const int64_t* rp, const int32_t* ci, const void* va,
                const ll_csr_options& opt, ll_operator** out) {
  use(ctx);
  check_options(opt, LL_SPMV_TILED);
  LL_REQUIRE(out && rp && (ci || nr == 0) && (va || nr == 0), "null argument");
  LL_REQUIRE(nr >= 0 && nc >= 1 && row_begin >= 0 && row_begin + nr <= nc, "bad shape");
  LL_REQUIRE(nr < (int64_t)0x7fffffff && nc < (int64_t)0x7fffffff, "dimension exceeds int32 indices");
  const bool on_device = opt.arrays_on_device != 0;
  std::vector<int64_t> rp_copy;
  const int64_t* rp_host = host_row_ptr(rp, nr, on_device, rp_copy);
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::CSR, nc, row_begin, nr);
  op->nnz = rp_host[nr];
  const size_t nnz = (size_t)op->nnz;
  if (on_device) {  // the caller's arrays: borrowed, never freed
    op->csr.col = DevArray<int32_t>::borrow(const_cast<int32_t*>(ci));
    op->csr.val = DevArray<void>::borrow(const_cast<void*>(va));
  } else {
    op->csr.col = ctx->dev_alloc<int32_t>(std::max<size_t>(nnz, 1), "CSR column indices");
    op->csr.val = ctx->dev_alloc<T>(std::max<size_t>(nnz, 1), "CSR values");
    LL_HIP(hipMemcpy(op->csr.col.get(), ci, nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    LL_HIP(hipMemcpy(op->csr.val.get(), va, nnz * sizeof(T), hipMemcpyHostToDevice));
  }
  // 64-bit row offsets once nnz exceeds int32 (LL_FORCE_RP64=1: exercise that kernel variant on small test matrices)
  op->csr.rp64 = op->nnz > (int64_t)0x7fffffff || ctx->tune.force_rp64;
  upload_csr_index<T>(ctx, op->csr, rp_host, nr, "row offsets", "SpMV tiles");
  // column range check and max absolute row sum (ll_op_inf_norm; determine_eigenvalue_offset.cpp:12-29), on the device
  // for host and device inputs alike, whatever kernel gets selected
  csr_check_device<T>(op.get());
  op->spmv_kind = LL_SPMV_CSR_STREAM;
  // LL_SPMV_* asked for, or -1: time the candidates; the caller's ll_csr_options.kernel outranks LL_SPMV_KERNEL
  const int kernel = opt.kernel >= 0 ? opt.kernel : ctx->tune.spmv_kernel;
  const bool auto_select = kernel < 0;
  const ImageForms forms = image_forms(opt.accuracy, ctx->tune.pb_phase2);
  // (sharded contexts: an empty shard takes part in the collective decisions all the same)
  const bool can_build = nnz > 0 || ctx->comm != nullptr;
  bool pb_ok = false, tl_ok = false;
  if ((auto_select || kernel == LL_SPMV_PB) && can_build)
    // The propagation-blocked image is built on the device from the CSR arrays (histogram + scatter kernels).  It is the
    // matrix again plus a product buffer (peak at creation: CSR + PB + timing scratch, about 2.3 x the matrix).
    pb_ok = build_optional_image(ctx, auto_select, op->pb, [&] { return pb_build_device<T>(op.get(), forms.pb_phase2); });
  if ((auto_select || kernel == LL_SPMV_TILED) && can_build) {
    // the 2-D tiled image: only for matrices whose row blocks touch few column tiles (tl_build_device decides).  One image serves
    // both accuracy classes: fixed-point sums (norm-wise) or the waves adding in turn in floating point (component-wise).
    tl_ok = build_optional_image(ctx, auto_select, op->tl, [&] { return nnz > 0 && tl_build_device<T>(op.get()); });
    op->tl.ordered = forms.tl_ordered;
  }
  // Asked for by name, the tiled kernel is an error where no tiled image exists — never a silent fallback, and never a kernel
  // selected without its image (launch_spmv_tiled would write nothing).
  LL_REQUIRE(kernel != LL_SPMV_TILED || tl_ok,
             can_build ? "this matrix is not eligible for the tiled SpMV kernel (its row blocks touch too many column tiles)"
                       : "the tiled SpMV kernel was asked for by name but no tiled image was built (matrix without entries)");
  if (kernel == LL_SPMV_PB && pb_ok) op->spmv_kind = LL_SPMV_PB;
  else if (kernel == LL_SPMV_TILED) op->spmv_kind = LL_SPMV_TILED;
  else if (auto_select && (pb_ok || tl_ok)) autotune_spmv<T>(op.get());
  if (op->spmv_kind == LL_SPMV_PB && ctx->tune.pb_placements > 1) {
    const double ms = tune_pb_placement<T>(op.get());
    if (ms > 0.0 && op->tune_ms[LL_SPMV_PB] >= 0.f) op->tune_ms[LL_SPMV_PB] = (float)ms;
  }
  release_unselected_image(op.get());
  // (every rank takes this branch or none: the kernel choice above is collective, the switch comes from the environment)
  if (ctx->nranks > 1 && ctx->tune.csr_split && op->csr.row_ptr) {
    // The split image is a second copy of the matrix.  When it does not fit next to the original (a shard that already fell
    // back to CSR-stream because the PB image did not fit), the operator stays usable in the gather-then-multiply form — safe
    // per rank: split and unsplit ranks issue the same single all-gather.
    try {
      build_csr_split<T>(op.get());
    } catch (const Failure& f) {
      if (f.code != LL_ERR_ALLOC) throw;
      (void)hipGetLastError();
    }
    // Once split, the unsplit arrays are never read again on this context: return them (steady-state footprint 1 x the matrix)
    // unless LL_SPMV_KEEP_BOTH=1 asked for every image to stay.  The row offsets stay (4 bytes per row): they mark the operator
    // as one that still has a CSR-stream image.
    if (op->csr_split() && !ctx->tune.keep_both && op->spmv_kind == LL_SPMV_CSR_STREAM) {
      op->csr.col.reset();
      op->csr.val.reset();
      op->csr.tiles.reset();
      op->csr.ntiles = 0;
    }
  }
  *out = op.release();
}

// {row, col, value} triplets (sample2_sparse.cpp:14-47) -> CSR, stable in input order inside a row (duplicates kept).
template <typename T>
void create_coo(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols, const void* vals,
                ll_operator** out) {
  LL_REQUIRE(n >= 1 && nnz >= 0 && (nnz == 0 || (rows && cols && vals)), "bad argument");
  std::vector<int64_t> rp((size_t)n + 1, 0);
  for (int64_t p = 0; p < nnz; ++p) {
    LL_REQUIRE(rows[p] >= 0 && rows[p] < n, "row index out of range");
    ++rp[(size_t)rows[p] + 1];
  }
  for (int64_t i = 0; i < n; ++i) rp[(size_t)i + 1] += rp[(size_t)i];
  std::vector<int64_t> cur(rp.begin(), rp.end() - 1);
  std::vector<int32_t> ci((size_t)std::max<int64_t>(nnz, 1));
  std::vector<T> va((size_t)std::max<int64_t>(nnz, 1));
  const T* v = (const T*)vals;
  for (int64_t p = 0; p < nnz; ++p) {
    const int64_t q = cur[(size_t)rows[p]]++;
    ci[(size_t)q] = cols[p];
    va[(size_t)q] = v[p];
  }
  create_csr<T>(ctx, n, n, 0, rp.data(), ci.data(), va.data(), csr_options_default(false), out);
}

// One stored triangle -> the operator.  Every row of A is taken in the order of the expansion a caller would build (upper:
// the mirrored entries of the rows above, by row, then the row's own; lower: the row's own, then the mirrored entries of the
// rows below, by row) — increasing column order when the triangle's rows are sorted by column.  The row exponents of the
// fixed-point grid and the infinity norm are summed in that order.  The one-triangle image is built from the triangle alone
// (nothing but the image reaches the device); any other choice expands the matrix on the host and goes through create_csr.
template <typename T>
void create_csr_sym(ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const void* va,
                    const ll_csr_options* opt, ll_operator** out) {
  use(ctx);
  LL_REQUIRE(out != nullptr && rp != nullptr, "null argument");
  LL_REQUIRE(ctx->nranks <= 1 && ctx->comm == nullptr,
             "a matrix stored as one triangle cannot be created on a sharded context (a rank's rows of the triangle do not hold "
             "its rows of the matrix): create the full matrix there");
  LL_REQUIRE(uplo == LL_UPPER || uplo == LL_LOWER, "uplo must name the upper (0) or the lower (1) triangle");
  LL_REQUIRE(n >= 1 && n < (int64_t)0x7fffffff, "bad shape");
  const ll_csr_options o = opt != nullptr ? *opt : csr_options_default(false);
  check_options(o, LL_SPMV_SYM);
  const bool on_device = o.arrays_on_device != 0;
  // the triangle on the host
  std::vector<int64_t> rp_copy;
  const int64_t* rp_h = host_row_ptr(rp, n, on_device, rp_copy);
  const int64_t nnz = rp_h[n];
  LL_REQUIRE(nnz == 0 || (ci != nullptr && va != nullptr), "null argument");
  std::vector<int32_t> ci_copy;
  std::vector<T> va_copy;
  const int32_t* ci_h = ci;
  const T* va_h = (const T*)va;
  if (on_device && nnz > 0) {
    ci_copy.resize((size_t)nnz);
    va_copy.resize((size_t)nnz);
    LL_HIP(hipMemcpy(ci_copy.data(), ci, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    LL_HIP(hipMemcpy(va_copy.data(), va, (size_t)nnz * sizeof(T), hipMemcpyDeviceToHost));
    ci_h = ci_copy.data();
    va_h = va_copy.data();
  }
  // checks, entries per column outside the diagonal
  std::vector<int64_t> mirrored((size_t)n, 0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t p = rp_h[i]; p < rp_h[i + 1]; ++p) {
      const int64_t j = ci_h[p];
      LL_REQUIRE(j >= 0 && j < n, "column index out of range");
      LL_REQUIRE(uplo == LL_UPPER ? j >= i : j <= i,
                 uplo == LL_UPPER ? "an entry lies below the diagonal of an upper triangle"
                                  : "an entry lies above the diagonal of a lower triangle");
      if (j != i) ++mirrored[(size_t)j];
    }
  // which kernel
  const ImageForms forms = image_forms(o.accuracy, ctx->tune.pb_phase2);
  const int64_t win_halo = sym_halo_for(rp_h, ci_h, n);  // (entries beyond it are read with x from memory)
  const int rb_rows = win_halo >= 0 ? sym_rows_for<T>(n, win_halo) : 0;
  if (o.kernel == LL_SPMV_SYM) {
    LL_REQUIRE(forms.sym_allowed, "the one-triangle kernel sums in fixed point only (norm-wise class): it has no component-wise form");
    LL_REQUIRE(nnz > 0, "the one-triangle kernel was asked for by name but the triangle has no entries");
    LL_REQUIRE(rb_rows > 0, "this triangle is not eligible for the one-triangle kernel (its half-bandwidth exceeds the row block "
                            "whose x window fits the LDS)");
  }
  const bool use_sym = o.kernel == LL_SPMV_SYM || (o.kernel == -1 && forms.sym_allowed && nnz > 0 && rb_rows > 0);
  if (use_sym) {
    // The expanded matrix is never built.  Its row sums are taken in one sweep over the triangle's rows in increasing order:
    // every row's mirrored entries then arrive by source row, before (upper) or after (lower) its own entries — the order of
    // the expanded rows above, in which the full-storage kernels sum them (pb_rowexp_kernel, csr_check_kernel; the same IEEE
    // operations, so the same bits).
    std::vector<double> s1((size_t)n, 0.0), s2((size_t)n, 0.0);  // sum |re| + |im| (row exponents), sum of moduli (inf norm)
    int64_t fnnz = 0;
    for (int64_t i = 0; i < n; ++i)
      for (int64_t p = rp_h[i]; p < rp_h[i + 1]; ++p) {
        const int64_t j = ci_h[p];
        const double a1 = abs1_host(va_h[p]), a2 = std::sqrt(abs2_fma_host(va_h[p]));
        s1[(size_t)i] += a1;
        s2[(size_t)i] += a2;
        ++fnnz;
        if (j != i) {
          s1[(size_t)j] += a1;
          s2[(size_t)j] += a2;
          ++fnnz;
        }
      }
    std::vector<int16_t> rexp((size_t)n);
    double mx = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      const double v = s1[(size_t)i];
      int e = -1100;
      if (v > 0.0 && std::isfinite(v)) (void)std::frexp(v, &e);
      else if (!(v == 0.0)) e = 32767;
      rexp[(size_t)i] = (int16_t)e;
      mx = std::fmax(mx, s2[(size_t)i]);
    }
    std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::CSR, n, 0, n);
    op->nnz = fnnz;
    op->inf_norm = mx;
    op->sym_stored = nnz;
    SymImage im;
    im.halo = (int)win_halo;
    im.rb_rows = rb_rows;
    sym_build<T>(*op, im, rp_h, ci_h, va_h);
    LL_HIP(hipMemcpy(im.rexp.get(), rexp.data(), rexp.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    op->sym = std::move(im);
    op->spmv_kind = LL_SPMV_SYM;
    *out = op.release();
    return;
  }
  // the expansion (stable: rows are visited in increasing order, so every row's mirrored entries arrive by source row)
  std::vector<int64_t> frp((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) frp[(size_t)i + 1] = frp[(size_t)i] + (rp_h[i + 1] - rp_h[i]) + mirrored[(size_t)i];
  const int64_t fnnz = frp[(size_t)n];
  std::vector<int32_t> fci((size_t)std::max<int64_t>(fnnz, 1));
  std::vector<T> fva((size_t)std::max<int64_t>(fnnz, 1));
  std::vector<int64_t> mcur((size_t)n);
  for (int64_t i = 0; i < n; ++i) mcur[(size_t)i] = uplo == LL_UPPER ? frp[(size_t)i] : frp[(size_t)i] + (rp_h[i + 1] - rp_h[i]);
  for (int64_t i = 0; i < n; ++i) {
    int64_t d = uplo == LL_UPPER ? frp[(size_t)i] + mirrored[(size_t)i] : frp[(size_t)i];
    for (int64_t p = rp_h[i]; p < rp_h[i + 1]; ++p) {
      const int32_t j = ci_h[p];
      fci[(size_t)d] = j;
      fva[(size_t)d++] = va_h[p];
      if (j != i) {
        const int64_t q = mcur[(size_t)j]++;
        fci[(size_t)q] = (int32_t)i;
        if constexpr (scalar_traits<T>::is_complex) fva[(size_t)q] = T{va_h[p].re, -va_h[p].im};
        else fva[(size_t)q] = va_h[p];
      }
    }
  }
  // (the caller's copies, if any, are released with this scope, after their last reader)
  ll_csr_options fo = o;
  fo.arrays_on_device = 0;
  ll_operator* raw = nullptr;
  create_csr<T>(ctx, n, n, 0, frp.data(), fci.data(), fva.data(), fo, &raw);
  raw->sym_stored = nnz;
  *out = raw;
}

template <typename T>
void create_dense(ll_context* ctx, int64_t nr, int64_t nc, int64_t row_begin, const void* a, ll_operator** out) {
  use(ctx);
  LL_REQUIRE(out && (a || nr == 0), "null argument");
  LL_REQUIRE(nr >= 0 && nc >= 1 && row_begin >= 0 && row_begin + nr <= nc, "bad shape");
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::DENSE, nc, row_begin, nr);
  op->nnz = nr * nc;
  const T* v = (const T*)a;
  double mx = 0.0;
  for (int64_t i = 0; i < nr; ++i) {
    double rs = 0.0;
    for (int64_t j = 0; j < nc; ++j) rs += std::sqrt(abs2_host(v[i * nc + j]));
    mx = std::max(mx, rs);
  }
  op->inf_norm = mx;
  const size_t bytes = (size_t)nr * (size_t)nc * sizeof(T);
  op->dense = ctx->dev_alloc<void>(std::max<size_t>(bytes, 16), "dense matrix");
  if (bytes) LL_HIP(hipMemcpy(op->dense.get(), a, bytes, hipMemcpyHostToDevice));
  *out = op.release();
}

template <typename T>
void create_stencil(ll_context* ctx, const ll_stencil_desc* d, int64_t row_begin, int64_t n_local, const double* onsite,
                    ll_operator** out) {
  use(ctx);
  LL_REQUIRE(out && d, "null argument");
  LL_REQUIRE(d->ndim >= 1 && d->ndim <= 3, "ndim must be 1, 2 or 3");
  int64_t n = 1;
  for (int k = 0; k < d->ndim; ++k) {
    LL_REQUIRE(d->dims[k] >= 1, "lattice dimensions must be positive");
    LL_REQUIRE(n <= ((int64_t)1 << 40) / d->dims[k], "lattice too large");
    n *= d->dims[k];
    if (!scalar_traits<T>::is_complex) {
      LL_REQUIRE(d->hop_im[k] == 0.0, "complex hopping needs a complex storage type");
      for (int e = 0; e < 3; ++e) LL_REQUIRE(d->phase_grad[k][e] == 0.0, "Peierls phases need a complex storage type");
    }
  }
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::STENCIL, n, row_begin, n_local);
  LL_REQUIRE(n_local < (int64_t)0x7fffffff, "shard exceeds 32-bit local indices");
  op->st = *d;
  int64_t stride = 1;
  for (int k = d->ndim - 1; k >= 0; --k) {
    op->st_stride[k] = stride;
    stride *= d->dims[k];
  }
  op->st_halo = op->st_stride[0];
  if (ctx->nranks > 1) {
    const int64_t last = n - op->n_shard * (ctx->nranks - 1);  // the shortest shard
    LL_REQUIRE(last >= op->st_halo && op->n_shard >= op->st_halo,
               "lattice operator: every shard must hold at least one hyperplane (n / dims[0] sites); use fewer ranks");
  }
  op->nnz = 0;
  double hops = 0.0;
  for (int k = 0; k < d->ndim; ++k) hops += 2.0 * std::hypot(d->hop_re[k], d->hop_im[k]);
  double diag_max = std::abs(d->diag);
  if (onsite) {
    diag_max = 0.0;
    for (int64_t i = 0; i < n_local; ++i) diag_max = std::max(diag_max, std::abs(d->diag + onsite[i]));
    typedef typename scalar_traits<T>::real R;
    std::vector<R> tmp((size_t)n_local);
    for (int64_t i = 0; i < n_local; ++i) tmp[(size_t)i] = (R)onsite[i];
    op->onsite = ctx->dev_alloc<void>(std::max<size_t>((size_t)n_local * sizeof(R), 16), "on-site terms");
    LL_HIP(hipMemcpy(op->onsite.get(), tmp.data(), (size_t)n_local * sizeof(R), hipMemcpyHostToDevice));
  }
  op->inf_norm = diag_max + hops;  // an upper bound of the max absolute row sum (equal to it for interior sites)
  *out = op.release();
}

// Sum of Pauli strings (pauli.hip, pauli_sector.hip): validate, fold i^nY into the coefficient (a sign for the real types, one
// of {1, i, -1, -i} for the complex ones), group the terms by x mask — groups by ascending mask, the terms of a group in the
// caller's order.
namespace {
struct PauliTables {
  std::vector<uint32_t> gx, tz;   // x mask per group, z mask per term
  std::vector<int32_t> gptr;      // [groups + 1] first term of each group
  std::vector<double> tc;         // per term: c i^nY (real types), (re, im) of it (complex types)
  double norm = 0.0;              // sum_t |c_t|
};
template <typename T>
PauliTables pauli_tables(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  use(ctx);
  LL_REQUIRE(out != nullptr, "null argument (out)");
  LL_REQUIRE(n_terms >= 0, "n_terms is negative");
  LL_REQUIRE(terms != nullptr || n_terms == 0, "null argument (terms)");
  LL_REQUIRE(n_sites >= 1 && n_sites <= kPauliMaxSites,
             "n_sites must lie in [1, " + std::to_string(kPauliMaxSites) + "] (2^n_sites states, 32-bit local indices)");
  LL_REQUIRE(ctx->nranks == 1,
             "a sum of Pauli strings cannot be created on a sharded context (flips of the sites that would number the ranks are "
             "exchanges between them, which are not built): use a single-GPU context");
  LL_REQUIRE(n_terms < (int64_t)0x7fffffff, "too many terms");
  constexpr bool cplx = scalar_traits<T>::is_complex;
  const uint64_t site_mask = ((uint64_t)1 << n_sites) - 1;
  std::vector<int64_t> order((size_t)n_terms);
  PauliTables pt;
  for (int64_t t = 0; t < n_terms; ++t) {
    const ll_pauli_term& q = terms[t];
    LL_REQUIRE(((q.x_mask | q.z_mask) & ~site_mask) == 0, "term " + std::to_string(t) + ": a mask bit at or above n_sites");
    LL_REQUIRE(std::isfinite(q.coef), "term " + std::to_string(t) + ": the coefficient is not finite");
    LL_REQUIRE(cplx || (__builtin_popcountll(q.x_mask & q.z_mask) & 1) == 0,
               "term " + std::to_string(t) + ": an odd number of Y factors makes the matrix complex; use a complex storage type");
    order[(size_t)t] = t;
    pt.norm += std::fabs(q.coef);
  }
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return terms[a].x_mask < terms[b].x_mask; });
  pt.tz.resize((size_t)n_terms);
  pt.tc.resize((size_t)n_terms * (cplx ? 2 : 1));
  for (int64_t k = 0; k < n_terms; ++k) {
    const ll_pauli_term& q = terms[order[(size_t)k]];
    if (pt.gx.empty() || pt.gx.back() != (uint32_t)q.x_mask) {
      pt.gx.push_back((uint32_t)q.x_mask);
      pt.gptr.push_back((int32_t)k);
    }
    pt.tz[(size_t)k] = (uint32_t)q.z_mask;
    const int ny = __builtin_popcountll(q.x_mask & q.z_mask) & 3;  // i^nY: 1, i, -1, -i
    const double c = ny >= 2 ? -q.coef : q.coef;
    if (cplx) {
      pt.tc[2 * (size_t)k] = (ny & 1) ? 0.0 : c;
      pt.tc[2 * (size_t)k + 1] = (ny & 1) ? c : 0.0;
    } else {
      pt.tc[(size_t)k] = c;
    }
  }
  pt.gptr.push_back((int32_t)n_terms);
  return pt;
}
// a host table on the device
template <typename V> void pauli_upload(ll_context* ctx, DevArray<V>& dst, const std::vector<V>& src, const char* what) {
  dst = ctx->dev_alloc<V>(std::max<size_t>(src.size(), 1), what);
  if (!src.empty()) LL_HIP(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
}
// the four term tables of an image on the device
void pauli_upload_tables(ll_context* ctx, PauliTermImage& im, const PauliTables& pt) {
  im.ngroups = (int)pt.gx.size();
  im.nterms = (int64_t)pt.tz.size();
  pauli_upload(ctx, im.gx, pt.gx, "Pauli x masks");
  pauli_upload(ctx, im.gptr, pt.gptr, "Pauli group offsets");
  pauli_upload(ctx, im.tz, pt.tz, "Pauli z masks");
  pauli_upload(ctx, im.tc, pt.tc, "Pauli coefficients");
}

// S_z conservation, group by group: over every assignment of the bits the group touches (its x mask and its z masks) for which
// flipping the x mask changes the number of set bits, the group's weight — summed as the kernel sums it, in double, terms in
// order — must be exactly 0.  R = doubles per coefficient (2: re, im, summed separately as the kernel does).
void pauli_require_sz_conserving(const PauliTables& pt, int R) {
  for (size_t g = 0; g < pt.gx.size(); ++g) {
    const uint32_t X = pt.gx[g];
    if (X == 0) continue;
    char hex[16];
    std::snprintf(hex, sizeof hex, "0x%x", (unsigned)X);
    const std::string who = "the terms with x mask " + std::string(hex);
    uint32_t U = X;
    for (int32_t k = pt.gptr[g]; k < pt.gptr[g + 1]; ++k) U |= pt.tz[(size_t)k];
    LL_REQUIRE(__builtin_popcount(U) <= kPauliSectorMaxSupport,
               who + " act on " + std::to_string(__builtin_popcount(U)) + " sites: the S_z conservation check cannot be made for more than " +
                   std::to_string(kPauliSectorMaxSupport) + " (it visits every assignment of them)");
    const int px = __builtin_popcount(X);
    uint32_t s = 0;
    do {  // every subset s of U
      if (2 * __builtin_popcount(s & X) != px) {
        for (int r = 0; r < R; ++r) {
          double w = 0.0;
          for (int32_t k = pt.gptr[g]; k < pt.gptr[g + 1]; ++k) {
            const double c = pt.tc[(size_t)k * R + r];
            w += (__builtin_popcount((s ^ X) & pt.tz[(size_t)k]) & 1) ? -c : c;
          }
          LL_REQUIRE(w == 0.0, who + " do not conserve S_z (they change the number of flipped spins with a weight that is not "
                                     "zero): a magnetisation sector needs an H that commutes with total S_z");
        }
      }
      s = (s - U) & U;
    } while (s != 0);
  }
}

// The states of the sector of n_down set bits in ascending order and the two tables that give a state's index back
// (ll_internal.hpp PauliSectorImage): one pass over the C(n_sites, n_down) states, on the host.
struct SectorTables {
  int h = 0;
  int64_t dim = 0;
  std::vector<uint32_t> states, lo_rank, hi_rank;
  uint32_t rank(uint32_t s) const { return lo_rank[s & (((uint32_t)1 << h) - 1)] + hi_rank[s >> h]; }
};
SectorTables sector_tables(int32_t n_sites, int32_t n_down) {
  // binom[p][k] = C(p, k), p <= n_sites <= 30: below 2^32
  std::vector<std::vector<uint64_t>> binom((size_t)n_sites + 1, std::vector<uint64_t>((size_t)n_sites + 2, 0));
  for (int p = 0; p <= n_sites; ++p) {
    binom[(size_t)p][0] = 1;
    for (int k = 1; k <= p; ++k) binom[(size_t)p][(size_t)k] = binom[(size_t)p - 1][(size_t)k - 1] + binom[(size_t)p - 1][(size_t)k];
  }
  SectorTables st;
  st.dim = (int64_t)binom[(size_t)n_sites][(size_t)n_down];
  const int h = st.h = (n_sites + 1) / 2, hb = n_sites - h;  // low / other bits: both tables at most 2^15 entries
  // rank(s) = sum_k C(p_k, k) over the set bits p_1 < p_2 < ...: the low bits count k from 1, the others from
  // n_down - popcount(others) + 1 (entries no state of the sector reaches stay 0)
  std::vector<uint32_t>& lo_rank = st.lo_rank;
  std::vector<uint32_t>& hi_rank = st.hi_rank;
  lo_rank.assign((size_t)1 << h, 0);
  hi_rank.assign((size_t)1 << hb, 0);
  for (uint32_t lo = 0; lo < ((uint32_t)1 << h); ++lo) {
    if (__builtin_popcount(lo) > n_down) continue;
    uint64_t r = 0;
    int k = 0;
    for (int p = 0; p < h; ++p)
      if (lo >> p & 1u) r += binom[(size_t)p][(size_t)++k];
    lo_rank[lo] = (uint32_t)r;
  }
  for (uint32_t hi = 0; hi < ((uint32_t)1 << hb); ++hi) {
    int k = n_down - __builtin_popcount(hi);
    if (k < 0 || k > h) continue;
    uint64_t r = 0;
    for (int p = 0; p < hb; ++p)
      if (hi >> p & 1u) r += binom[(size_t)(p + h)][(size_t)++k];
    hi_rank[hi] = (uint32_t)r;
  }
  const int64_t dim = st.dim;
  std::vector<uint32_t>& states = st.states;
  states.resize((size_t)dim);
  {
    uint64_t s = ((uint64_t)1 << n_down) - 1;  // the smallest state; the next one with as many set bits follows (Gosper)
    for (int64_t i = 0; i < dim; ++i) {
      states[(size_t)i] = (uint32_t)s;
      if (s == 0) break;
      const uint64_t c = s & (0 - s), r = s + c;
      s = (((r ^ s) >> 2) >> __builtin_ctzll(s)) | r;
    }
  }
  return st;
}
}  // namespace

template <typename T>
void create_pauli(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  const int64_t n = (int64_t)1 << n_sites;
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::PAULI, n, 0, n);
  op->nnz = n_terms;
  op->inf_norm = pt.norm;  // sum_t |c_t|: a bound of every absolute row sum
  PauliImage im;
  im.n_sites = n_sites;
  pauli_upload_tables(ctx, im.terms, pt);
  op->pauli = std::move(im);
  *out = op.release();
}

// The same terms on the sector of n_down set bits (pauli_sector.hip).  The states and the two rank tables are built here, on the
// host: one pass over the C(n_sites, n_down) states in ascending order.
template <typename T>
void create_pauli_sector(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                         ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(n_down >= 0 && n_down <= n_sites, "n_down must lie in [0, n_sites] (the number of flipped spins of the sector)");
  pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
  const SectorTables st = sector_tables(n_sites, n_down);
  const int64_t dim = st.dim;
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::PAULI_SECTOR, dim, 0, dim);
  op->nnz = n_terms;
  op->inf_norm = pt.norm;  // sum_t |c_t|: a bound of every absolute row sum
  PauliSectorImage im;
  im.n_sites = n_sites;
  im.n_down = n_down;
  im.h = st.h;
  im.dim = dim;
  pauli_upload_tables(ctx, im.terms, pt);
  pauli_upload(ctx, im.states, st.states, "S_z sector states");
  pauli_upload(ctx, im.lo_rank, st.lo_rank, "S_z sector rank table (low bits)");
  pauli_upload(ctx, im.hi_rank, st.hi_rank, "S_z sector rank table (high bits)");
  op->pauli_sector = std::move(im);
  *out = op.release();
}

namespace {
// Translation invariance on the ring: with the coefficients of equal (x_mask, z_mask) merged (summed in the caller's order),
// rotating every term's masks by one site must map the term set onto itself with exactly equal coefficients (a missing term
// counts as coefficient 0).  i^nY does not change under the rotation, so the caller's coefficients are compared.
void pauli_require_translation_invariant(int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms) {
  const uint64_t site_mask = ((uint64_t)1 << n_sites) - 1;
  auto rot = [&](uint64_t v) { return ((v << 1) | (v >> (n_sites - 1))) & site_mask; };
  std::map<std::pair<uint64_t, uint64_t>, double> merged;
  for (int64_t t = 0; t < n_terms; ++t) merged[{terms[t].x_mask, terms[t].z_mask}] += terms[t].coef;
  for (int64_t t = 0; t < n_terms; ++t) {
    const std::pair<uint64_t, uint64_t> key{terms[t].x_mask, terms[t].z_mask}, moved{rot(key.first), rot(key.second)};
    const auto it = merged.find(moved);
    const double there = it == merged.end() ? 0.0 : it->second;
    if (there == merged[key]) continue;
    char hex[64];
    std::snprintf(hex, sizeof hex, "(x_mask 0x%llx, z_mask 0x%llx)", (unsigned long long)key.first, (unsigned long long)key.second);
    LL_REQUIRE(false, "term " + std::to_string(t) + " " + hex + " does not commute with the one-site translation of the ring: "
                      "shifted by one site it meets a different coefficient (an open chain, or bonds that differ); a momentum "
                      "sector needs a translation-invariant H");
  }
}
// the momentum argument of the three momentum-block operators
template <typename T> void pauli_require_momentum(int32_t n_sites, int32_t momentum) {
  LL_REQUIRE(momentum >= 0 && momentum < n_sites, "momentum must lie in [0, n_sites) (the block of k = 2 pi momentum / n_sites)");
  LL_REQUIRE(scalar_traits<T>::is_complex || (2 * momentum) % n_sites == 0,
             "a real storage type takes momentum 0 and n_sites / 2 only (the other blocks are complex Hermitian); use a complex "
             "storage type");
}
// ratio[Ra * 32 + Rb] = sqrt(Ra / Rb) for the orbit lengths of a ring of at most 30 sites: the table of both momentum-block operators
std::vector<double> momentum_ratio_table() {
  std::vector<double> ratio(32 * 32, 0.0);
  for (int a = 1; a < 32; ++a)
    for (int b = 1; b < 32; ++b) ratio[(size_t)a * 32 + (size_t)b] = std::sqrt((double)a / (double)b);
  return ratio;
}
// phase[l] = e^(-2 pi i m l / n_sites) as (re, im), l < n_sites, exact on the axes: the table of the three momentum-block operators
void momentum_phase_table(int32_t n_sites, int32_t momentum, std::vector<double>& phase) {
  for (int l = 0; l < n_sites; ++l) {
    const int k = (int)(((int64_t)momentum * l) % n_sites);
    const double th = 2.0 * M_PI * (double)k / (double)n_sites;
    double c = std::cos(th), sn = -std::sin(th);
    if (4 * k % n_sites == 0) {
      const int quarter = 4 * k / n_sites;  // 0 .. 3
      c = quarter == 0 ? 1.0 : quarter == 2 ? -1.0 : 0.0;
      sn = quarter == 1 ? -1.0 : quarter == 3 ? 1.0 : 0.0;
    }
    phase[2 * (size_t)l] = c;
    phase[2 * (size_t)l + 1] = sn;
  }
}
// The binary necklaces of n_sites bits in ascending order with their periods, by the Fredricksen-Kessler-Maiorana enumeration: a
// string read from site n_sites - 1 down to site 0 that is the lexicographically smallest of its rotations is the smallest
// integer of its orbit, and the enumeration yields these strings in ascending order with their period (the length of the Lyndon
// word they repeat) — one step per pre-necklace, about two steps per necklace, no pass over the 2^n_sites states.  A step: raise
// the lowest 0 bit (position i from the top), drop what lies below it and repeat the top i bits downwards; the result is a
// necklace iff i divides n_sites, and then its period is i.  visit(a, period) is called for every necklace, the string of zeros
// (period 1) first.
template <typename Visit> void for_each_necklace(int L, Visit visit) {
  const uint32_t site_mask = (uint32_t)(((uint64_t)1 << L) - 1);
  visit((uint32_t)0, 1);
  uint32_t a = 0;
  while (a != site_mask) {
    const int low0 = __builtin_ctz(~a);  // the lowest 0 bit of a (a != all ones): string position i = L - low0 from the top
    const int i = L - low0;
    a = ((a >> low0) | 1u) << low0;      // raise it, clear what lies below
    for (int sft = i; sft < L; sft *= 2) a |= a >> sft;  // repeat the top i bits downwards (bits shifted out fall off the end)
    if (L % i != 0) continue;            // a pre-necklace only
    visit(a, i);
  }
}
// The bucket table over the top bits of ascending representatives (PauliMomentumFullImage): the largest power of two not above
// dim / 8 buckets (the table stays below dim / 2 bytes), and the halvings that bring the largest bucket down to one candidate.
struct RepBuckets {
  std::vector<uint32_t> start;
  int shift = 0, trips = 0;
  int64_t max_bucket = 0;
};
RepBuckets rep_buckets(int L, const std::vector<uint32_t>& reps) {
  const int64_t dim = (int64_t)reps.size();
  RepBuckets rb;
  int pb = 0;
  while (pb < L && ((int64_t)2 << pb) <= dim / 8) ++pb;
  rb.shift = L - pb;
  rb.start.assign(((size_t)1 << pb) + 1, 0);
  for (int64_t k = 0; k < dim; ++k) ++rb.start[(size_t)(reps[(size_t)k] >> rb.shift) + 1];
  for (size_t q = 1; q < rb.start.size(); ++q) {
    rb.max_bucket = std::max<int64_t>(rb.max_bucket, rb.start[q]);
    rb.start[q] += rb.start[q - 1];
  }
  for (int64_t n = rb.max_bucket; n > 1; n -= n / 2) ++rb.trips;  // n -> n - n / 2
  return rb;
}
// the representatives, their orbit lengths and the bucket table of an image on the device, under the allocation names what[3]
void pauli_upload_reps(ll_context* ctx, PauliRepImage& im, const std::vector<uint32_t>& reps, const std::vector<uint8_t>& orbit_len,
                       const RepBuckets& rb, const char* const (&what)[3]) {
  im.prefix_shift = rb.shift;
  im.search_trips = rb.trips;
  im.max_bucket = rb.max_bucket;
  pauli_upload(ctx, im.reps, reps, what[0]);
  pauli_upload(ctx, im.orbit_len, orbit_len, what[1]);
  pauli_upload(ctx, im.start, rb.start, what[2]);
}
// Reflection invariance: with the coefficients of equal (x_mask, z_mask) merged (summed in the caller's order), reversing the
// n_sites bits of every term's masks must map the term set onto itself with exactly equal coefficients (a missing term counts
// as coefficient 0).  A site permutation moves X, Y, Z factors without a sign, so the caller's coefficients are compared.
void pauli_require_reflection_invariant(int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms) {
  auto rev = [&](uint64_t v) {
    uint64_t r = 0;
    for (int j = 0; j < n_sites; ++j) r |= ((v >> j) & 1u) << (n_sites - 1 - j);
    return r;
  };
  std::map<std::pair<uint64_t, uint64_t>, double> merged;
  for (int64_t t = 0; t < n_terms; ++t) merged[{terms[t].x_mask, terms[t].z_mask}] += terms[t].coef;
  for (int64_t t = 0; t < n_terms; ++t) {
    const std::pair<uint64_t, uint64_t> key{terms[t].x_mask, terms[t].z_mask}, moved{rev(key.first), rev(key.second)};
    const auto it = merged.find(moved);
    const double there = it == merged.end() ? 0.0 : it->second;
    if (there == merged[key]) continue;
    char hex[64];
    std::snprintf(hex, sizeof hex, "(x_mask 0x%llx, z_mask 0x%llx)", (unsigned long long)key.first, (unsigned long long)key.second);
    LL_REQUIRE(false, "term " + std::to_string(t) + " " + hex + " does not commute with the reflection of the ring (site j -> "
                      "n_sites - 1 - j): reflected it meets a different coefficient (a Dzyaloshinskii-Moriya bond, or bonds that "
                      "differ); a parity block needs a reflection-invariant H");
  }
}
// Spin-inversion invariance: prod_j X_j anticommutes with every Y and Z factor, so a string commutes with it iff popcount(z_mask)
// is even; with equal masks merged, a term of odd popcount(z_mask) must have the coefficient 0.
void pauli_require_inversion_invariant(int64_t n_terms, const ll_pauli_term* terms) {
  std::map<std::pair<uint64_t, uint64_t>, double> merged;
  for (int64_t t = 0; t < n_terms; ++t) merged[{terms[t].x_mask, terms[t].z_mask}] += terms[t].coef;
  for (int64_t t = 0; t < n_terms; ++t) {
    const std::pair<uint64_t, uint64_t> key{terms[t].x_mask, terms[t].z_mask};
    if ((__builtin_popcountll(key.second) & 1) == 0 || merged[key] == 0.0) continue;
    char hex[64];
    std::snprintf(hex, sizeof hex, "(x_mask 0x%llx, z_mask 0x%llx)", (unsigned long long)key.first, (unsigned long long)key.second);
    LL_REQUIRE(false, "term " + std::to_string(t) + " " + hex + " does not commute with the global spin flip (the product of all "
                      "X_j): it holds an odd number of Y and Z factors (a longitudinal field, for example); a spin-inversion "
                      "block needs an H that is even under the flip");
  }
}
}  // namespace

// One momentum block of that sector (pauli_momentum.hip).  One pass over the sector's states in ascending order, on the host: the
// first state of an orbit not seen before is its representative; walking the orbit gives its period R and, for the blocks's
// orbits (m R = 0 mod n_sites), the entries orbit[rank(T^j r)] = (index of r << 5 | j).
template <typename T>
void create_pauli_momentum(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                           const ll_pauli_term* terms, ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(n_down >= 0 && n_down <= n_sites, "n_down must lie in [0, n_sites] (the number of flipped spins of the sector)");
  pauli_require_momentum<T>(n_sites, momentum);
  pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
  pauli_require_translation_invariant(n_sites, n_terms, terms);
  const SectorTables st = sector_tables(n_sites, n_down);
  const uint32_t site_mask = (uint32_t)(((uint64_t)1 << n_sites) - 1);
  auto rot = [&](uint32_t v) { return ((v << 1) | (v >> (n_sites - 1))) & site_mask; };
  std::vector<uint32_t> orbit((size_t)st.dim, kPauliOrbitExcluded), reps;
  std::vector<uint8_t> orbit_len;
  std::vector<bool> seen((size_t)st.dim, false);
  bool any_short = false;
  for (int64_t i = 0; i < st.dim; ++i) {
    if (seen[(size_t)i]) continue;
    const uint32_t r = st.states[(size_t)i];  // ascending order: the smallest state of a new orbit
    int R = 0;
    for (uint32_t t = r;;) {
      seen[(size_t)st.rank(t)] = true;
      ++R;
      if ((t = rot(t)) == r) break;
    }
    if (((int64_t)momentum * R) % n_sites != 0) continue;  // the orbit's states keep kPauliOrbitExcluded
    const uint64_t idx = reps.size();
    LL_REQUIRE(idx < ((uint64_t)1 << (32 - kPauliOrbitShiftBits)) - 1, "internal: a momentum block of 2^27 states or more");
    uint32_t t = r;
    for (int j = 0; j < R; ++j, t = rot(t)) orbit[(size_t)st.rank(t)] = (uint32_t)(idx << kPauliOrbitShiftBits) | (uint32_t)j;
    reps.push_back(r);
    orbit_len.push_back((uint8_t)R);
    any_short = any_short || R != n_sites;
  }
  static_assert(kPauliMaxSites < (1 << kPauliOrbitShiftBits), "the shift l of an orbit entry needs n_sites < 2^5");
  const int64_t dim = (int64_t)reps.size();
  LL_REQUIRE(dim >= 1, "the momentum block is empty: no orbit of the sector (n_sites " + std::to_string(n_sites) + ", n_down " +
                           std::to_string(n_down) + ") has a length R with momentum * R = 0 (mod n_sites)");
  const std::vector<double> ratio = momentum_ratio_table();
  std::vector<double> phase(2 * (size_t)n_sites);
  momentum_phase_table(n_sites, momentum, phase);
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::PAULI_MOMENTUM, dim, 0, dim);
  op->nnz = n_terms;
  op->inf_norm = pt.norm;  // sum_t |c_t| >= ||H||_2 >= ||B^H H B||_2: a bound of every |eigenvalue| of the block
  PauliMomentumImage im;
  im.n_sites = n_sites;
  im.n_down = n_down;
  im.momentum = momentum;
  im.h = st.h;
  im.dim = dim;
  im.sector_dim = st.dim;
  if (any_short)  // the primes q of n_sites: a state has a short orbit iff rotating it by n_sites / q gives it back for one of them
    for (int q = 2, rest = n_sites; rest > 1; ++q)
      if (rest % q == 0) {
        LL_REQUIRE(im.nshort < 3, "internal: more than three primes in n_sites");
        im.short_shift[im.nshort++] = n_sites / q;
        while (rest % q == 0) rest /= q;
      }
  pauli_upload_tables(ctx, im.terms, pt);
  pauli_upload(ctx, im.reps, reps, "momentum block representatives");
  pauli_upload(ctx, im.orbit_len, orbit_len, "momentum block orbit lengths");
  pauli_upload(ctx, im.orbit, orbit, "momentum block orbit table");
  pauli_upload(ctx, im.lo_rank, st.lo_rank, "S_z sector rank table (low bits)");
  pauli_upload(ctx, im.hi_rank, st.hi_rank, "S_z sector rank table (high bits)");
  pauli_upload(ctx, im.ratio, ratio, "momentum block norm ratios");
  pauli_upload(ctx, im.phase, phase, "momentum block phases");
  op->pauli_momentum = std::move(im);
  *out = op.release();
}

// One momentum block of the full 2^n_sites space (pauli_momentum_full.hip).  The representatives and their periods come from the
// necklace enumeration (for_each_necklace): ascending, about two steps per representative, no pass over the 2^n_sites states.
template <typename T>
void create_pauli_momentum_full(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  pauli_require_momentum<T>(n_sites, momentum);
  pauli_require_translation_invariant(n_sites, n_terms, terms);
  const int L = n_sites;
  std::vector<uint32_t> reps;
  std::vector<uint8_t> orbit_len;
  {
    // a lower bound of D_m that saves most of the re-allocations: the orbits of full length alone, when the block takes them
    reps.reserve((size_t)(((uint64_t)1 << L) / (uint64_t)L) + 64);
    orbit_len.reserve(reps.capacity());
    for_each_necklace(L, [&](uint32_t a, int i) {  // the string of zeros (period 1) lies in block 0 only
      if (((int64_t)momentum * i) % L != 0) return;
      LL_REQUIRE(reps.size() < (((size_t)1 << 27) - 1), "internal: a momentum block of 2^27 states or more");
      reps.push_back(a);
      orbit_len.push_back((uint8_t)i);
    });
  }
  const int64_t dim = (int64_t)reps.size();
  // never empty: the state 0..01 has the full period n_sites, which every m admits (n_sites = 1: m = 0, and both states have R = 1)
  LL_REQUIRE(dim >= 1, "internal: an empty momentum block of the full space");
  const RepBuckets rb = rep_buckets(L, reps);
  const std::vector<double> ratio = momentum_ratio_table();
  std::vector<double> phase(2 * (size_t)n_sites);
  momentum_phase_table(n_sites, momentum, phase);
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::PAULI_MOMENTUM_FULL, dim, 0, dim);
  op->nnz = n_terms;
  op->inf_norm = pt.norm;  // sum_t |c_t| >= ||H||_2 >= ||B^H H B||_2: a bound of every |eigenvalue| of the block
  PauliMomentumFullImage im;
  im.n_sites = n_sites;
  im.momentum = momentum;
  im.dim = dim;
  pauli_upload_tables(ctx, im.terms, pt);
  pauli_upload_reps(ctx, im.basis, reps, orbit_len, rb,
                    {"momentum block representatives", "momentum block orbit lengths", "momentum block bucket table"});
  pauli_upload(ctx, im.ratio, ratio, "momentum block norm ratios");
  pauli_upload(ctx, im.phase, phase, "momentum block phases");
  op->pauli_momentum_full = std::move(im);
  *out = op.release();
}

// One block under momentum, reflection and spin inversion (pauli_symmetric.hip).  Every necklace a (the smallest of its
// rotations) is the representative of its G-orbit iff it is not above the smallest rotation of rev(a), ~a and ~rev(a), whichever
// are in use; walking the L rotations of each stream in use collects its stabiliser — the orbit length R = |G| / |stabiliser|
// and whether the character is 1 on all of it — and the popcount filter follows: O(n_sites) per necklace, O(2^n_sites) steps
// over all of them, on the host, with no table over the states.
template <typename T>
void create_pauli_symmetric(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity, int32_t inversion,
                            int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(parity >= -1 && parity <= 1, "parity must be 0 (the reflection is not used), +1 or -1");
  LL_REQUIRE(inversion >= -1 && inversion <= 1, "inversion must be 0 (the global spin flip is not used), +1 or -1");
  LL_REQUIRE(n_down >= -1 && n_down <= n_sites,
             "n_down must lie in [-1, n_sites] (-1: the full space; else the number of flipped spins of the sector)");
  pauli_require_momentum<T>(n_sites, momentum);
  LL_REQUIRE(parity == 0 || (2 * momentum) % n_sites == 0,
             "parity != 0 takes momentum 0 and n_sites / 2 only (the reflection maps momentum k to -k: the group of shifts and "
             "the reflection has one-dimensional characters only there); use parity = 0");
  pauli_require_translation_invariant(n_sites, n_terms, terms);
  if (parity != 0) pauli_require_reflection_invariant(n_sites, n_terms, terms);
  if (inversion != 0) pauli_require_inversion_invariant(n_terms, terms);
  if (n_down >= 0) {
    pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
    LL_REQUIRE(inversion == 0 || 2 * n_down == n_sites,
               "inversion != 0 with n_down >= 0 needs 2 n_down = n_sites (the global spin flip maps the sector n_down onto "
               "n_sites - n_down)");
  }
  const int L = n_sites;
  const uint32_t site_mask = (uint32_t)(((uint64_t)1 << L) - 1);
  const int group_size = L * (parity != 0 ? 2 : 1) * (inversion != 0 ? 2 : 1);
  auto rot = [&](uint32_t v) { return ((v << 1) | (v >> (L - 1))) & site_mask; };
  auto rev = [&](uint32_t v) {
    uint32_t r = 0;
    for (int j = 0; j < L; ++j) r |= ((v >> j) & 1u) << (L - 1 - j);
    return r;
  };
  std::vector<uint32_t> reps;
  std::vector<uint8_t> orbit_len;
  for_each_necklace(L, [&](uint32_t a, int) {
    if (n_down >= 0 && __builtin_popcount(a) != n_down) return;  // G keeps the popcount (inversion: 2 n_down = L)
    int stab = 0;
    bool least = true, admitted = true;
    for (int rho = 0; rho <= (parity != 0 ? 1 : 0); ++rho)
      for (int zeta = 0; zeta <= (inversion != 0 ? 1 : 0); ++zeta) {
        uint32_t cur = rho ? rev(a) : a;
        if (zeta) cur ^= site_mask;
        const bool neg = (rho && parity < 0) != (zeta && inversion < 0);
        for (int j = 0; j < L; ++j) {  // cur = T^j P^rho Z^zeta a; its character in units of pi / L: 2 m j, + L for a factor -1
          if (cur < a) least = false;
          if (cur == a) {
            ++stab;
            if ((2 * (int64_t)momentum * j + (neg ? L : 0)) % (2 * L) != 0) admitted = false;
          }
          cur = rot(cur);
        }
      }
    if (!least || !admitted) return;
    LL_REQUIRE(reps.size() < (((size_t)1 << 27) - 1), "a block of 2^27 - 1 states or more (32-bit indices with room for the search)");
    reps.push_back(a);
    orbit_len.push_back((uint8_t)(group_size / stab));
  });
  const int64_t dim = (int64_t)reps.size();
  LL_REQUIRE(dim >= 1, "the block (momentum " + std::to_string(momentum) + ", parity " + std::to_string(parity) + ", inversion " +
                           std::to_string(inversion) + ", n_down " + std::to_string(n_down) +
                           ") is empty: no orbit carries this character");
  const RepBuckets rb = rep_buckets(L, reps);
  // ratio[R_a][c] = sqrt(R_a / R_b) for the orbit length R_b = |G| / c of a stabiliser of c elements
  std::vector<double> ratio((size_t)kPauliSymmetricRatioStride * kPauliSymmetricRatioStride, 0.0), phase(2 * (size_t)n_sites);
  for (int a = 1; a <= group_size; ++a)
    for (int c = 1; c <= group_size; ++c)
      if (group_size % c == 0)
        ratio[(size_t)a * kPauliSymmetricRatioStride + (size_t)c] = std::sqrt((double)a / (double)(group_size / c));
  momentum_phase_table(n_sites, momentum, phase);
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, ll_operator::PAULI_SYMMETRIC, dim, 0, dim);
  op->nnz = n_terms;
  op->inf_norm = pt.norm;  // sum_t |c_t| >= ||H||_2 >= ||B^H H B||_2: a bound of every |eigenvalue| of the block
  PauliSymmetricImage im;
  im.n_sites = n_sites;
  im.n_down = n_down;
  im.momentum = momentum;
  im.parity = parity;
  im.inversion = inversion;
  im.group_size = group_size;
  im.dim = dim;
  pauli_upload_tables(ctx, im.terms, pt);
  pauli_upload_reps(ctx, im.basis, reps, orbit_len, rb,
                    {"symmetry block representatives", "symmetry block orbit lengths", "symmetry block bucket table"});
  pauli_upload(ctx, im.ratio, ratio, "symmetry block norm ratios");
  pauli_upload(ctx, im.phase, phase, "symmetry block phases");
  op->pauli_symmetric = std::move(im);
  *out = op.release();
}

template <typename T>
void create_cb(ll_context* ctx, int64_t n, ll_host_mv_mul_z host_fn, ll_dev_mv_mul dev_fn, void* user, ll_operator** out) {
  LL_REQUIRE(host_fn != nullptr || dev_fn != nullptr, "null callback");
  use(ctx);
  LL_REQUIRE(out != nullptr && n >= 1, "bad argument");
  LL_REQUIRE(ctx->nranks == 1, "callback operators are not supported on sharded contexts");
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, host_fn ? ll_operator::HOST_CB : ll_operator::DEV_CB, n, 0, n);
  op->host_fn = host_fn;
  op->dev_fn = dev_fn;
  op->user = user;
  *out = op.release();
}

#define LL_INST_OPERATORS(T)                                                                                                     \
  template void create_csr<T>(ll_context*, int64_t, int64_t, int64_t, const int64_t*, const int32_t*, const void*,              \
                              const ll_csr_options&, ll_operator**);                                                            \
  template void create_coo<T>(ll_context*, int64_t, int64_t, const int32_t*, const int32_t*, const void*, ll_operator**);       \
  template void create_csr_sym<T>(ll_context*, int64_t, int, const int64_t*, const int32_t*, const void*, const ll_csr_options*, \
                                  ll_operator**);                                                                               \
  template void create_dense<T>(ll_context*, int64_t, int64_t, int64_t, const void*, ll_operator**);                            \
  template void create_stencil<T>(ll_context*, const ll_stencil_desc*, int64_t, int64_t, const double*, ll_operator**);        \
  template void create_pauli<T>(ll_context*, int32_t, int64_t, const ll_pauli_term*, ll_operator**);                             \
  template void create_pauli_sector<T>(ll_context*, int32_t, int32_t, int64_t, const ll_pauli_term*, ll_operator**);             \
  template void create_pauli_momentum<T>(ll_context*, int32_t, int32_t, int32_t, int64_t, const ll_pauli_term*, ll_operator**);  \
  template void create_pauli_momentum_full<T>(ll_context*, int32_t, int32_t, int64_t, const ll_pauli_term*, ll_operator**);    \
  template void create_pauli_symmetric<T>(ll_context*, int32_t, int32_t, int32_t, int32_t, int32_t, int64_t, const ll_pauli_term*, \
                                          ll_operator**);                                                                      \
  template void create_cb<T>(ll_context*, int64_t, ll_host_mv_mul_z, ll_dev_mv_mul, void*, ll_operator**);
LL_FOR_EACH_SCALAR(LL_INST_OPERATORS)

}  // namespace ll
