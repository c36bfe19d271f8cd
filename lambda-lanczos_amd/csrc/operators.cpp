// Operator construction: the images of a CSR matrix (upload, SpMV tiles, the column split, the PB and tiled builds, their
// creation-time timing and the kernel choice), the one-triangle and COO forms, the dense, lattice and callback operators, and the
// accuracy policy that gives every image its form (the Pauli-string operators: pauli_operators.cpp).  The extern "C" entry points (capi.cpp, documented in include/lanczos_hip.h)
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
      if (ctx->tune.test_workspace_fill >= 0)  // (test hook: the product buffer behind the copied matrix streams)
        ctx->test_fill((char*)cand.back().get() + pb.arena_static_bytes, cand_bytes - pb.arena_static_bytes);
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

}  // namespace

const char* operator_kind_name(int kind) {
  switch (kind) {
    case ll_operator::PAULI: return "a full-space sum of Pauli strings";
    case ll_operator::PAULI_SECTOR: return "a sum of Pauli strings on an S_z sector";
    case ll_operator::CSR: return "a CSR operator";
    case ll_operator::HOST_CB: return "a host-callback operator";
    case ll_operator::DEV_CB: return "a device-callback operator";
    case ll_operator::DENSE: return "a dense operator";
    case ll_operator::STENCIL: return "a lattice operator";
    case ll_operator::PAULI_MOMENTUM: return "a momentum block of an S_z sector";
    case ll_operator::PAULI_MOMENTUM_FULL: return "a momentum block of the full space";
    case ll_operator::PAULI_SYMMETRIC: return "a momentum / reflection / spin-inversion block";
    case ll_operator::PAULI_TORUS: return "a translation block of a torus";
    default: return "an operator of an unknown kind";
  }
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

namespace {
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
  template std::unique_ptr<ll_operator> new_operator<T>(ll_context*, ll_operator::Kind, int64_t, int64_t, int64_t);           \
  template void create_csr<T>(ll_context*, int64_t, int64_t, int64_t, const int64_t*, const int32_t*, const void*,              \
                              const ll_csr_options&, ll_operator**);                                                            \
  template void create_coo<T>(ll_context*, int64_t, int64_t, const int32_t*, const int32_t*, const void*, ll_operator**);       \
  template void create_csr_sym<T>(ll_context*, int64_t, int, const int64_t*, const int32_t*, const void*, const ll_csr_options*, \
                                  ll_operator**);                                                                               \
  template void create_dense<T>(ll_context*, int64_t, int64_t, int64_t, const void*, ll_operator**);                            \
  template void create_stencil<T>(ll_context*, const ll_stencil_desc*, int64_t, int64_t, const double*, ll_operator**);        \
  template void create_cb<T>(ll_context*, int64_t, ll_host_mv_mul_z, ll_dev_mv_mul, void*, ll_operator**);
LL_FOR_EACH_SCALAR(LL_INST_OPERATORS)

}  // namespace ll
