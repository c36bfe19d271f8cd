// extern "C" surface of liblanczos_hip.so: declared in include/lanczos_hip.h, which documents every entry point
// and cites the reference interface it replaces.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdlib>
#include <limits>
#include <memory>

#include "engine.hpp"

namespace ll {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
}  // namespace ll

using namespace ll;

// ---------------------------------------------------------------- tuning (ll_internal.hpp: ll::Tuning)
// ONE parser for every setting, by key.  The library reads the USER-FACING switches from the environment (kEnvSwitches:
// the list of INTEGRATION.md section 8) when a context is created; everything else — block geometries, forced code paths, the
// hooks the test suite needs — is reachable only through ll_ctx_set_tuning(ctx, key, value), an explicit call on one context
// that is documented as unstable: a stray variable in a user's environment cannot change the numerics path of a drop-in.
namespace ll {
namespace {
long long to_ll(const std::string& v) { return std::atoll(v.c_str()); }
bool to_flag(const std::string& v) { return std::atoi(v.c_str()) != 0; }
// the block-geometry keys of the Pauli kernels: 2^b states or indices per workgroup
int Tuning::*pauli_bits_key(const std::string& key) {
  static const std::pair<const char*, int Tuning::*> keys[] = {
      {"pauli_tile_bits", &Tuning::pauli_tile_bits}, {"pauli_sector_block_bits", &Tuning::pauli_sector_block_bits},
      {"pauli_momentum_block_bits", &Tuning::pauli_momentum_block_bits},
      {"pauli_momentum_full_block_bits", &Tuning::pauli_momentum_full_block_bits},
      {"pauli_symmetric_block_bits", &Tuning::pauli_symmetric_block_bits}};
  for (const auto& k : keys)
    if (key == k.first) return k.second;
  return nullptr;
}
}  // namespace
bool tuning_apply(Tuning& t, const std::string& key, const std::string& v) {
  const Tuning d;  // defaults (an empty value restores the default of its key)
  const bool e = v.empty();
  // ---- user-facing (also read from the environment, kEnvSwitches below)
  if (key == "spmv_kernel") t.spmv_kernel = v == "csr" ? LL_SPMV_CSR_STREAM : (v == "pb" ? LL_SPMV_PB : (v == "tiled" ? LL_SPMV_TILED : -1));
  else if (key == "spmv_keep_both") t.keep_both = e ? d.keep_both : to_flag(v);
  else if (key == "pb_phase2") t.pb_phase2 = v == "atomic" ? LL_PB_ATOMIC : (v == "ordered" ? LL_PB_ORDERED : LL_PB_FIXED);
  else if (key == "pb_placements") t.pb_placements = e ? d.pb_placements : (int)std::max<long long>(1, std::min<long long>(16, to_ll(v)));
  else if (key == "pb_placement_trace") t.pb_placement_trace = e ? false : to_flag(v);
  else if (key == "comm_overlap") t.comm_overlap = e ? d.comm_overlap : to_flag(v);
  else if (key == "gather_chunks") t.gather_chunks = e ? 0 : (int)std::max<long long>(0, to_ll(v));
  else if (key == "csr_split") t.csr_split = e ? d.csr_split : to_flag(v);
  else if (key == "iter_trace") t.iter_trace = v;
  else if (key == "sharded_norm") t.sharded_norm_measured = v == "measured";
  else if (key == "pair_gs") t.pair_gs = e ? d.pair_gs : to_flag(v);
  else if (key == "pb_diag") t.pb_diag = e ? d.pb_diag : to_flag(v);
  else if (key == "fuse_launches") {
    const long long level = e ? 2 : to_ll(v);
    t.fuse_launches = level >= 1;
    t.lagged_gs = level >= 2;
  } else if (key == "blas_small_bytes") t.blas_small_bytes = e ? d.blas_small_bytes : to_ll(v);
  else if (key == "tridiag_thread") t.tridiag_thread = e ? d.tridiag_thread : to_flag(v);
  else if (key == "tridiag_lag") t.tridiag_lag = e ? d.tridiag_lag : (int)to_ll(v);
  else if (key == "dgks_threshold") t.dgks_threshold = e ? d.dgks_threshold : std::atof(v.c_str());
  else if (key == "slab_bytes") t.slab_bytes = e ? d.slab_bytes : std::max<long long>(1, to_ll(v));
  // ---- unstable: ll_ctx_set_tuning only (tests, tools/ probes, A/B measurements)
  else if (key == "pb_block") t.pb_block = e ? 0 : (int)std::max<long long>(0, to_ll(v));
  else if (key == "pb_row_block") t.pb_row_block = e ? 0 : (int)std::max<long long>(0, to_ll(v));
  else if (key == "pb_col_block") t.pb_col_block = e ? 0 : (int)std::max<long long>(0, to_ll(v));
  else if (key == "pb_threads1") {
    t.pb_threads1 = e ? 0 : (int)to_ll(v);
    if (t.pb_threads1 != 256 && t.pb_threads1 != 512 && t.pb_threads1 != 1024) t.pb_threads1 = 0;
  } else if (key == "pb_pad") {
    t.pb_pad = e ? 0 : (int)to_ll(v);
    if (t.pb_pad != 4 && t.pb_pad != 16) t.pb_pad = 0;
  } else if (key == "pb_xpre") t.pb_xpre = e ? d.pb_xpre : to_flag(v);
  else if (key == "pb_test_all_remote") t.pb_test_all_remote = e ? false : to_flag(v);
  else if (key == "force_rp64") t.force_rp64 = e ? false : to_flag(v);
  else if (key == "spmv_tile_balance") t.spmv_tile_balance = e ? d.spmv_tile_balance : to_flag(v);
  else if (int Tuning::*bits = pauli_bits_key(key)) t.*bits = e ? d.*bits : (int)std::max<long long>(0, std::min<long long>(30, to_ll(v)));
  else if (key == "stencil_vec") t.stencil_vec = e ? d.stencil_vec : to_flag(v);
  else if (key == "tl_force") t.tl_force = e ? false : to_flag(v);
  else if (key == "tl_xcd") t.tl_xcd_order = e ? d.tl_xcd_order : to_flag(v);
  else if (key == "tl_walk") t.tl_walk_modulo = e ? d.tl_walk_modulo : to_flag(v);
  else if (key == "ritz_tail") t.ritz_tail = e ? d.ritz_tail : to_flag(v);
  else if (key == "event_in_launch") t.event_in_launch = e ? d.event_in_launch : to_flag(v);
  else if (key == "sweep_pipeline") t.sweep_pipeline = e ? d.sweep_pipeline : (int)std::max<long long>(0, std::min<long long>(2, to_ll(v)));
  else if (key == "pair_split") t.pair_split_vecs = e ? 0 : (int)std::max<long long>(0, to_ll(v));
  else if (key == "pair_max_stored") t.pair_max_stored = e ? 0 : (int)std::max<long long>(0, to_ll(v));
  else if (key == "lagged_pieces") t.lagged_pieces = e ? 0 : (int)to_ll(v);
  else if (key == "lagged_min_bytes") t.lagged_min_bytes = e ? -1 : to_ll(v);
  else if (key == "tridiag_test_jitter_us") t.tridiag_test_jitter_us = e ? 0 : (int)to_ll(v);
  else if (key == "stall_trace") t.stall_trace_ms = e ? -1.0 : std::atof(v.c_str());
  else return false;
  return true;
}
// environment variable -> key: the switches a user may set.  LL_COMM_PLUGIN and LL_ROCTX are read
// where they are used (comm.cpp, trace.hpp), once per communicator / process.
static const char* const kEnvSwitches[][2] = {
    {"LL_SPMV_KERNEL", "spmv_kernel"},       {"LL_SPMV_KEEP_BOTH", "spmv_keep_both"}, {"LL_PB_PHASE2", "pb_phase2"},
    {"LL_PB_PLACEMENTS", "pb_placements"},   {"LL_PB_PLACEMENT_TRACE", "pb_placement_trace"},
    {"LL_COMM_OVERLAP", "comm_overlap"},     {"LL_GATHER_CHUNKS", "gather_chunks"},   {"LL_CSR_SPLIT", "csr_split"},
    {"LL_ITER_TRACE", "iter_trace"},         {"LL_SHARDED_NORM", "sharded_norm"},     {"LL_PAIR_GS", "pair_gs"},
    {"LL_PB_DIAG", "pb_diag"},               {"LL_FUSE_LAUNCHES", "fuse_launches"},   {"LL_BLAS_SMALL_BYTES", "blas_small_bytes"},
    {"LL_TRIDIAG_THREAD", "tridiag_thread"}, {"LL_TRIDIAG_LAG", "tridiag_lag"},       {"LL_DGKS_THRESHOLD", "dgks_threshold"},
    {"LL_SLAB_BYTES", "slab_bytes"},
};
Tuning read_tuning(const std::map<std::string, std::string>* overrides) {
  Tuning t;
  for (auto& sw : kEnvSwitches) {
    const char* e = std::getenv(sw[0]);
    if (e && *e) (void)tuning_apply(t, sw[1], e);
  }
  if (overrides)
    for (auto& kv : *overrides) (void)tuning_apply(t, kv.first, kv.second);
  return t;
}
}  // namespace ll

// ---------------------------------------------------------------- context workspace
static size_t grow(size_t have, size_t want) { return std::max(want, have + have / 2 + 64); }

void ll_context::dev_malloc(void** out, size_t bytes, const char* what) {
  hipError_t e = hipMalloc(out, std::max<size_t>(bytes, 16));
  if (e != hipSuccess && !slab_cache.empty()) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(stream);
    for (auto& c : slab_cache) (void)hipFree(c.first);
    slab_cache.clear();
    e = hipMalloc(out, std::max<size_t>(bytes, 16));
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error(std::string("out of device memory: ") + what + " (" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    throw Failure{LL_ERR_ALLOC};
  }
}
void ll_context::cache_put(void* p, size_t bytes) {
  slab_cache.emplace_back(p, bytes);
  // Bounded: over the limit, a buffer of a DIFFERENT size than the one just returned goes first (oldest of those) — a Basis
  // that returns more slabs than the bound must not push out its own first slabs, which the next run of the same problem
  // would have to allocate again (hipFree synchronises the device); only when every entry has the incoming size does the
  // oldest one go.  One pass per eviction; evictions happen at the bound only, never inside a loop.
  while (slab_cache.size() > kSlabCacheMaxEntries) {
    size_t victim = 0;
    for (size_t i = 0; i + 1 < slab_cache.size(); ++i)
      if (slab_cache[i].second != bytes) {
        victim = i;
        break;
      }
    (void)hipFree(slab_cache[victim].first);
    slab_cache.erase(slab_cache.begin() + (long)victim);
  }
}
template <typename T> T* ll_context::ensure(Workspace<T>& w, size_t count, bool geometric, const char* what) {
  if (count <= w.cap) return w.get();
  LL_HIP(w.buf.free_now());
  const size_t cap = geometric ? grow(w.cap, count) : count;
  w.buf = dev_alloc<T>(cap, what);
  w.cap = cap;
  return w.get();
}
template double* ll_context::ensure<double>(Workspace<double>&, size_t, bool, const char*);
template void* ll_context::ensure<void>(Workspace<void>&, size_t, bool, const char*);
void ll_context::ensure_pinned(size_t doubles) {
  if (doubles <= pinned.cap) return;
  LL_HIP(pinned.buf.free_now());
  const size_t cap = grow(pinned.cap, doubles);
  // device-mapped, coherent host memory: the publish kernel stores the per-iteration scalars straight into it
  double* p = nullptr;
  hipError_t e = hipHostMalloc((void**)&p, cap * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    LL_HIP(hipHostMalloc((void**)&p, cap * sizeof(double), hipHostMallocDefault));
  }
  pinned.buf = HostArray<double>(p);
  pinned.cap = cap;
}
static void* ensure_host(Workspace<void, hipHostFree>& w, size_t bytes) {
  LL_HIP(w.buf.free_now());
  const size_t cap = grow(w.cap, bytes);
  void* p = nullptr;
  LL_HIP(hipHostMalloc(&p, cap, hipHostMallocDefault));
  w.buf = HostArray<void>(p);
  w.cap = cap;
  return p;
}
void* ll_context::ensure_stage(size_t bytes) { return bytes <= stage.cap ? stage.get() : ensure_host(stage, bytes); }
void* ll_context::ensure_cb_stage(size_t bytes) {
  if (bytes <= cb.cap) return cb.get();
  LL_HIP(hipStreamSynchronize(stream));  // an H2D copy out of the old buffer may still be in flight
  return ensure_host(cb, bytes);
}
void ll_context::sync() { LL_HIP(hipStreamSynchronize(stream)); }
void ll_context::drain_comm_events(double* gather_s, double* allreduce_s) {
  auto drain = [](std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double* acc) {
    for (auto& p : v) {
      float ms = 0.f;
      if (hipEventSynchronize(p.second) == hipSuccess && hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess && acc)
        *acc += ms * 1e-3;
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
    v.clear();
  };
  drain(ev_gather, gather_s);
  drain(ev_allreduce, allreduce_s);
  (void)hipGetLastError();
}

// ---------------------------------------------------------------- operator storage
ll_operator::~ll_operator() {
  if (ctx) (void)hipSetDevice(ctx->device);  // before the images free their arrays
}

// ---------------------------------------------------------------- exception -> status
template <typename F> static int guarded(F&& f) {
  try {
    f();
    return LL_OK;
  } catch (const Failure& e) {
    return e.code;
  } catch (const std::bad_alloc&) {
    set_error("host allocation failed");
    return LL_ERR_ALLOC;
  } catch (const std::exception& e) {
    set_error(std::string("unexpected exception: ") + e.what());
    return LL_ERR_INVALID;
  }
}

void ll::use(ll_context* ctx) {
  LL_REQUIRE(ctx != nullptr, "null context");
  LL_HIP(hipSetDevice(ctx->device));
}

extern "C" {

const char* ll_last_error(void) { return g_last_error.c_str(); }
int ll_version(void) { return LL_VERSION_MAJOR * 1000 + LL_VERSION_MINOR; }
int ll_abi_check(int caller_major, int caller_minor, size_t sizeof_run_stats, size_t sizeof_lanczos_params) {
  // minors 3 -> 4 only added entry points: a caller compiled against any of them sees the same structs
  if (caller_major == LL_VERSION_MAJOR && caller_minor >= 3 && caller_minor <= LL_VERSION_MINOR && sizeof_run_stats == sizeof(ll_run_stats) &&
      sizeof_lanczos_params == sizeof(ll_lanczos_params))
    return LL_OK;
  set_error("ABI mismatch: the caller was compiled against lanczos_hip.h " + std::to_string(caller_major) + "." +
            std::to_string(caller_minor) + " (ll_run_stats " + std::to_string(sizeof_run_stats) + " B, ll_lanczos_params " +
            std::to_string(sizeof_lanczos_params) + " B), the loaded library is " + std::to_string(LL_VERSION_MAJOR) + "." +
            std::to_string(LL_VERSION_MINOR) + " (" + std::to_string(sizeof(ll_run_stats)) + " / " +
            std::to_string(sizeof(ll_lanczos_params)) + " B): rebuild the caller");
  return LL_ERR_INVALID;
}

static int ctx_create_impl(int device, void* stream, bool own, ll_context** out) {
  return guarded([&] {
    LL_REQUIRE(out != nullptr, "null output pointer");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
      set_error(std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                "); this library has no CPU fallback");
      (void)hipGetLastError();
      throw Failure{LL_ERR_HIP};
    }
    LL_REQUIRE(device >= 0 && device < count, "device index out of range");
    LL_HIP(hipSetDevice(device));
    std::unique_ptr<ll_context> c(new ll_context);
    c->device = device;
    c->tune = read_tuning(nullptr);
    if (own) {
      LL_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
      c->own_stream = true;
    } else {
      c->stream = (hipStream_t)stream;
    }
    double* scal = nullptr;
    LL_HIP(hipMalloc((void**)&scal, kScalCount * sizeof(double)));
    c->scal = DevArray<double>(scal);
    LL_HIP(hipMemset(scal, 0, kScalCount * sizeof(double)));
    *out = c.release();
  });
}
int ll_ctx_create(int device, ll_context** out) { return ctx_create_impl(device, nullptr, true, out); }
int ll_ctx_create_on_stream(int device, void* hip_stream, ll_context** out) {
  return ctx_create_impl(device, hip_stream, false, out);
}
int ll_ctx_destroy(ll_context* ctx) {
  return guarded([&] {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
    ctx->drain_comm_events(nullptr, nullptr);
    comm_destroy(ctx->comm);
    if (ctx->ev_x_ready) (void)hipEventDestroy(ctx->ev_x_ready);
    for (auto e : ctx->ev_chunk)
      if (e) (void)hipEventDestroy(e);
    if (ctx->ev_xmax) (void)hipEventDestroy(ctx->ev_xmax);
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    if (ctx->ev_cb) (void)hipEventDestroy(ctx->ev_cb);
    for (auto& c : ctx->slab_cache) (void)hipFree(c.first);
    for (auto e : ctx->timer_events) (void)hipEventDestroy(e);
    if (ctx->t0) (void)hipEventDestroy(ctx->t0);
    if (ctx->t1) (void)hipEventDestroy(ctx->t1);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;  // (the workspace buffers free themselves)
  });
}
int ll_ctx_reload_env(ll_context* ctx) {
  return guarded([&] {
    LL_REQUIRE(ctx != nullptr, "null context");
    ctx->tune = read_tuning(&ctx->tuning_overrides);
  });
}
int ll_ctx_set_tuning(ll_context* ctx, const char* key, const char* value) {
  return guarded([&] {
    LL_REQUIRE(ctx != nullptr && key != nullptr, "null argument");
    Tuning probe;
    LL_REQUIRE(tuning_apply(probe, key, value ? value : ""), std::string("ll_ctx_set_tuning: unknown key '") + key + "'");
    if (value) ctx->tuning_overrides[key] = value;
    else ctx->tuning_overrides.erase(key);
    ctx->tune = read_tuning(&ctx->tuning_overrides);
  });
}
int ll_ctx_stream(ll_context* ctx, void** out) {
  return guarded([&] {
    LL_REQUIRE(ctx && out, "null argument");
    *out = (void*)ctx->stream;
  });
}
int ll_ctx_synchronize(ll_context* ctx) {
  return guarded([&] {
    use(ctx);
    ctx->sync();
  });
}
int ll_ctx_release_cache(ll_context* ctx) {
  return guarded([&] {
    use(ctx);
    ctx->sync();
    for (auto& c : ctx->slab_cache) (void)hipFree(c.first);
    ctx->slab_cache.clear();
  });
}
int ll_ctx_set_profiling(ll_context* ctx, int enabled) {
  return guarded([&] {
    LL_REQUIRE(ctx != nullptr, "null context");
    ctx->profiling = enabled != 0;
    if (!ctx->profiling) ctx->drain_comm_events(nullptr, nullptr);
  });
}

// ---------------------------------------------------------------- device timer (HIP events on the context's stream)
int ll_timer_start(ll_context* ctx) {
  return guarded([&] {
    use(ctx);
    if (!ctx->t0) {
      LL_HIP(hipEventCreate(&ctx->t0));
      LL_HIP(hipEventCreate(&ctx->t1));
    }
    LL_HIP(hipEventRecord(ctx->t0, ctx->stream));
  });
}
int ll_timer_stop(ll_context* ctx, double* ms_out) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(ctx->t0 != nullptr && ms_out != nullptr, "timer not started");
    LL_HIP(hipEventRecord(ctx->t1, ctx->stream));
    LL_HIP(hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    LL_HIP(hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    *ms_out = (double)ms;
  });
}
int ll_bandwidth_probe(ll_context* ctx, size_t bytes, double* read_GBps, double* copy_GBps) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(bytes >= ((size_t)1 << 20) && read_GBps && copy_GBps, "ll_bandwidth_probe: at least 1 MiB and two outputs");
    bytes &= ~(size_t)4095;
    struct Events {
      hipEvent_t e0 = nullptr, e1 = nullptr;
      ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
      }
    } w;
    hipStream_t s = ctx->stream;
    const DevArray<void> a = ctx->dev_alloc<void>(bytes, "bandwidth probe (source)");
    const DevArray<void> b = ctx->dev_alloc<void>(bytes, "bandwidth probe (destination)");
    const DevArray<double> out = ctx->dev_alloc<double>(2, "bandwidth probe (sink)");
    LL_HIP(hipMemsetAsync(a.get(), 0, bytes, s));
    LL_HIP(hipMemsetAsync(b.get(), 0, bytes, s));
    LL_HIP(hipEventCreate(&w.e0));
    LL_HIP(hipEventCreate(&w.e1));
    auto timed = [&](auto launch) {  // best grid of a few, three launches each behind one warm-up
      double best = 1e30;
      for (int grid : {512, 1024, 2048, 8192}) {
        launch(grid);
        LL_HIP(hipEventRecord(w.e0, s));
        for (int r = 0; r < 3; ++r) launch(grid);
        LL_HIP(hipEventRecord(w.e1, s));
        LL_HIP(hipEventSynchronize(w.e1));
        float ms = 0.f;
        LL_HIP(hipEventElapsedTime(&ms, w.e0, w.e1));
        best = std::min(best, (double)ms / 3.0);
      }
      return best;
    };
    const double ms_r = timed([&](int g) { launch_bw_read(a.get(), bytes, out.get(), g, s); });
    const double ms_c = timed([&](int g) { launch_bw_copy(a.get(), b.get(), bytes, g, s); });
    *read_GBps = (double)bytes / (ms_r * 1e-3) / 1e9;
    *copy_GBps = 2.0 * (double)bytes / (ms_c * 1e-3) / 1e9;  // bytes read + bytes written
  });
}

// ---------------------------------------------------------------- multi-GPU
int ll_comm_unique_id(void* id) {
  return guarded([&] {
    LL_REQUIRE(id != nullptr, "null id buffer");
    comm_unique_id(id);
  });
}
extern "C++" {
namespace {
// After the communicator exists: the second stream + events of the overlapped exchange, and a SELF-CHECK — every rank
// contributes (rank + 1) to an all-gather and the constant 1 to an all-reduce; a communicator that silently spans
// fewer ranks than asked for (or delivers shards in another order) fails here instead of producing a wrong spectrum.
void finish_comm_setup_impl(ll_context* ctx) {
  LL_HIP(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
  LL_HIP(hipEventCreateWithFlags(&ctx->ev_x_ready, hipEventDisableTiming));
  for (auto& e : ctx->ev_chunk) LL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  LL_HIP(hipEventCreateWithFlags(&ctx->ev_xmax, hipEventDisableTiming));
  const int P = ctx->nranks;
  double* p = nullptr;
  LL_HIP(hipMalloc((void**)&p, (size_t)(P + 2) * sizeof(double)));
  const DevArray<double> buf(p);
  double* const d = buf.get();
  std::vector<double> h((size_t)P + 2, 0.0);
  h[(size_t)P] = (double)(ctx->rank + 1);  // send slot
  h[(size_t)P + 1] = 1.0;                  // all-reduce slot
  LL_HIP(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // the gather runs on the communication stream, the reduction on the compute stream: the two-stream order of the loop
  LL_HIP(hipEventRecord(ctx->ev_x_ready, ctx->stream));
  LL_HIP(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_x_ready, 0));
  comm_allgather(ctx->comm, d + P, d, sizeof(double), ctx->comm_stream);
  LL_HIP(hipEventRecord(ctx->ev_chunk[0], ctx->comm_stream));
  LL_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_chunk[0], 0));
  comm_allreduce_sum(ctx->comm, d + P + 1, 1, ctx->stream);
  LL_HIP(hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LL_HIP(hipStreamSynchronize(ctx->stream));
  int seen = 0;
  for (int r = 0; r < P; ++r)
    if (h[(size_t)r] == (double)(r + 1)) ++seen;
  ctx->ranks_seen = seen;
  if (seen != P || h[(size_t)P + 1] != (double)P) {
    set_error("communicator self-check failed: all-gather delivered " + std::to_string(seen) + " of " + std::to_string(P) +
              " rank tags, all-reduce of ones gave " + std::to_string(h[(size_t)P + 1]));
    throw Failure{LL_ERR_RCCL};
  }
}
// A communicator whose set-up or self-check failed must not stay attached: the context would look sharded with a
// transport known to be broken (later operators would be created as shards, their collectives could hang, and a retry
// of ll_comm_init / ll_comm_attach would be refused).  Everything is undone and the error is passed on.
void finish_comm_setup(ll_context* ctx) {
  try {
    finish_comm_setup_impl(ctx);
  } catch (...) {
    (void)hipGetLastError();
    if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
    (void)hipStreamSynchronize(ctx->stream);
    comm_destroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->rank = 0;
    ctx->nranks = 1;
    ctx->ranks_seen = 0;
    if (ctx->ev_x_ready) (void)hipEventDestroy(ctx->ev_x_ready);
    ctx->ev_x_ready = nullptr;
    for (auto& e : ctx->ev_chunk) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
    if (ctx->ev_xmax) (void)hipEventDestroy(ctx->ev_xmax);
    ctx->ev_xmax = nullptr;
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    ctx->comm_stream = nullptr;
    (void)hipGetLastError();
    throw;
  }
}
}  // namespace
}  // extern "C++"

int ll_comm_init(ll_context* ctx, const void* id, int rank, int n_ranks) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(id != nullptr, "null id");
    LL_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "rank out of range");
    LL_REQUIRE(ctx->comm == nullptr, "communicator already attached");
    ctx->comm = comm_create(id, rank, n_ranks, ctx->device);
    ctx->rank = rank;
    ctx->nranks = n_ranks;
    finish_comm_setup(ctx);
  });
}
int ll_comm_attach(ll_context* ctx, const ll_transport* transport, int rank, int n_ranks) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(transport && transport->all_gather && transport->all_reduce_sum_f64 && transport->halo_exchange,
               "incomplete transport table");
    LL_REQUIRE(n_ranks >= 1 && rank >= 0 && rank < n_ranks, "rank out of range");
    LL_REQUIRE(ctx->comm == nullptr, "communicator already attached");
    ctx->comm = comm_attach(transport, rank, n_ranks);
    ctx->rank = rank;
    ctx->nranks = n_ranks;
    finish_comm_setup(ctx);
  });
}
int ll_comm_ranks_seen(ll_context* ctx, int* out) {
  return guarded([&] {
    LL_REQUIRE(ctx != nullptr && out != nullptr, "null argument");
    *out = ctx->comm ? ctx->ranks_seen : 1;
  });
}
int ll_comm_transport(ll_context* ctx, char* out, size_t cap) {
  return guarded([&] {
    LL_REQUIRE(ctx != nullptr && out != nullptr && cap > 0, "null argument");
    const std::string name = comm_transport_name(ctx->comm);
    std::snprintf(out, cap, "%s", name.c_str());
  });
}
int ll_comm_rank(ll_context* ctx, int* rank, int* n_ranks) {
  return guarded([&] {
    LL_REQUIRE(ctx != nullptr, "null context");
    if (rank) *rank = ctx->rank;
    if (n_ranks) *n_ranks = ctx->nranks;
  });
}
int ll_partition(int64_t n, int n_ranks, int rank, int64_t* row_begin, int64_t* n_local) {
  return guarded([&] {
    LL_REQUIRE(n >= 0 && n_ranks >= 1 && rank >= 0 && rank < n_ranks, "bad partition request");
    const int64_t shard = (n + n_ranks - 1) / n_ranks;
    const int64_t b = std::min<int64_t>(n, shard * rank), e = std::min<int64_t>(n, shard * (rank + 1));
    if (row_begin) *row_begin = b;
    if (n_local) *n_local = e - b;
  });
}

// ---------------------------------------------------------------- memory helpers
int ll_malloc(ll_context* ctx, size_t bytes, void** out) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(out != nullptr, "null output pointer");
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) {
      set_error(std::string("hipMalloc(") + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
      throw Failure{LL_ERR_ALLOC};
    }
  });
}
int ll_free(ll_context* ctx, void* p) {
  return guarded([&] {
    use(ctx);
    if (p) LL_HIP(hipFree(p));
  });
}
int ll_memcpy_h2d(ll_context* ctx, void* dst, const void* src, size_t bytes) {
  return guarded([&] {
    use(ctx);
    LL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();
  });
}
int ll_memcpy_d2h(ll_context* ctx, void* dst, const void* src, size_t bytes) {
  return guarded([&] {
    use(ctx);
    LL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
  });
}
int ll_memset(ll_context* ctx, void* dst, int byte, size_t bytes) {
  return guarded([&] {
    use(ctx);
    LL_HIP(hipMemsetAsync(dst, byte, bytes, ctx->stream));
  });
}

// ---------------------------------------------------------------- operators (operators.cpp, pauli_operators.cpp build them)
int ll_op_create_csr_d(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                       const double* va, ll_operator** out) {
  return guarded([&] { create_csr<double>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(false), out); });
}
int ll_op_create_csr_z(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                       const void* va, ll_operator** out) {
  return guarded([&] { create_csr<zc>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(false), out); });
}
int ll_csr_options_default(ll_csr_options* opt) {
  return guarded([&] {
    LL_REQUIRE(opt != nullptr, "null options");
    std::memset(opt, 0, sizeof(*opt));
    opt->accuracy = LL_ACCURACY_DEFAULT;
    opt->kernel = -1;
  });
}
int ll_op_create_csr_opt_d(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const double* va, const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr<double>(ctx, nr, nc, rb, rp, ci, va, opt ? *opt : csr_options_default(false), out); });
}
int ll_op_create_csr_opt_z(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const void* va, const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr<zc>(ctx, nr, nc, rb, rp, ci, va, opt ? *opt : csr_options_default(false), out); });
}
int ll_op_create_csr_opt_s(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const float* va, const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr<float>(ctx, nr, nc, rb, rp, ci, va, opt ? *opt : csr_options_default(false), out); });
}
int ll_op_create_csr_opt_c(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const void* va, const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr<cf>(ctx, nr, nc, rb, rp, ci, va, opt ? *opt : csr_options_default(false), out); });
}
int ll_op_create_csr_dev_d(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const double* va, ll_operator** out) {
  return guarded([&] { create_csr<double>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(true), out); });
}
int ll_op_create_csr_dev_z(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const void* va, ll_operator** out) {
  return guarded([&] { create_csr<zc>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(true), out); });
}
int ll_op_create_csr_sym_d(ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const double* va,
                           const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr_sym<double>(ctx, n, uplo, rp, ci, va, opt, out); });
}
int ll_op_create_csr_sym_z(ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const void* va,
                           const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr_sym<zc>(ctx, n, uplo, rp, ci, va, opt, out); });
}
int ll_op_create_csr_sym_s(ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const float* va,
                           const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr_sym<float>(ctx, n, uplo, rp, ci, va, opt, out); });
}
int ll_op_create_csr_sym_c(ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const void* va,
                           const ll_csr_options* opt, ll_operator** out) {
  return guarded([&] { create_csr_sym<cf>(ctx, n, uplo, rp, ci, va, opt, out); });
}
int ll_op_device_bytes(const ll_operator* op, int64_t* bytes) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && bytes != nullptr, "null argument");
    if (op->ctx) LL_HIP(hipSetDevice(op->ctx->device));
    *bytes = op->device_bytes();
  });
}
int ll_op_create_coo_d(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols,
                       const double* vals, ll_operator** out) {
  return guarded([&] { create_coo<double>(ctx, n, nnz, rows, cols, vals, out); });
}
int ll_op_create_coo_z(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols,
                       const void* vals, ll_operator** out) {
  return guarded([&] { create_coo<zc>(ctx, n, nnz, rows, cols, vals, out); });
}
int ll_op_inf_norm(const ll_operator* op, double* out) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && out != nullptr, "null argument");
    LL_REQUIRE(op->inf_norm >= 0.0, "the infinity norm is only known for CSR/COO/dense/lattice operators created from host data");
    *out = op->inf_norm;
  });
}
int ll_op_create_dense_d(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const double* a, ll_operator** out) {
  return guarded([&] { create_dense<double>(ctx, nr, nc, rb, a, out); });
}
int ll_op_create_stencil_d(ll_context* ctx, const ll_stencil_desc* desc, int64_t rb, int64_t nl, const double* onsite,
                           ll_operator** out) {
  return guarded([&] { create_stencil<double>(ctx, desc, rb, nl, onsite, out); });
}
int ll_op_create_dense_z(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const void* a, ll_operator** out) {
  return guarded([&] { create_dense<zc>(ctx, nr, nc, rb, a, out); });
}
int ll_op_create_stencil_z(ll_context* ctx, const ll_stencil_desc* desc, int64_t rb, int64_t nl, const double* onsite,
                           ll_operator** out) {
  return guarded([&] { create_stencil<zc>(ctx, desc, rb, nl, onsite, out); });
}
int ll_op_create_pauli_d(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli<double>(ctx, n_sites, n_terms, terms, out); });
}
int ll_op_create_pauli_z(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli<zc>(ctx, n_sites, n_terms, terms, out); });
}
int ll_op_create_pauli_s(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli<float>(ctx, n_sites, n_terms, terms, out); });
}
int ll_op_create_pauli_c(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli<cf>(ctx, n_sites, n_terms, terms, out); });
}
int ll_op_create_pauli_sector_d(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out) {
  return guarded([&] { create_pauli_sector<double>(ctx, n_sites, n_down, n_terms, terms, out); });
}
int ll_op_create_pauli_sector_z(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out) {
  return guarded([&] { create_pauli_sector<zc>(ctx, n_sites, n_down, n_terms, terms, out); });
}
int ll_op_create_pauli_sector_s(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out) {
  return guarded([&] { create_pauli_sector<float>(ctx, n_sites, n_down, n_terms, terms, out); });
}
int ll_op_create_pauli_sector_c(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out) {
  return guarded([&] { create_pauli_sector<cf>(ctx, n_sites, n_down, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_d(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum<double>(ctx, n_sites, n_down, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_z(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum<zc>(ctx, n_sites, n_down, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_s(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum<float>(ctx, n_sites, n_down, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_c(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum<cf>(ctx, n_sites, n_down, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_full_d(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum_full<double>(ctx, n_sites, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_full_z(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum_full<zc>(ctx, n_sites, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_full_s(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum_full<float>(ctx, n_sites, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_momentum_full_c(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_momentum_full<cf>(ctx, n_sites, momentum, n_terms, terms, out); });
}
int ll_op_create_pauli_symmetric_d(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_symmetric<double>(ctx, n_sites, n_down, momentum, parity, inversion, n_terms, terms, out); });
}
int ll_op_create_pauli_symmetric_z(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_symmetric<zc>(ctx, n_sites, n_down, momentum, parity, inversion, n_terms, terms, out); });
}
int ll_op_create_pauli_symmetric_s(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_symmetric<float>(ctx, n_sites, n_down, momentum, parity, inversion, n_terms, terms, out); });
}
int ll_op_create_pauli_symmetric_c(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] { create_pauli_symmetric<cf>(ctx, n_sites, n_down, momentum, parity, inversion, n_terms, terms, out); });
}
int ll_op_create_host_d(ll_context* ctx, int64_t n, ll_host_mv_mul_d fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<double>(ctx, n, reinterpret_cast<ll_host_mv_mul_z>(fn), nullptr, user, out); });
}
int ll_op_create_host_z(ll_context* ctx, int64_t n, ll_host_mv_mul_z fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<zc>(ctx, n, fn, nullptr, user, out); });
}
int ll_op_create_device_d(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<double>(ctx, n, nullptr, fn, user, out); });
}
int ll_op_create_device_z(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<zc>(ctx, n, nullptr, fn, user, out); });
}
int ll_op_destroy(ll_operator* op) {
  return guarded([&] { delete op; });  // ~ll_operator releases the device arrays
}
int ll_op_select_spmv(ll_operator* op, int kind) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && op->kind == ll_operator::CSR, "not a CSR operator");
    LL_REQUIRE(kind == LL_SPMV_CSR_STREAM || kind == LL_SPMV_PB || kind == LL_SPMV_TILED || kind == LL_SPMV_SYM, "unknown SpMV kernel");
    LL_REQUIRE(kind != LL_SPMV_SYM || op->sym.present(),
               "operator has no one-triangle image (only ll_op_create_csr_sym_* builds it, when it selects that kernel)");
    LL_REQUIRE(kind != LL_SPMV_PB || op->pb.present(),
               "operator has no propagation-blocked image (not selected at creation; LL_SPMV_KEEP_BOTH=1 keeps every image)");
    LL_REQUIRE(kind != LL_SPMV_CSR_STREAM || op->has_csr_stream(),
               "operator has released its CSR image (another kernel was selected at creation; LL_SPMV_KEEP_BOTH=1 keeps every image)");
    LL_REQUIRE(kind != LL_SPMV_TILED || op->tl.present(),
               "operator has no tiled image (matrix not eligible, or not selected at creation; LL_SPMV_KEEP_BOTH=1 keeps every image)");
    op->spmv_kind = kind;
  });
}
int ll_op_set_accuracy(ll_operator* op, int accuracy) {
  return guarded([&] { set_op_accuracy(op, accuracy); });
}
int ll_op_accuracy(const ll_operator* op, int* accuracy_out) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && accuracy_out != nullptr, "null argument");
    *accuracy_out = op_accuracy(op);
  });
}
int ll_op_selected_spmv(const ll_operator* op, int* kind_out) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && kind_out != nullptr, "null argument");
    *kind_out = op->spmv_kind;
  });
}
int ll_op_autotune_ms(const ll_operator* op, double* csr_stream_ms, double* pb_ms) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr, "null operator");
    if (csr_stream_ms) *csr_stream_ms = (double)op->tune_ms[LL_SPMV_CSR_STREAM];
    if (pb_ms) *pb_ms = (double)op->tune_ms[LL_SPMV_PB];
  });
}
int ll_op_autotune_ms_of(const ll_operator* op, int kind, double* ms) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && ms != nullptr && kind >= LL_SPMV_CSR_STREAM && kind <= LL_SPMV_SYM, "bad argument");
    *ms = kind == LL_SPMV_SYM ? -1.0 : (double)op->tune_ms[kind];  // (the one-triangle kernel is never timed)
  });
}
int ll_op_tiled_layout(const ll_operator* op, int* row_blocks, int* own_column_row_blocks) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr, "null operator");
    if (row_blocks) *row_blocks = op->tl.nrb;
    if (own_column_row_blocks) *own_column_row_blocks = op->ctx->nranks > 1 ? op->tl.n_interior : op->tl.nrb;
  });
}
int ll_op_info(const ll_operator* op, int64_t* n, int64_t* n_local, int64_t* nnz) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr, "null operator");
    if (n) *n = op->n;
    if (n_local) *n_local = op->n_local;
    if (nnz) *nnz = op->sym_stored >= 0 ? op->sym_stored : op->nnz;  // created from one triangle: the entries stored
  });
}

// ---------------------------------------------------------------- primitives
extern "C++" {
namespace {
template <typename T> void spmv_impl(ll_context* ctx, ll_operator* op, const T* x, T* y, double offset, double* dot) {
  use(ctx);
  LL_REQUIRE(op && op->ctx == ctx && x && y, "bad argument");
  LL_REQUIRE(op->is_complex == scalar_traits<T>::is_complex && op->elem_bytes == (int)sizeof(T),
             "operator scalar type mismatch");
  Engine<T> E(ctx, op, op->n_local);
  E.apply(x, y, offset, dot ? E.S(kScalSpare) : nullptr);
  if (dot) E.fetch(E.S(kScalSpare), dot, 1);
}
template <typename T> void dot_impl(ll_context* ctx, int64_t n, const T* a, const T* b, double* out) {
  use(ctx);
  LL_REQUIRE(n >= 0 && a && b && out, "bad argument");
  Engine<T> E(ctx, nullptr, n);
  E.dot_dev(a, b, E.S(kScalSpare));
  E.fetch(E.S(kScalSpare), out, scalar_traits<T>::reals);
}
template <typename T> void nrm2_impl(ll_context* ctx, int64_t n, const T* v, double* out) {
  use(ctx);
  LL_REQUIRE(n >= 0 && v && out, "bad argument");
  Engine<T> E(ctx, nullptr, n);
  E.norm2_dev(v, E.S(kScalSpare));
  double nn = 0;
  E.fetch(E.S(kScalSpare), &nn, 1);
  *out = std::sqrt(nn);
}
template <typename T> void normalize_impl(ll_context* ctx, int64_t n, T* v, double* norm_out) {
  use(ctx);
  LL_REQUIRE(n >= 0 && v, "bad argument");
  Engine<T> E(ctx, nullptr, n);
  E.norm2_dev(v, E.S(kScalSpare));
  const NormRefs nr = E.plain_norm(E.S(kScalSpare));
  launch_scale<T>(n, v, 0.0, &nr, ctx->stream);
  if (norm_out) {
    double nn = 0;
    E.fetch(E.S(kScalSpare), &nn, 1);
    *norm_out = std::sqrt(nn);
  }
}
template <typename T>
void orth_impl(ll_context* ctx, int64_t n, int64_t nb, const T* basis, int64_t ld, T* w, int mode, double* norm_out,
               double* h_out) {
  use(ctx);
  LL_REQUIRE(n >= 0 && nb >= 0 && w && (basis || nb == 0) && ld >= n, "bad argument");
  LL_REQUIRE(mode >= LL_ORTH_CGS_DGKS && mode <= LL_ORTH_MGS, "unknown orthogonalisation mode");
  constexpr int R = scalar_traits<T>::reals;
  Engine<T> E(ctx, nullptr, n);
  RunList<T> runs;
  runs.ld = ld;
  runs.add(basis, nb);
  const ThreeTerm<T> no_tt{nullptr, nullptr, nullptr, NormRefs{nullptr, nullptr, nullptr, 0}};
  double* d_htot = nullptr;
  if (h_out && nb > 0) LL_HIP(hipMalloc((void**)&d_htot, (size_t)R * nb * sizeof(double)));
  const DevArray<double> htot(d_htot);
  const NormRefs refs = E.orth(w, runs, mode, no_tt, E.S(kScalScratch), d_htot);
  ctx->ensure_pinned(16);
  launch_publish(ctx->pinned.get() + 8, nullptr, refs, ctx->stream);
  ctx->sync();
  if (norm_out) *norm_out = std::sqrt(ctx->pinned.get()[9]);
  if (d_htot) LL_HIP(hipMemcpy(h_out, d_htot, (size_t)R * nb * sizeof(double), hipMemcpyDeviceToHost));
}
template <typename T, typename C>
void gemv_impl(ll_context* ctx, int64_t n, int64_t m, const T* basis, int64_t ld, int64_t nout, const C* coeff,
               T* out, int64_t ld_out) {
  use(ctx);
  LL_REQUIRE(n >= 0 && m >= 1 && nout >= 1 && basis && coeff && out && ld >= n && ld_out >= n, "bad argument");
  Engine<T> E(ctx, nullptr, n);
  RunList<T> runs;
  runs.ld = ld;
  runs.add(basis, m);
  if constexpr (std::is_same<C, T>::value) E.gemv(runs, m, (int)nout, coeff, out, ld_out);
  else E.gemv_acc(runs, m, (int)nout, coeff, out, ld_out);
}
}  // namespace
}  // extern "C++"

int ll_spmv_d(ll_context* ctx, ll_operator* op, const double* x, double* y, double offset, double* dot) {
  return guarded([&] { spmv_impl<double>(ctx, op, x, y, offset, dot); });
}
int ll_spmv_z(ll_context* ctx, ll_operator* op, const void* x, void* y, double offset, double* dot) {
  return guarded([&] { spmv_impl<zc>(ctx, op, (const zc*)x, (zc*)y, offset, dot); });
}
int ll_dot_d(ll_context* ctx, int64_t n, const double* a, const double* b, double* out) {
  return guarded([&] { dot_impl<double>(ctx, n, a, b, out); });
}
int ll_dot_z(ll_context* ctx, int64_t n, const void* a, const void* b, double* out) {
  return guarded([&] { dot_impl<zc>(ctx, n, (const zc*)a, (const zc*)b, out); });
}
int ll_nrm2_d(ll_context* ctx, int64_t n, const double* v, double* out) {
  return guarded([&] { nrm2_impl<double>(ctx, n, v, out); });
}
int ll_nrm2_z(ll_context* ctx, int64_t n, const void* v, double* out) {
  return guarded([&] { nrm2_impl<zc>(ctx, n, (const zc*)v, out); });
}
int ll_scal_d(ll_context* ctx, int64_t n, double a, double* v) {
  return guarded([&] {
    use(ctx);
    launch_scale<double>(n, v, a, nullptr, ctx->stream);
  });
}
int ll_scal_z(ll_context* ctx, int64_t n, double a, void* v) {
  return guarded([&] {
    use(ctx);
    launch_scale<zc>(n, (zc*)v, a, nullptr, ctx->stream);
  });
}
int ll_normalize_d(ll_context* ctx, int64_t n, double* v, double* norm_out) {
  return guarded([&] { normalize_impl<double>(ctx, n, v, norm_out); });
}
int ll_normalize_z(ll_context* ctx, int64_t n, void* v, double* norm_out) {
  return guarded([&] { normalize_impl<zc>(ctx, n, (zc*)v, norm_out); });
}
int ll_three_term_d(ll_context* ctx, int64_t n, double* w, const double* up, const double* uc, double beta,
                    double alpha) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(w && uc, "null vector");
    launch_three_term<double>(n, w, up, uc, beta, alpha, ctx->stream);
  });
}
int ll_three_term_z(ll_context* ctx, int64_t n, void* w, const void* up, const void* uc, double beta, double alpha) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(w && uc, "null vector");
    launch_three_term<zc>(n, (zc*)w, (const zc*)up, (const zc*)uc, beta, alpha, ctx->stream);
  });
}
extern "C++" {
namespace {
template <typename T>
void recur_accum_impl(ll_context* ctx, int64_t n, void* y, const void* x, const void* p, double a, double b, double g, void* psi) {
  use(ctx);
  LL_REQUIRE(n >= 0 && y && x && psi, "null vector");
  launch_recur_accum<T>(n, (T*)y, (const T*)x, (const T*)p, (T*)psi, nullptr, nullptr, 0, a, b, g, nullptr, 0, nullptr, ctx->stream);
}
template <typename T>
void two_pass_impl(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, void* eigvec, int64_t* itern,
                   double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  LL_REQUIRE(ctx && p && eigval, "null argument");
  two_pass_run<T>(ctx, op, *p, eigval, (T*)eigvec, itern, residual, alpha_out, beta_out, stats);
}
}  // namespace
}  // extern "C++"
int ll_recur_accum_d(ll_context* ctx, int64_t n, double* y, const double* x, const double* p, double a, double b, double g,
                     double* psi) {
  return guarded([&] { recur_accum_impl<double>(ctx, n, y, x, p, a, b, g, psi); });
}
int ll_recur_accum_z(ll_context* ctx, int64_t n, void* y, const void* x, const void* p, double a, double b, double g, void* psi) {
  return guarded([&] { recur_accum_impl<zc>(ctx, n, y, x, p, a, b, g, psi); });
}
int ll_recur_accum_c(ll_context* ctx, int64_t n, void* y, const void* x, const void* p, double a, double b, double g, void* psi) {
  return guarded([&] { recur_accum_impl<cf>(ctx, n, y, x, p, a, b, g, psi); });
}
int ll_recur_accum_s(ll_context* ctx, int64_t n, float* y, const float* x, const float* p, double a, double b, double g,
                     float* psi) {
  return guarded([&] { recur_accum_impl<float>(ctx, n, y, x, p, a, b, g, psi); });
}
int ll_lanczos_two_pass_d(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, double* eigvec,
                          int64_t* itern, double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] { two_pass_impl<double>(ctx, op, p, eigval, eigvec, itern, residual, alpha_out, beta_out, stats); });
}
int ll_lanczos_two_pass_z(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, void* eigvec,
                          int64_t* itern, double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] { two_pass_impl<zc>(ctx, op, p, eigval, eigvec, itern, residual, alpha_out, beta_out, stats); });
}
int ll_lanczos_two_pass_c(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, void* eigvec,
                          int64_t* itern, double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] { two_pass_impl<cf>(ctx, op, p, eigval, eigvec, itern, residual, alpha_out, beta_out, stats); });
}
int ll_lanczos_two_pass_s(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, float* eigvec,
                          int64_t* itern, double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] { two_pass_impl<float>(ctx, op, p, eigval, eigvec, itern, residual, alpha_out, beta_out, stats); });
}
int ll_orth_block_d(ll_context* ctx, int64_t n, int64_t nb, const double* basis, int64_t ld, double* w, int mode,
                    double* norm_out, double* h_out) {
  return guarded([&] { orth_impl<double>(ctx, n, nb, basis, ld, w, mode, norm_out, h_out); });
}
int ll_orth_block_z(ll_context* ctx, int64_t n, int64_t nb, const void* basis, int64_t ld, void* w, int mode,
                    double* norm_out, double* h_out) {
  return guarded([&] { orth_impl<zc>(ctx, n, nb, (const zc*)basis, ld, (zc*)w, mode, norm_out, h_out); });
}
int ll_gemv_basis_d(ll_context* ctx, int64_t n, int64_t m, const double* basis, int64_t ld, int64_t nout,
                    const double* coeff, double* out, int64_t ld_out) {
  return guarded([&] { gemv_impl<double>(ctx, n, m, basis, ld, nout, coeff, out, ld_out); });
}
int ll_gemv_basis_z(ll_context* ctx, int64_t n, int64_t m, const void* basis, int64_t ld, int64_t nout,
                    const double* coeff, void* out, int64_t ld_out) {
  return guarded([&] { gemv_impl<zc>(ctx, n, m, (const zc*)basis, ld, nout, (const zc*)coeff, (zc*)out, ld_out); });
}
int ll_tridiag_eig(int64_t m, const double* alpha, const double* beta, double* ev, double* q, int64_t* unconverged) {
  return guarded([&] {
    LL_REQUIRE(m >= 1 && alpha && ev && (beta || m == 1), "bad argument");
    const int64_t u = tridiag_qr(m, alpha, beta, ev, q);
    if (unconverged) *unconverged = u;
  });
}
int ll_tridiag_bisect_multi(int64_t m, const double* alpha, const double* beta, int64_t nk, const int64_t* ks, double* out) {
  return guarded([&] {
    LL_REQUIRE(m >= 1 && alpha && out && ks && nk >= 1 && (beta || m == 1), "bad argument");
    for (int64_t j = 0; j < nk; ++j) LL_REQUIRE(ks[j] >= 0 && ks[j] < m, "root index out of range");
    tridiag_bisect_multi(m, alpha, beta, (int)nk, ks, out);
  });
}
int ll_tridiag_eigvecs(int64_t m, const double* alpha, const double* beta, int64_t nw, const double* lambdas,
                       double* out) {
  return guarded([&] {
    LL_REQUIRE(m >= 1 && nw >= 1 && alpha && lambdas && out && (beta || m == 1), "bad argument");
    tridiag_inverse_iteration(m, alpha, beta, nw, lambdas, out);
  });
}
int ll_tridiag_bisect(int64_t m, const double* alpha, const double* beta, int64_t k, double* out) {
  return guarded([&] {
    LL_REQUIRE(m >= 1 && alpha && out && k >= 0 && k < m && (beta || m == 1), "bad argument");
    *out = tridiag_bisect(m, alpha, beta, k);
  });
}

// ---------------------------------------------------------------- whole-loop entry points
int ll_lanczos_params_default(ll_lanczos_params* p, int64_t n, int find_maximum, int64_t num_eigs) {
  return guarded([&] {
    LL_REQUIRE(p != nullptr, "null params");
    std::memset(p, 0, sizeof(*p));
    p->matrix_size = n;                                           // LL:136
    p->max_iteration = n;                                         // LL:206
    p->eps = std::numeric_limits<double>::epsilon() * 1e3;        // LL:150
    p->find_maximum = find_maximum ? 1 : 0;                       // LL:153
    p->num_eigs = num_eigs;                                       // LL:156
    p->eigenvalue_offset = 0.0;                                   // LL:165
    p->num_eigs_per_iteration = 5;                                // LL:173
    p->initial_vector_size = 200;                                 // LL:181
    p->tridiag_mode = LL_TRIDIAG_AUTO;  // decision- and value-identical to the reference's per-iteration QR, O(k) instead of O(k^2)
    p->orth_mode = LL_ORTH_CGS_DGKS;
  });
}
int ll_expo_params_default(ll_expo_params* p, int64_t n) {
  return guarded([&] {
    LL_REQUIRE(p != nullptr, "null params");
    std::memset(p, 0, sizeof(*p));
    p->matrix_size = n;                                           // EX:44
    p->max_iteration = n;                                         // EX:81
    p->eps = std::numeric_limits<double>::epsilon() * 1e2;        // EX:58
    p->full_orthogonalize = 0;                                    // EX:63
    p->orth_mode = LL_ORTH_CGS_DGKS;
    p->initial_vector_size = 200;                                 // EX:71
  });
}

int ll_lanczos_run_d(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals, double* eigvecs,
                     int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,
                     ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
    lanczos_run<double>(ctx, op, *p, eigvals, eigvecs, n_found, iter_counts, iter_cap, alpha_out, beta_out, stats);
  });
}
int ll_lanczos_run_z(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals, void* eigvecs,
                     int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,
                     ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
    lanczos_run<zc>(ctx, op, *p, eigvals, (zc*)eigvecs, n_found, iter_counts, iter_cap, alpha_out, beta_out, stats);
  });
}
extern "C++" {
namespace {
template <typename T>
void run_iteration_impl(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot, int64_t n_orth,
                        const void* orth, double* eigvals, void* eigvecs, int64_t* n_found, int64_t* itern,
                        double* alpha_out, double* beta_out, ll_run_stats* stats) {
  LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
  ll_lanczos_params q = *p;
  q.num_eigs = 1;  // unused by the single-pass mode; keep the range check of the common driver happy
  const IterationSpec<T> spec{nroot, n_orth, (const T*)orth};
  int64_t count = 0;
  lanczos_run<T>(ctx, op, q, eigvals, (T*)eigvecs, n_found, &count, 1, alpha_out, beta_out, stats, &spec);
  if (itern) *itern = count;
}
}  // namespace
}  // extern "C++"
int ll_lanczos_run_iteration_d(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const double* orth, double* eigvals, double* eigvecs, int64_t* n_found,
                               int64_t* itern, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] {
    run_iteration_impl<double>(ctx, op, p, nroot, n_orth, orth, eigvals, eigvecs, n_found, itern, alpha_out, beta_out, stats);
  });
}
int ll_lanczos_run_iteration_z(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const void* orth, double* eigvals, void* eigvecs, int64_t* n_found,
                               int64_t* itern, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] {
    run_iteration_impl<zc>(ctx, op, p, nroot, n_orth, orth, eigvals, eigvecs, n_found, itern, alpha_out, beta_out, stats);
  });
}
int ll_expo_run_d(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const double* input,
                  double* output, int64_t* itern, ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && itern, "null argument");
    expo_run<double>(ctx, op, *p, a, input, output, itern, stats);
  });
}
int ll_expo_run_z(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                  const void* input, void* output, int64_t* itern, ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && itern, "null argument");
    expo_run<zc>(ctx, op, *p, std::complex<double>(a_re, a_im), (const zc*)input, (zc*)output, itern, stats);
  });
}
int ll_expo_taylor_run_d(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const double* input,
                         double* output, int64_t* nterms) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && nterms, "null argument");
    taylor_run<double>(ctx, op, *p, a, input, output, nterms);
  });
}
int ll_expo_taylor_run_z(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                         const void* input, void* output, int64_t* nterms) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && nterms, "null argument");
    taylor_run<zc>(ctx, op, *p, std::complex<double>(a_re, a_im), (const zc*)input, (zc*)output, nterms);
  });
}

// ---------------------------------------------------------------- float storage types: _s (float), _c (complex float)
// Mechanical twins of the _z entry points above (scalars stay double; data pointers are float / re,im float pairs).
int ll_op_create_csr_c(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                       const void* va, ll_operator** out) {
  return guarded([&] { create_csr<cf>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(false), out); });
}
int ll_op_create_csr_s(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                       const float* va, ll_operator** out) {
  return guarded([&] { create_csr<float>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(false), out); });
}
int ll_op_create_csr_dev_c(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const void* va, ll_operator** out) {
  return guarded([&] { create_csr<cf>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(true), out); });
}
int ll_op_create_csr_dev_s(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,
                           const float* va, ll_operator** out) {
  return guarded([&] { create_csr<float>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(true), out); });
}
int ll_op_create_coo_c(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols,
                       const void* vals, ll_operator** out) {
  return guarded([&] { create_coo<cf>(ctx, n, nnz, rows, cols, vals, out); });
}
int ll_op_create_coo_s(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols,
                       const float* vals, ll_operator** out) {
  return guarded([&] { create_coo<float>(ctx, n, nnz, rows, cols, vals, out); });
}
int ll_op_create_dense_s(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const float* a, ll_operator** out) {
  return guarded([&] { create_dense<float>(ctx, nr, nc, rb, a, out); });
}
int ll_op_create_stencil_s(ll_context* ctx, const ll_stencil_desc* desc, int64_t rb, int64_t nl, const double* onsite,
                           ll_operator** out) {
  return guarded([&] { create_stencil<float>(ctx, desc, rb, nl, onsite, out); });
}
int ll_op_create_dense_c(ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const void* a, ll_operator** out) {
  return guarded([&] { create_dense<cf>(ctx, nr, nc, rb, a, out); });
}
int ll_op_create_stencil_c(ll_context* ctx, const ll_stencil_desc* desc, int64_t rb, int64_t nl, const double* onsite,
                           ll_operator** out) {
  return guarded([&] { create_stencil<cf>(ctx, desc, rb, nl, onsite, out); });
}
int ll_op_create_host_c(ll_context* ctx, int64_t n, ll_host_mv_mul_z fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<cf>(ctx, n, fn, nullptr, user, out); });
}
int ll_op_create_host_s(ll_context* ctx, int64_t n, ll_host_mv_mul_s fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<float>(ctx, n, reinterpret_cast<ll_host_mv_mul_z>(fn), nullptr, user, out); });
}
int ll_op_create_device_c(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<cf>(ctx, n, nullptr, fn, user, out); });
}
int ll_op_create_device_s(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out) {
  return guarded([&] { create_cb<float>(ctx, n, nullptr, fn, user, out); });
}
int ll_spmv_c(ll_context* ctx, ll_operator* op, const void* x, void* y, double offset, double* dot) {
  return guarded([&] { spmv_impl<cf>(ctx, op, (const cf*)x, (cf*)y, offset, dot); });
}
int ll_spmv_s(ll_context* ctx, ll_operator* op, const float* x, float* y, double offset, double* dot) {
  return guarded([&] { spmv_impl<float>(ctx, op, (const float*)x, (float*)y, offset, dot); });
}
int ll_dot_c(ll_context* ctx, int64_t n, const void* a, const void* b, double* out) {
  return guarded([&] { dot_impl<cf>(ctx, n, (const cf*)a, (const cf*)b, out); });
}
int ll_dot_s(ll_context* ctx, int64_t n, const float* a, const float* b, double* out) {
  return guarded([&] { dot_impl<float>(ctx, n, (const float*)a, (const float*)b, out); });
}
int ll_nrm2_c(ll_context* ctx, int64_t n, const void* v, double* out) {
  return guarded([&] { nrm2_impl<cf>(ctx, n, (const cf*)v, out); });
}
int ll_nrm2_s(ll_context* ctx, int64_t n, const float* v, double* out) {
  return guarded([&] { nrm2_impl<float>(ctx, n, (const float*)v, out); });
}
int ll_scal_c(ll_context* ctx, int64_t n, double a, void* v) {
  return guarded([&] {
    use(ctx);
    launch_scale<cf>(n, (cf*)v, a, nullptr, ctx->stream);
  });
}
int ll_scal_s(ll_context* ctx, int64_t n, double a, float* v) {
  return guarded([&] {
    use(ctx);
    launch_scale<float>(n, (float*)v, a, nullptr, ctx->stream);
  });
}
int ll_normalize_c(ll_context* ctx, int64_t n, void* v, double* norm_out) {
  return guarded([&] { normalize_impl<cf>(ctx, n, (cf*)v, norm_out); });
}
int ll_normalize_s(ll_context* ctx, int64_t n, float* v, double* norm_out) {
  return guarded([&] { normalize_impl<float>(ctx, n, (float*)v, norm_out); });
}
int ll_three_term_c(ll_context* ctx, int64_t n, void* w, const void* up, const void* uc, double beta, double alpha) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(w && uc, "null vector");
    launch_three_term<cf>(n, (cf*)w, (const cf*)up, (const cf*)uc, beta, alpha, ctx->stream);
  });
}
int ll_three_term_s(ll_context* ctx, int64_t n, float* w, const float* up, const float* uc, double beta, double alpha) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(w && uc, "null vector");
    launch_three_term<float>(n, (float*)w, (const float*)up, (const float*)uc, beta, alpha, ctx->stream);
  });
}
int ll_orth_block_c(ll_context* ctx, int64_t n, int64_t nb, const void* basis, int64_t ld, void* w, int mode,
                    double* norm_out, double* h_out) {
  return guarded([&] { orth_impl<cf>(ctx, n, nb, (const cf*)basis, ld, (cf*)w, mode, norm_out, h_out); });
}
int ll_orth_block_s(ll_context* ctx, int64_t n, int64_t nb, const float* basis, int64_t ld, float* w, int mode,
                    double* norm_out, double* h_out) {
  return guarded([&] { orth_impl<float>(ctx, n, nb, (const float*)basis, ld, (float*)w, mode, norm_out, h_out); });
}
int ll_gemv_basis_c(ll_context* ctx, int64_t n, int64_t m, const void* basis, int64_t ld, int64_t nout,
                    const double* coeff, void* out, int64_t ld_out) {
  return guarded([&] {  // coefficients arrive as doubles (re,im pairs) like every scalar of the _s/_c API and stay double
    gemv_impl<cf, zc>(ctx, n, m, (const cf*)basis, ld, nout, (const zc*)coeff, (cf*)out, ld_out);
  });
}
int ll_gemv_basis_s(ll_context* ctx, int64_t n, int64_t m, const float* basis, int64_t ld, int64_t nout,
                    const double* coeff, float* out, int64_t ld_out) {
  return guarded([&] { gemv_impl<float, double>(ctx, n, m, (const float*)basis, ld, nout, coeff, (float*)out, ld_out); });
}
int ll_lanczos_run_c(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals, void* eigvecs,
                     int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,
                     ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
    lanczos_run<cf>(ctx, op, *p, eigvals, (cf*)eigvecs, n_found, iter_counts, iter_cap, alpha_out, beta_out, stats);
  });
}
int ll_lanczos_run_s(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals, float* eigvecs,
                     int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,
                     ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
    lanczos_run<float>(ctx, op, *p, eigvals, (float*)eigvecs, n_found, iter_counts, iter_cap, alpha_out, beta_out, stats);
  });
}
int ll_lanczos_run_iteration_s(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const float* orth, double* eigvals, float* eigvecs, int64_t* n_found,
                               int64_t* itern, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] {
    run_iteration_impl<float>(ctx, op, p, nroot, n_orth, orth, eigvals, eigvecs, n_found, itern, alpha_out, beta_out, stats);
  });
}
int ll_lanczos_run_iteration_c(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const void* orth, double* eigvals, void* eigvecs, int64_t* n_found,
                               int64_t* itern, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  return guarded([&] {
    run_iteration_impl<cf>(ctx, op, p, nroot, n_orth, orth, eigvals, eigvecs, n_found, itern, alpha_out, beta_out, stats);
  });
}
int ll_expo_run_c(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                  const void* input, void* output, int64_t* itern, ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && itern, "null argument");
    expo_run<cf>(ctx, op, *p, std::complex<double>(a_re, a_im), (const cf*)input, (cf*)output, itern, stats);
  });
}
int ll_expo_taylor_run_c(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                         const void* input, void* output, int64_t* nterms) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && nterms, "null argument");
    taylor_run<cf>(ctx, op, *p, std::complex<double>(a_re, a_im), (const cf*)input, (cf*)output, nterms);
  });
}
int ll_expo_run_s(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const float* input,
                  float* output, int64_t* itern, ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && itern, "null argument");
    expo_run<float>(ctx, op, *p, a, input, output, itern, stats);
  });
}
int ll_expo_taylor_run_s(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const float* input,
                         float* output, int64_t* nterms) {
  return guarded([&] {
    LL_REQUIRE(ctx && p && input && output && nterms, "null argument");
    taylor_run<float>(ctx, op, *p, a, input, output, nterms);
  });
}

}  // extern "C"
