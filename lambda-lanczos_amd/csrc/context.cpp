// Everything that is about ll_context: the last-error text, the tuning-key parser, the workspace members, and the entry
// points that create, time, connect and fill a context (ll_ctx_*, ll_timer_*, ll_bandwidth_probe, ll_comm_*, ll_partition,
// the memory helpers).  The operator, primitive and whole-loop entry points: capi.cpp.
#include <algorithm>
#include <cstdlib>
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
      {"pauli_symmetric_block_bits", &Tuning::pauli_symmetric_block_bits},
      {"pauli_torus_block_bits", &Tuning::pauli_torus_block_bits},
      {"pauli_block_expand_block_bits", &Tuning::pauli_block_expand_block_bits},
      {"pauli_block_project_block_bits", &Tuning::pauli_block_project_block_bits},
      {"pauli_rdm_tile_bits", &Tuning::pauli_rdm_tile_bits}, {"pauli_rdm_block_bits", &Tuning::pauli_rdm_block_bits}};
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
  else if (key == "block_gs") t.block_gs = e ? d.block_gs : to_flag(v);
  else if (key == "block_gs_max") {
    const long long m = e ? d.block_gs_max : to_ll(v);
    if (m != 4 && m != 8) return false;  // (ll_ctx_set_tuning: LL_ERR_INVALID)
    t.block_gs_max = (int)m;
  } else if (key == "pb_diag") t.pb_diag = e ? d.pb_diag : to_flag(v);
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
  else if (key == "pauli_rdm_tiled_kc") t.pauli_rdm_tiled_kc = e ? d.pauli_rdm_tiled_kc : (int)std::max<long long>(0, std::min<long long>(1 << 20, to_ll(v)));
  else if (key == "pauli_rdm_tiled_ksplit") t.pauli_rdm_tiled_ksplit = e ? d.pauli_rdm_tiled_ksplit : (int)std::max<long long>(0, std::min<long long>(1 << 20, to_ll(v)));
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
  else if (key == "test_workspace_fill") t.test_workspace_fill = e ? -1 : (int)std::max<long long>(0, std::min<long long>(255, to_ll(v)));
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
void ll_context::test_fill(void* p, size_t bytes) {
  // on the context's stream, then waited for: the buffer may be used first on the exchange stream
  LL_HIP(hipMemsetAsync(p, tune.test_workspace_fill, bytes, stream));
  LL_HIP(hipStreamSynchronize(stream));
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
}  // extern "C"
