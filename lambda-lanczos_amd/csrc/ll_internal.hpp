// Internal declarations shared by the HIP kernels, the host drivers and the C ABI.
// Not installed; the public surface is include/lanczos_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#if defined(__HIPCC__)
#include <hip/hip_ext.h>  // hipExtLaunchKernelGGL (device-code translation units only: the host-only sanitizer builds use g++)
#endif

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lanczos_hip.h"
#include "../../include/lanczos_hip_transport.h"
#include "scalar_types.hpp"
#include "spmv_plan.hpp"  // GatherPlan, PbColMap, kPbLdsCap: the host-side planning of the PB and tiled images

#if defined(__HIPCC__)
// A launch whose completion IS an event: hipExtLaunchKernelGGL hangs the event on the kernel's own dispatch packet; hipEventRecord
// behind the launch is a marker packet of its own between two dependent kernels (config 5: 5.9 -> 4.5 us in front of the next kernel,
// 16.5 k -> 16.9 k it/s; n = 1e5: + 1.4 %; same-box A/B through the key event_in_launch).
#define LL_LAUNCH_STOP(stop, kernel, grid, block, lds, s, ...)                                      \
  do {                                                                                              \
    if (stop) hipExtLaunchKernelGGL(kernel, grid, block, lds, s, nullptr, stop, 0, __VA_ARGS__);    \
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, __VA_ARGS__);                              \
  } while (0)
#endif

namespace ll {

// ---------------------------------------------------------------- scalar types: scalar_types.hpp
// The floating-point element types of device buffers (what the test hook test_workspace_fill fills; never an index type).
template <typename T>
inline constexpr bool is_float_elem_v = std::is_same_v<T, double> || std::is_same_v<T, float> || std::is_same_v<T, zc> || std::is_same_v<T, cf>;

// ---------------------------------------------------------------- errors
void set_error(const std::string& msg);
struct Failure {
  int code;
};

#define LL_HIP(expr)                                                                                         \
  do {                                                                                                       \
    hipError_t e_ = (expr);                                                                                  \
    if (e_ != hipSuccess) {                                                                                  \
      ::ll::set_error(std::string(#expr) + " failed: " + hipGetErrorString(e_) + " (" + __FILE__ + ":" +     \
                      std::to_string(__LINE__) + ")");                                                       \
      throw ::ll::Failure{LL_ERR_HIP};                                                                       \
    }                                                                                                        \
  } while (0)

#define LL_REQUIRE(cond, msg)                                                      \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      ::ll::set_error(std::string("invalid argument: ") + (msg));                  \
      throw ::ll::Failure{LL_ERR_INVALID};                                         \
    }                                                                              \
  } while (0)

// exception -> status: the body of every extern "C" entry point (capi.cpp, context.cpp) runs inside it
template <typename F> int guarded(F&& f) {
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

// ---------------------------------------------------------------- owned device memory
// The one owner of a library allocation: freed (Free: hipFree, or hipHostFree for pinned host memory) when reset, replaced or
// destroyed; moved, never copied.  A BORROWED handle (the caller's arrays of ll_op_create_csr_dev_*) is forgotten instead
// of freed and holds no bytes of the library's.
template <typename T, hipError_t (*Free)(void*) = hipFree> class DevArray {
 public:
  DevArray() = default;
  explicit DevArray(T* p, bool owned = true) : p_(p), owned_(owned) {}
  static DevArray borrow(T* p) { return DevArray(p, false); }
  DevArray(DevArray&& o) noexcept : p_(o.p_), owned_(o.owned_) { o.p_ = nullptr; }
  // typed -> untyped, like T* -> void* (images keep their arrays of the storage type T as void)
  template <typename U, typename V = T, typename = std::enable_if_t<std::is_void_v<V> && !std::is_void_v<U>>>
  DevArray(DevArray<U, Free>&& o) noexcept : owned_(o.owned()) { p_ = o.release(); }
  DevArray& operator=(DevArray&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      owned_ = o.owned_;
      o.p_ = nullptr;
    }
    return *this;
  }
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  ~DevArray() { reset(); }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  bool owned() const { return owned_; }
  void reset() noexcept { (void)free_now(); }
  // reset, with the status of the free (the growth path of the workspace reports it)
  hipError_t free_now() noexcept {
    const hipError_t e = p_ != nullptr && owned_ ? Free((void*)p_) : hipSuccess;
    p_ = nullptr;
    return e;
  }
  T* release() noexcept {  // the caller takes the allocation over
    T* p = p_;
    p_ = nullptr;
    return p;
  }
  // size of the owned allocation (0: none, or borrowed)
  int64_t bytes() const {
    if (p_ == nullptr || !owned_) return 0;
    size_t b = 0;
    LL_HIP(hipMemPtrGetInfo((void*)p_, &b));
    return (int64_t)b;
  }

 private:
  T* p_ = nullptr;
  bool owned_ = true;
};
template <typename T> using HostArray = DevArray<T, hipHostFree>;

// A workspace buffer that only grows (ll_context::ensure_*); cap counts elements of T (bytes for void).
template <typename T, hipError_t (*Free)(void*) = hipFree> struct Workspace {
  DevArray<T, Free> buf;
  size_t cap = 0;
  T* get() const { return buf.get(); }
};

// ---------------------------------------------------------------- launch geometry
constexpr int kBlock = 256;          // threads per workgroup (4 waves of 64)
constexpr int kCUs = 256;            // MI355X
constexpr int kXcds = 8;
constexpr int kMaxGrid = kCUs * 8;   // persistent grids: at most 8 workgroups per CU (multiple of 8 XCDs)
constexpr int kMaxSpmvGrid = kCUs * 16;  // CSR-stream SpMV with 16-byte values (its partial dot products: d_alpha_partials)
constexpr int kSpmvTileNnz = 1024;   // nonzeros staged through LDS per SpMV tile
constexpr int kXmaxParts = 512;      // maxima of |x| the pre-pass of the tiled and one-triangle kernels leaves (one per workgroup)
constexpr int kMaxSegs = 26;         // basis segments (slabs) per multi-dot / multi-axpy launch: 5000 vectors in slabs of 200

// f() once per device and mask (a static of the caller: one bit per device).  The opt-in to > 64 KiB of dynamic LDS is per device
// and per kernel symbol: pb_opt_in is what f calls for each kernel of a family (spmv_pb.hip, spmv_tiled.hip).
template <typename F> void once_per_device(std::atomic<unsigned long long>& mask, F&& f) {
  int dev = 0;
  LL_HIP(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (mask.load(std::memory_order_acquire) & bit) return;
  f();
  mask.fetch_or(bit, std::memory_order_release);
}
template <typename K> void pb_opt_in(K kernel) {
  LL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPbLdsCap));
}

// A run of basis vectors stored with a common leading dimension: vector j at base + j*ld.
template <typename T> struct BasisSegs {
  const T* base[kMaxSegs];
  int count[kMaxSegs];
  int nseg;
  long long ld;
  int total() const {  // vectors in all runs
    int t = 0;
    for (int i = 0; i < nseg; ++i) t += count[i];
    return t;
  }
};

// The three squared norms of one Gram-Schmidt call, as device scalars:
//   c0 = ||w||^2 before pass 1, c1 = after pass 1, c2 = after pass 2 (valid only if the second pass ran).
// Device-predicated form (the one-call primitive ll_orth_block_*): the second pass runs iff force2 (LL_ORTH_CGS2) or
// c1 < c0/2 (DGKS "twice is enough" test) and every consumer (scale, next three-term update, host read-back) applies
// the same selection.  The whole-loop drivers enqueue pass 1 only (c2 aliases c1, force2 = 0) and take the DGKS
// decision on the host from the published (c0, c1) one iteration later (engine.hpp, Engine::second_pass).
struct NormRefs {
  const double* c0;
  const double* c1;
  const double* c2;
  int force2;
  double thr = 0.5;  // DGKS threshold of the device-predicated form (LL_DGKS_THRESHOLD overrides it, like on the host)
};

// ---------------------------------------------------------------- communicator (RCCL, lazily loaded; or an external transport)
struct Comm;
Comm* comm_attach(const struct ::ll_transport* t, int rank, int nranks);
Comm* comm_create(const void* id128, int rank, int nranks, int device);
void comm_destroy(Comm*);
std::string comm_transport_name(const Comm*);  // "none" | "rccl" | "plugin:<path>" | "attached"
void comm_unique_id(void* id128);
void comm_allgather(Comm*, const void* send, void* recv, size_t bytes, hipStream_t s);
void comm_allreduce_sum(Comm*, double* buf, size_t n_doubles, hipStream_t s);
// Ring halo exchange: `bytes` from send_prev go to rank `prev` (they become its recv_next) and `bytes` from send_next
// go to rank `next` (its recv_prev); the matching messages arrive in recv_prev / recv_next.  prev / next = -1: no such
// neighbour (open boundary).  prev == next (two ranks on a ring) and prev == next == own rank are legal.
void comm_halo_exchange(Comm*, const void* send_prev, void* recv_prev, int prev, const void* send_next, void* recv_next,
                        int next, size_t bytes, hipStream_t s);

}  // namespace ll

// ---------------------------------------------------------------- tuning: environment switches and per-context settings
// The USER-FACING LL_* switches are read from the environment ONCE, when a context is created
// (ll_ctx_create*), into the context; operators copy what shapes their image when THEY are created.  Nothing on a launch path
// calls getenv.  ll_ctx_reload_env() reads them again.  Every other field below — geometry overrides, forced code paths, the
// hooks of the test suite — is NOT read from the environment: it is set per context through ll_ctx_set_tuning(ctx, key, value)
// (context.cpp tuning_apply holds the one parser; the comments below name the key).
namespace ll {
struct Tuning {
  // --- operator creation
  int spmv_kernel = -1;            // LL_SPMV_KERNEL = csr | pb | tiled: that LL_SPMV_* kernel; anything else -1 (auto: time the candidates, keep the fastest)
  bool keep_both = false;          // LL_SPMV_KEEP_BOTH=1: keep the image that lost the timing (ll_op_select_spmv A/B)
  int pb_phase2 = 4;               // LL_PB_PHASE2 = fixed (4, default) | ordered (1) | atomic (0); with the accuracy request: operators.cpp image_forms
  int pb_block = 0;                // key pb_block = n: rows AND columns per block (0: automatic); tests force ragged blocks
  int pb_row_block = 0;            // keys pb_row_block = n / pb_col_block = n: one of the two only
  int pb_col_block = 0;
  int pair_max_stored = 0;         // key pair_max_stored = n: the pair form hands over to the one-sweep form beyond n stored vectors (test hook; by itself at 4 992 real / 2 492 complex)
  int pair_split_vecs = 0;         // key pair_split = n: at most n stored vectors per launch of the pair sweep (test hook: split sweeps on small problems)
  int pb_threads1 = 0;             // key pb_threads1 = 256 | 512 | 1024: lanes per workgroup of PB phase 1 (0: automatic — 512 for the thin column blocks of a sharded image, 1024 on one GPU); read at creation
  int pb_pad = 0;                  // key pb_pad = 4 | 16: entries every segment of the PB image is padded to (0: automatic — 4 sharded, 16 on one GPU); read at creation
  int pb_placements = 8;           // LL_PB_PLACEMENTS: arena placements timed at creation (1: keep the first; LL_PB_PLACEMENT_TRACE=1 prints every draw); operators.cpp
  bool pb_xpre = true;             // key pb_xpre = 0: phase 2 of the PB SpMV loads x_i in its epilogue (A/B of the early request)
  bool pb_diag = true;             // LL_PB_DIAG=0: the diagonal entries travel through the PB streams like every other entry (A/B)
  int gather_chunks = 0;           // LL_GATHER_CHUNKS: pieces of the all-gather (0: 4 on two ranks, 2 on more)
  bool spmv_tile_balance = true;   // key spmv_tile_balance = 0: CSR-stream tiles always hold up to 1024 nonzeros (operators.cpp build_tiles)
  bool csr_split = true;           // LL_CSR_SPLIT=0: sharded CSR-stream / dense operators gather first, then multiply (round-3 form)
  bool comm_overlap = true;        // LL_COMM_OVERLAP=0: exchange and compute on one stream (serial A/B reference)
  // --- the loops
  bool tridiag_thread = true;      // LL_TRIDIAG_THREAD=0: host Ritz step inline instead of on the helper thread
  int tridiag_lag = 3;             // LL_TRIDIAG_LAG: fixed verdict lag of sharded runs (lanczos_loop.hpp)
  double dgks_threshold = 0.5;     // LL_DGKS_THRESHOLD: second Gram-Schmidt pass when ||w'||^2 < thr * ||w||^2
  bool sharded_norm_measured = false;  // LL_SHARDED_NORM=measured: all-reduce the post-pass norm instead of deriving it
  int64_t slab_bytes = (int64_t)4 << 30;       // LL_SLAB_BYTES: cap of one Krylov-basis slab
  int64_t blas_small_bytes = (int64_t)4 << 20;  // LL_BLAS_SMALL_BYTES: vectors below this use the small-vector kernels
  bool fuse_launches = true;       // LL_FUSE_LAUNCHES=0: separate fold / publish kernels (A/B of the launch fusion)
  long long lagged_min_bytes = -1; // key lagged_min_bytes: shortest vector of the one-sweep form (-1 = default)
  int lagged_pieces = 0;           // key lagged_pieces: strip geometry of the one-sweep kernel (0 = by length)
  bool lagged_gs = true;           // LL_FUSE_LAUNCHES=1: fused folds but the two-sweep Gram-Schmidt form; 2 (default): one sweep
  bool event_in_launch = true;     // key event_in_launch = 0: iteration events as marker packets behind the publishing kernel (A/B)
  bool ritz_tail = true;           // key ritz_tail = 0: a pair pending at the end of a pass is completed by sweeps of its own instead of entering the Ritz GEMV through its raw vectors (A/B)
  int sweep_pipeline = 1;          // key sweep_pipeline: 1 (default) the software-pipelined pair sweep on streaming vectors (> ~9 MiB), 0 never (A/B: same bits), 2 on every length (parity tests on small cases)
  bool block_gs = true;            // key block_gs = 0: never the raw-basis block form (up to eight iterations per sweep); the pair form where it applies (A/B)
  int block_gs_max = 8;            // key block_gs_max = 4|8: the largest block the form takes (eight: real double only); 4: never eight iterations per sweep (the form as it was before blocks of eight, A/B)
  bool pair_gs = true;             // LL_PAIR_GS=0: never two iterations per sweep (the one-sweep form throughout; A/B and parity hunts)
  // --- test hooks (not for users)
  bool force_rp64 = false;         // key force_rp64 = 1: 64-bit row offsets on small matrices
  bool tl_xcd_order = true;        // key tl_xcd = 0: row blocks of the tiled kernel in launch order instead of one contiguous eighth per XCD (A/B)
  bool tl_walk_modulo = true;      // key tl_walk = 0: a row block's tiles in ascending column order instead of by column index modulo the longest tile list (A/B; read at creation)
  bool tl_force = false;           // key tl_force = 1: build the tiled image even for matrices that are not eligible (parity tests on small cases)
  bool pb_test_all_remote = false; // key pb_test_all_remote = 1: own columns are read from the gathered buffer too
  int tridiag_test_jitter_us = 0;  // key tridiag_test_jitter_us = n: random delay of every helper-thread verdict
  int pauli_tile_bits = -1;        // key pauli_tile_bits = b: the Pauli-string kernel's tiles hold 2^b states (-1: what fills kPauliTileBytes of LDS); tests force remote groups on small problems
  int pauli_momentum_block_bits = -1;  // key pauli_momentum_block_bits = b: the same for the momentum-block kernel (-1: kPauliMomentumBlockBits)
  int pauli_momentum_full_block_bits = -1;  // key pauli_momentum_full_block_bits = b: the same for the full-space momentum-block kernel (-1: kPauliMomentumFullBlockBits)
  int pauli_torus_block_bits = -1;  // key pauli_torus_block_bits = b: the same for the torus kernel (-1: kPauliTorusBlockBits)
  int pauli_symmetric_block_bits = -1;  // key pauli_symmetric_block_bits = b: the same for the momentum / reflection / spin-inversion kernel (-1: kPauliSymmetricBlockBits)
  int pauli_block_expand_block_bits = -1;   // key pauli_block_expand_block_bits = b: ll_pauli_block_expand's workgroups take blocks of 2^b output indices (-1: kPauliBlockExpandBlockBits, pauli_block_embed_plan.hpp); tests force several trips of the grid-stride loop
  int pauli_block_project_block_bits = -1;  // key pauli_block_project_block_bits = b: ll_pauli_block_project's take blocks of 2^b representatives (-1: kPauliBlockProjectBlockBits)
  int pauli_sector_block_bits = -1;  // key pauli_sector_block_bits = b: the S_z-sector kernel's workgroups take blocks of 2^b indices (-1: kPauliSectorBlockBits); tests force many blocks on small sectors
  int pauli_rdm_tile_bits = -1;    // key pauli_rdm_tile_bits = t: the reduced-density-matrix kernel's tiles hold 2^t states (-1: what fills kPauliTileBytes of LDS with the super-tile); tests force subsystem sites above the tile on small problems
  int pauli_rdm_block_bits = -1;   // key pauli_rdm_block_bits = b: its sector form gathers 2^b environment configurations per LDS batch (-1: what fills kPauliTileBytes)
  int pauli_rdm_tiled_kc = 0;      // key pauli_rdm_tiled_kc = KC: the tiled reduced-density-matrix kernel stages KC environment configurations per K-step (0: 16; a power of two in 4 .. 16, others are lowered to one); tests force many K-steps on small problems
  int pauli_rdm_tiled_ksplit = 0;  // key pauli_rdm_tiled_ksplit = s: its K-steps are dealt to s slices (0: what fills twice the CUs within 64 MiB of partials; lowered to a power of two that the K-steps allow)
  int test_workspace_fill = -1;    // key test_workspace_fill = 0..255: every device buffer of floating-point element type that the context hands out (dev_alloc<T>, Krylov slabs, DevBuf<T>; new or from the slab cache) is filled with that byte before use (-1, unset: not touched); tests poison the workspace with it
  bool stencil_vec = true;         // key stencil_vec = 0: scalar lattice kernel on shapes the vector kernel would take
  double stall_trace_ms = -1.0;    // key stall_trace = ms: print where a whole-loop call longer than this spent its time
  std::string iter_trace;          // LL_ITER_TRACE=path: the eigen-solver loop appends one line per collected iteration
                                   // (pass k alpha beta^2 c0 c1 second-pass) and one per stop verdict — for parity hunts
  bool pb_placement_trace = false; // LL_PB_PLACEMENT_TRACE=1: print every placement draw of the PB image (operators.cpp)
};
// context.cpp: defaults <- the user-facing environment switches <- the context's overrides (ll_ctx_set_tuning), in that order
Tuning read_tuning(const std::map<std::string, std::string>* overrides);
bool tuning_apply(Tuning& t, const std::string& key, const std::string& value);  // false: unknown key

}  // namespace ll

// ---------------------------------------------------------------- context
struct ll_context {
  ll::Tuning tune;
  std::map<std::string, std::string> tuning_overrides;  // ll_ctx_set_tuning: key -> value, applied on top of the environment
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  ll::Comm* comm = nullptr;
  int rank = 0, nranks = 1;
  int ranks_seen = 0;                 // result of the rank self-check at ll_comm_init (== nranks when healthy)
  // Exchange overlap: the all-gather of a sharded vector is issued on comm_stream, chunk by chunk, so that
  // SpMV work on the rank's own columns runs under it and every chunk's remote-column work starts when that chunk
  // has arrived.  LL_COMM_OVERLAP=0 issues everything on `stream` instead (serial reference path for A/B tests).
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_x_ready = nullptr;
  hipEvent_t ev_chunk[ll::kMaxGatherChunks] = {};
  hipEvent_t ev_xmax = nullptr;  // the tiled kernel's max|x| all-gather, in front of the vector's chunks
  bool profiling = false;
  hipEvent_t t0 = nullptr, t1 = nullptr;  // ll_timer_*

  // workspace, all sized lazily
  ll::Workspace<double> partials;        // [grid][ncols] block partial sums
  ll::Workspace<double> alpha_partials;  // the operator kernels' partial <x, Ax> (kept apart: the multi-dot that follows
                                         // may fold them itself while it writes its own partials)
  ll::Workspace<double> h;               // reduced projection coefficients / small scalars
  ll::DevArray<double> scal;             // 64 doubles of device scalars (ring slots, flags)
  ll::DevArray<double> norm_partials;    // kMaxGrid norm partials of the folding multi-axpy (must not alias partials)
  ll::Workspace<double, hipHostFree> pinned;  // pinned host mirror for scalar read-back
  ll::Workspace<void> coeff;             // coefficient upload area for gemv_basis
  std::vector<hipEvent_t> timer_events;  // PhaseTimer's ring of timing events (profiling mode), created once and kept between runs
  std::vector<std::pair<void*, size_t>> slab_cache;  // Krylov-basis slabs kept between runs (ptr, bytes), oldest first
  // Return a buffer to the cache.  The cache is bounded (kSlabCacheMaxEntries): a long-lived context that solves problems
  // of many different shapes frees its oldest cached buffers instead of accumulating them (hipFree synchronises the device;
  // it happens only when the bound is hit, never inside a loop).
  static constexpr size_t kSlabCacheMaxEntries = 64;
  void cache_put(void* p, size_t bytes);
  ll::Workspace<void> xfull;      // all-gather target (sharded runs)
  ll::Workspace<void> halo;       // received halos of the lattice operator: [from prev | from next]

  // hipMalloc that makes room first when the device is full: the cached Krylov slabs of earlier runs are returned to
  // the device and the allocation is retried; LL_ERR_ALLOC (with the size in the message) if it still fails.
  void dev_malloc(void** out, size_t bytes, const char* what);
  // Test hook test_workspace_fill: fill a buffer that is about to be handed out (context.cpp; call it only when the key is set).
  void test_fill(void* p, size_t bytes);
  template <typename T> void test_fill_if_set(T* p, size_t count) {
    if constexpr (ll::is_float_elem_v<T>)
      if (tune.test_workspace_fill >= 0) test_fill((void*)p, count * sizeof(T));
  }
  // the same, owned: count elements of T (bytes for void)
  template <typename T> ll::DevArray<T> dev_alloc(size_t count, const char* what) {
    void* p = nullptr;
    if constexpr (std::is_void_v<T>) dev_malloc(&p, count, what);
    else {
      dev_malloc(&p, count * sizeof(T), what);
      test_fill_if_set((T*)p, count);
    }
    return ll::DevArray<T>((T*)p);
  }
  // Grow a device workspace buffer to at least `count` elements: geometrically (1.5 x + 64) or to exactly `count`.
  template <typename T> T* ensure(ll::Workspace<T>& w, size_t count, bool geometric, const char* what);
  void ensure_partials(size_t doubles) { ensure(partials, doubles, true, "partial sums"); }
  void ensure_alpha_partials(size_t doubles) { ensure(alpha_partials, doubles, true, "alpha partial sums"); }
  void ensure_h(size_t doubles) { ensure(h, doubles, true, "projection coefficients"); }
  void ensure_coeff(size_t bytes) { ensure(coeff, bytes, true, "Ritz coefficients"); }
  void ensure_xfull(size_t bytes) { ensure(xfull, bytes, false, "gathered vector"); }
  void ensure_halo(size_t bytes) { ensure(halo, bytes, false, "halo buffer"); }
  void ensure_pinned(size_t doubles);
  // device-time stamps of the exchange steps (only with profiling on): (start, end) pairs on the stream they ran on
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_gather, ev_allreduce;
  void drain_comm_events(double* gather_s, double* allreduce_s);  // adds the elapsed device seconds, frees the events
  ll::Workspace<void, hipHostFree> stage;  // pinned host staging buffer for n-sized transfers (start vector, Ritz vectors)
  void* ensure_stage(size_t bytes);
  ll::Workspace<void, hipHostFree> cb;     // pinned [in | out] buffers of the host-callback operator
  hipEvent_t ev_cb = nullptr;    // recorded after the upload of a callback result
  hipEvent_t stop_next = nullptr;  // set by the loop in front of an operator application whose kernel publishes an iteration's scalars: that
                                   // launch completes the event itself (LL_LAUNCH_STOP) and clears the field; still set afterwards = not taken
  void* ensure_cb_stage(size_t bytes);
  void sync();
};
namespace ll {
// The launcher of a publishing kernel takes the event over (and hangs it on its launch: LL_LAUNCH_STOP); null: none pending.
inline hipEvent_t take_stop(ll_context* ctx) {
  hipEvent_t stop = ctx->stop_next;
  ctx->stop_next = nullptr;
  return stop;
}
}  // namespace ll

// ---------------------------------------------------------------- SpMV images of an operator
// Every image owns its arrays and knows its own geometry; a builder fills a local image and moves it into the operator
// only when it succeeds, and dropping an image is resetting it.
namespace ll {
// CSR: row offsets (int32, or int64 when rp64), columns, values and the ntiles + 1 row boundaries of the SpMV tiles
struct CsrImage {
  DevArray<void> row_ptr;
  DevArray<int32_t> col;
  DevArray<void> val;
  DevArray<int32_t> tiles;
  int ntiles = 0;
  bool rp64 = false;
  int64_t device_bytes() const { return row_ptr.bytes() + col.bytes() + val.bytes() + tiles.bytes(); }
};
// f(RP{}) with RP = the type of an image's row offsets: the one place that turns CsrImage::rp64 into a template argument
template <typename F> void for_row_ptr_type(bool rp64, F&& f) {
  if (rp64) f(int64_t{});
  else f(int32_t{});
}

// Propagation-blocked image (kernels: spmv_pb.hip; built by spmv_image_build.hip from the plan of spmv_plan.hpp).
// Column-block table order: the blocks over the rank's OWN columns first (their x
// slice is the local shard, no exchange needed), then, gather chunk by gather chunk, the blocks over the other ranks' columns
// (x slice in the gathered buffer).  One phase-1 launch per range, so own-column work runs under the all-gather.
struct PbImage {
  int ncb = 0, nrb = 0, cb_cols = 0, rb_rows = 0;  // cb_cols = longest column block (LDS sizing)
  DevArray<int64_t> segq;        // [ncb][nrb+1] entry offsets of the segments in column-block order
  DevArray<int64_t> segdest;     // [ncb][nrb]   position of each segment in row-block order
  DevArray<int64_t> rptr;        // [nrb+1]      entry offsets of the row blocks in row-block order
  DevArray<int64_t> xoff;        // [ncb]        element offset of the block's x slice in ITS source buffer
  DevArray<int32_t> ncols;       // [ncb]        columns of the block
  DevArray<void> arena;          // the one allocation that holds the four big streams below (interior pointers)
  size_t arena_bytes = 0, arena_static_bytes = 0;  // its size; the part in front of the product buffer
  void* val = nullptr;           // values, column-block order (the start of the arena)
  uint16_t* col = nullptr;       // local column, column-block order
  uint16_t* row = nullptr;       // local row, row-block order
  void* prod = nullptr;          // product buffer P (nnz elements of T), row-block order
  DevArray<int16_t> rexp;        // LL_PB_PHASE2=fixed: exponent of every local row's absolute sum
  DevArray<double> blockmax;     // LL_PB_PHASE2=fixed: max |x| per column block, left by phase 1
  DevArray<void> diag;           // a_ii of every local row (T): the diagonal is kept outside the streams (pb_diag_kernel)
  int64_t entries = 0;           // padded entry count of the image
  int phase2 = 4;                // form of phase 2 (ll::LL_PB_FIXED / _ORDERED / _ATOMIC): set when the image is built,
                                 // changed by ll_op_set_accuracy (both forms read the same image)
  int threads1 = 1024;           // lanes per workgroup of phase 1 (1024; 512 for the thin column blocks of a sharded image)
  bool xpre = true;              // fixed-point phase 2 requests the epilogue's x_i before its stream (key pb_xpre)
  int own_count = 0;             // table range [0, own_count)
  int chunk_first[kMaxGatherChunks] = {0};  // remote blocks of gather chunk c: [first, first + count)
  int chunk_count[kMaxGatherChunks] = {0};
  GatherPlan gather;             // how a sharded vector is all-gathered when the PB kernels are selected
  bool present() const { return (bool)arena; }
  // point the interior pointers at a copy of the arena that starts at `base` (placement search, operators.cpp)
  void rebase(void* base) {
    const ptrdiff_t d = (char*)base - (char*)val;
    val = base;
    col = (uint16_t*)((char*)col + d);
    row = (uint16_t*)((char*)row + d);
    prod = (char*)prod + d;
  }
  int64_t device_bytes() const {
    return segq.bytes() + segdest.bytes() + rptr.bytes() + xoff.bytes() + ncols.bytes() + arena.bytes() + rexp.bytes() +
           blockmax.bytes() + diag.bytes();
  }
};

// 2-D tiled image (kernel: spmv_tiled.hip; built by spmv_image_build.hip): row blocks with the y slice in LDS, each walking its
// non-empty column tiles of 16 KiB of x;
// entries = value (pre-scaled by the row's exponent) + packed 16-bit local column / row
struct TiledImage {
  int nrb = 0, rb_rows = 0, ncb = 0;
  int n_interior = 0;            // sharded: row blocks whose tiles are all own-column tiles (first in rbmap; they run under the all-gather)
  DevArray<int32_t> rbmap;       // sharded: [nrb] row blocks in launch order (interior first); null on one GPU
  int64_t entries = 0, tiles = 0;
  DevArray<int32_t> first;       // [nrb + 1]     first tile of each row block in the tile list
  DevArray<int32_t> col;         // [ntiles]      column tile index
  DevArray<int64_t> quad;        // [ntiles + 1]  first quad (4 entries) of each tile in the entry stream
  DevArray<void> val;            // values in tile order
  DevArray<uint32_t> idx;        // local column | local row << 16
  DevArray<int16_t> rexp;        // exponent of every row's absolute sum (the scale the values were divided by)
  DevArray<double> xmax;         // maxima of |x| the kernel folds (per workgroup of the pre-pass; sharded: one per rank), then scratch of the own-shard pre-pass
  bool ordered = false;          // the tiled kernel sums in floating point, the waves in turn (component-wise class) instead of in fixed point
  bool present() const { return nrb > 0; }
  int64_t device_bytes() const {
    return rbmap.bytes() + first.bytes() + col.bytes() + quad.bytes() + val.bytes() + idx.bytes() + rexp.bytes() + xmax.bytes();
  }
};

// One-triangle image of a symmetric / Hermitian matrix (spmv_sym.hip): one stream per row block of every stored entry with an
// end in the block; an entry whose two ends lie in different blocks is in both streams
struct SymImage {
  int nrb = 0, rb_rows = 0, halo = 0;  // row blocks, rows per block, half-bandwidth max |i - j| of the triangle
  DevArray<int64_t> qptr;        // [nrb + 1] first quad (4 entries) of each row block's stream
  DevArray<void> val;            // values as stored (T)
  DevArray<uint32_t> idx;        // window index of the entry's row | of its column << 16 (0xffffffff: padding)
  DevArray<int16_t> rexp;        // exponent of every row's absolute sum over the FULL row of A
  DevArray<double> xmax;         // kXmaxParts maxima of |x| (pre-pass)
  DevArray<void> diag;           // [n] the first diagonal entry of every row, kept outside the streams (0: none)
  // entries whose other end lies outside the row block's x window (the few beyond the halo, e.g. the wrap-around corners of a
  // periodic band): one product each, x read from memory — destination local row | 1 << 31 for the mirrored product, source row
  DevArray<int64_t> fptr;        // [nrb + 1] first far entry of each row block
  DevArray<void> fval;
  DevArray<uint32_t> fdst;
  DevArray<int32_t> fsrc;
  bool present() const { return nrb > 0; }
  int64_t device_bytes() const {
    return qptr.bytes() + val.bytes() + idx.bytes() + rexp.bytes() + xmax.bytes() + diag.bytes() + fptr.bytes() + fval.bytes() +
           fdst.bytes() + fsrc.bytes();
  }
};

// Sum of Pauli strings (pauli.hip): the terms grouped by x mask — groups by ascending mask, the terms of a group in the
// caller's order; that order is the kernel's order of summation
constexpr int kPauliMaxSites = 30;               // 2^30 states: the local indices of the library are signed 32-bit (n_local < 2^31 - 1)
constexpr int kPauliTileBytes = 32 << 10;        // LDS tile of one workgroup (four workgroups per CU beside their reduction scratch)
constexpr int kPauliMaxTileBytes = 64 << 10;     // largest tile pauli_tile_bits may ask for
// the term tables on the device: what every image below holds and every kernel's term loop reads
struct PauliTermImage {
  int ngroups = 0;
  int64_t nterms = 0;
  DevArray<uint32_t> gx;         // [ngroups]      x mask of the group
  DevArray<int32_t> gptr;        // [ngroups + 1]  first term of each group
  DevArray<uint32_t> tz;         // [nterms]       z mask
  DevArray<double> tc;           // [nterms] (real types) / [nterms][2] (complex: re, im): c_t i^nY_t
  int64_t device_bytes() const { return gx.bytes() + gptr.bytes() + tz.bytes() + tc.bytes(); }
};
struct PauliImage {
  int n_sites = 0;
  PauliTermImage terms;
  int64_t device_bytes() const { return terms.device_bytes(); }
};
// The same sum on one S_z sector (pauli_sector.hip): the term tables above, the sector's states in ascending order, and the
// two tables that give a state's index back: rank(s) = lo_rank[s & (2^h - 1)] + hi_rank[s >> h].  With the set bits of s at
// p_1 < ... < p_m the index is sum_k C(p_k, k); the low bits' share depends on them alone, the others' on them alone too,
// since popcount(low bits) = n_down - popcount(the others).
constexpr int kPauliSectorBlockBits = 10;        // indices of a workgroup's block: one pass of kBlock lanes with four states each
constexpr int kPauliSectorMaxSupport = 20;       // creation's conservation check enumerates 2^|support| assignments per group
struct PauliSectorImage {
  int n_sites = 0, n_down = 0, h = 0;
  int64_t dim = 0;               // dim = C(n_sites, n_down)
  PauliTermImage terms;
  DevArray<uint32_t> states;     // [dim]                 the states of the sector, ascending
  DevArray<uint32_t> lo_rank;    // [2^h]
  DevArray<uint32_t> hi_rank;    // [2^(n_sites - h)]
  int64_t device_bytes() const { return terms.device_bytes() + states.bytes() + lo_rank.bytes() + hi_rank.bytes(); }
};
// One momentum block of an S_z sector of a ring (pauli_momentum.hip): the basis is the representatives (smallest member of an orbit
// under the one-site shift T) whose period R satisfies m R = 0 (mod n_sites), ascending.  orbit[rank(s)] packs, for every state s
// of the sector, (index of its representative in the block << 5 | l) with s = T^l representative; kPauliOrbitExcluded marks a
// state whose orbit the block excludes.  ratio[Ra * 32 + Rb] = sqrt(Ra / Rb); phase[l] = e^(-2 pi i m l / n_sites) as (re, im).
constexpr uint32_t kPauliOrbitExcluded = 0xffffffffu;
constexpr int kPauliMomentumBlockBits = 8;       // indices of a workgroup's block: one state per lane (blocks are L times fewer than the sector's: 2^8 fills the device sooner)
constexpr int kPauliOrbitShiftBits = 5;          // l < n_sites <= 30 < 2^5; index of the representative < 2^27
struct PauliMomentumImage {
  int n_sites = 0, n_down = 0, momentum = 0, h = 0;
  int nshort = 0;                // distinct primes q of n_sites: a state s has a short orbit iff T^(n_sites / q) s = s for one of them;
  int short_shift[3] = {0, 0, 0};  // the shifts n_sites / q (0 entries when the block holds no short orbit: nothing to test)
  int64_t dim = 0, sector_dim = 0;   // dim = D_m, sector_dim = C(n_sites, n_down)
  PauliTermImage terms;
  DevArray<uint32_t> reps;       // [dim]                 the representatives, ascending
  DevArray<uint8_t> orbit_len;   // [dim]                 their orbit lengths R
  DevArray<uint32_t> orbit;      // [sector_dim]          see above
  DevArray<uint32_t> lo_rank;    // [2^h]
  DevArray<uint32_t> hi_rank;    // [2^(n_sites - h)]
  DevArray<double> ratio;        // [32 * 32]
  DevArray<double> phase;        // [n_sites][2]
  int64_t device_bytes() const {
    return terms.device_bytes() + reps.bytes() + orbit_len.bytes() + orbit.bytes() + lo_rank.bytes() + hi_rank.bytes() +
           ratio.bytes() + phase.bytes();
  }
};
// An ascending list of representatives that a kernel searches (pauli_shared.hpp pauli_bucket_search): no table over the states.
// The kernel rotates a partner to its representative b in registers and finds b's number by a bounded binary search in reps[]
// inside one bucket of the top bits: start[q] = the number of representatives below q << prefix_shift,
// 2^(n_sites - prefix_shift) + 1 entries (about dim / 8 buckets: at most dim / 2 bytes); search_trips = the halvings the LARGEST
// bucket needs (measured at creation: representatives crowd at small integers), the uniform length of the kernel's search loop.
struct PauliRepImage {
  int prefix_shift = 0, search_trips = 0;
  int64_t max_bucket = 0;        // the most representatives under one prefix
  DevArray<uint32_t> reps;       // [dim]                 the representatives, ascending
  DevArray<uint8_t> orbit_len;   // [dim]                 their orbit lengths R
  DevArray<uint32_t> start;      // [2^(n_sites - prefix_shift) + 1]
  int64_t device_bytes() const { return reps.bytes() + orbit_len.bytes() + start.bytes(); }
};
// One block of a ring under momentum, reflection and spin inversion, of the full space or of one S_z sector: the image of both
// searched-basis kinds.  The basis is every representative (the smallest integer of its orbit under the group G generated by the
// shift, by the reflection if parity != 0 and by the global flip if inversion != 0) on whose stabiliser the character is 1 and,
// with n_down >= 0, whose popcount is n_down, ascending; orbit lengths R = |G| / |stabiliser|; phase[] as PauliMomentumImage.
// PAULI_SYMMETRIC (pauli_symmetric.hip): ratio[R_a * kPauliSymmetricRatioStride + c] = sqrt(R_a / (|G| / c)) for the stabiliser
// sizes c that divide |G| (R <= |G| <= 120); the kernel decides membership by comparing the entry it finds with the representative.
// PAULI_MOMENTUM_FULL (pauli_momentum_full.hip): the shift alone on the full space (n_down = -1, parity = inversion = 0, group_size
// = n_sites: every representative whose period R satisfies m R = 0 mod n_sites); ratio[] as PauliMomentumImage.
constexpr int kPauliMomentumFullBlockBits = 8;   // indices of a workgroup's block: one state per lane, as kPauliMomentumBlockBits
constexpr int kPauliSymmetricBlockBits = kPauliMomentumFullBlockBits;  // taken over from the full-momentum kernel, unmeasured
constexpr unsigned kPauliSymmetricRatioStride = 121;
// PAULI_TORUS (pauli_torus.hip): an Lx x Ly torus, site (x, y) = bit x + Lx y, n_sites = Lx Ly; G = the Lx Ly translations
// T_x^a T_y^b (code a + Lx b), parity = inversion = 0, group_size = n_sites; momentum = m_x, momentum_y = m_y;
// phase[code] = e^(-2 pi i (m_x a Ly + m_y b Lx) / (Lx Ly)) as (re, im); ratio[R_a * kPauliTorusRatioStride + c] as PAULI_SYMMETRIC
// (R <= |G| <= 30).  lx = ly = 0 for the two ring kinds.
constexpr int kPauliTorusBlockBits = kPauliSymmetricBlockBits;  // the symmetric kernel's: the same search form and as many images; unmeasured
constexpr unsigned kPauliTorusRatioStride = 32;
struct PauliBlockImage {
  int n_sites = 0, n_down = -1, momentum = 0, parity = 0, inversion = 0, group_size = 0;
  int lx = 0, ly = 0, momentum_y = 0;  // PAULI_TORUS only
  int64_t dim = 0;
  PauliTermImage terms;
  PauliRepImage basis;
  DevArray<double> ratio;        // [121 * 121] (PAULI_SYMMETRIC) / [32 * 32] (PAULI_MOMENTUM_FULL, PAULI_TORUS)
  DevArray<double> phase;        // [n_sites][2]
  int64_t device_bytes() const { return terms.device_bytes() + basis.device_bytes() + ratio.bytes() + phase.bytes(); }
};
}  // namespace ll

// ---------------------------------------------------------------- operator
struct ll_operator {
  enum Kind { CSR, HOST_CB, DEV_CB, DENSE, STENCIL, PAULI, PAULI_SECTOR, PAULI_MOMENTUM, PAULI_MOMENTUM_FULL, PAULI_SYMMETRIC, PAULI_TORUS } kind = CSR;
  bool is_complex = false;
  int elem_bytes = 8;  // sizeof(T): 4 float, 8 double / complex float, 16 complex double
  ll_context* ctx = nullptr;
  int64_t n = 0, n_local = 0, row_begin = 0, nnz = 0;
  int64_t n_shard = 0;  // padded shard length used by the all-gather (= n when not sharded)
  double inf_norm = -1.0;  // max absolute row sum of the local rows (-1: unknown)
  // CSR-stream image (op_kernels.hip launch_spmv).  Sharded contexts, CSR-stream selected: the same rows split by column ownership
  // (operators.cpp build_csr_split) — csr_own holds the entries over the rank's OWN columns (indices rebased to the local shard; their
  // product needs no exchange and runs under the all-gather), csr_rem the entries over the other ranks' columns (global indices
  // into the gathered vector).
  ll::CsrImage csr, csr_own, csr_rem;
  bool csr_split() const { return (bool)csr_own.row_ptr; }
  bool has_csr_stream() const { return csr.row_ptr && (csr.col || nnz == 0 || csr_split()); }
  int spmv_kind = 0;                 // LL_SPMV_*
  float tune_ms[3] = {-1.f, -1.f, -1.f};  // what the creation-time autotune measured per LL_SPMV_* kernel (-1: not timed)
  ll::PbImage pb;                    // propagation-blocked image (spmv_pb.hip pb_phase1 / pb_phase2)
  ll::TiledImage tl;                 // 2-D tiled image (spmv_tiled.hip; LL_SPMV_TILED)
  int64_t sym_stored = -1;           // entries of the triangle the operator was created from (ll_op_info); -1: full storage
  ll::SymImage sym;                  // one-triangle image (spmv_sym.hip; LL_SPMV_SYM, ll_op_create_csr_sym_*)
  // dense row-major block (kind DENSE): n_local x n values of T
  ll::DevArray<void> dense;
  // lattice operator (kind STENCIL)
  ll_stencil_desc st = {};
  int64_t st_stride[3] = {0, 0, 0};  // flattened-index stride of each dimension (last index fastest)
  int64_t st_halo = 0;               // sites of one hyperplane = reach of the operator in the flattened index
  ll::DevArray<void> onsite;         // n_local on-site terms in the real type of T (nullable)
  ll::PauliImage pauli;              // sum of Pauli strings (kind PAULI)
  ll::PauliSectorImage pauli_sector; // the same on one S_z sector (kind PAULI_SECTOR)
  ll::PauliMomentumImage pauli_momentum;  // one momentum block of an S_z sector of a ring (kind PAULI_MOMENTUM)
  ll::PauliBlockImage pauli_block;   // one symmetry block of a ring or a torus by a searched basis (kinds PAULI_MOMENTUM_FULL, PAULI_SYMMETRIC, PAULI_TORUS)
  static_assert(PAULI_SECTOR == PAULI + 1 && PAULI_MOMENTUM == PAULI + 2 && PAULI_MOMENTUM_FULL == PAULI + 3 &&
                    PAULI_SYMMETRIC == PAULI + 4 && PAULI_TORUS == PAULI + 5,
                "is_pauli: the six Pauli kinds are one range of Kind (a seventh goes inside it)");
  static bool is_pauli(int kind) { return kind >= PAULI && kind <= PAULI_TORUS; }
  bool is_pauli() const { return is_pauli(kind); }
  // device bytes the operator holds (the caller's borrowed arrays excluded)
  int64_t device_bytes() const {
    return csr.device_bytes() + csr_own.device_bytes() + csr_rem.device_bytes() + pb.device_bytes() + tl.device_bytes() +
           sym.device_bytes() + dense.bytes() + onsite.bytes() + pauli.device_bytes() +
           pauli_sector.device_bytes() + pauli_momentum.device_bytes() + pauli_block.device_bytes();
  }
  // callbacks
  ll_host_mv_mul_z host_fn = nullptr;  // every host callback is stored under the void* signature
  ll_dev_mv_mul dev_fn = nullptr;
  void* user = nullptr;
  ll_operator() = default;
  ll_operator(const ll_operator&) = delete;
  ll_operator& operator=(const ll_operator&) = delete;
  ~ll_operator();  // selects the device; the images free their arrays (context.cpp)
};

namespace ll {

// f(T{}) with T = the operator's storage type: the one place that turns is_complex / elem_bytes into a template argument
template <typename F> void for_storage_type(const ll_operator& op, F&& f) {
  const bool wide = op.elem_bytes == (op.is_complex ? (int)sizeof(zc) : (int)sizeof(double));
  if (op.is_complex && wide) f(zc{});
  else if (op.is_complex) f(cf{});
  else if (wide) f(double{});
  else f(float{});
}
// f(T{}) with T = the storage type a character names (the untyped primitives of capi.cpp)
template <typename F> void for_storage_char(int storage, F&& f) {
  switch (storage) {
    case 'd': f(double{}); break;
    case 'z': f(zc{}); break;
    case 's': f(float{}); break;
    case 'c': f(cf{}); break;
    default: LL_REQUIRE(false, "storage must be one of 'd', 'z', 's', 'c'");
  }
}
const char* operator_kind_name(int kind);  // "a CSR operator", ...: what a refusal calls an operator (operators.cpp)

// ---------------------------------------------------------------- operator construction (operators.cpp, pauli_operators.cpp)
// What the extern "C" entry points (capi.cpp) call.  create_csr takes resolved options: csr_options_default(false) for the plain
// entry points, csr_options_default(true) for the _dev_ ones, the caller's for the _opt_ ones.
void use(ll_context* ctx);  // null check, then the context's device (context.cpp)
template <typename T>  // the header of every operator: kind, storage type, context and the checked row range (operators.cpp)
std::unique_ptr<ll_operator> new_operator(ll_context* ctx, ll_operator::Kind kind, int64_t n, int64_t row_begin, int64_t n_local);
ll_csr_options csr_options_default(bool arrays_on_device);
template <typename T>
void create_csr(ll_context* ctx, int64_t nr, int64_t nc, int64_t row_begin, const int64_t* rp, const int32_t* ci, const void* va,
                const ll_csr_options& opt, ll_operator** out);
template <typename T>
void create_coo(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols, const void* vals,
                ll_operator** out);
template <typename T>  // opt nullable: the defaults
void create_csr_sym(ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const void* va,
                    const ll_csr_options* opt, ll_operator** out);
template <typename T> void create_dense(ll_context* ctx, int64_t nr, int64_t nc, int64_t row_begin, const void* a, ll_operator** out);
template <typename T>
void create_stencil(ll_context* ctx, const ll_stencil_desc* d, int64_t row_begin, int64_t n_local, const double* onsite,
                    ll_operator** out);
// n = 2^n_sites, single GPU; real types take terms with an even number of Y only
template <typename T>
void create_pauli(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out);
// n = C(n_sites, n_down): the same terms on the states with n_down set bits; refuses an H that does not conserve S_z
template <typename T>
void create_pauli_sector(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                         ll_operator** out);
// n = D_m: the block of momentum 2 pi m / n_sites of that sector, for an H that also commutes with the one-site shift of the ring;
// real types take m = 0 and m = n_sites / 2 only
template <typename T>
void create_pauli_momentum(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                           const ll_pauli_term* terms, ll_operator** out);
// n = D_m: the block of momentum 2 pi m / n_sites of ALL 2^n_sites states of a ring, for an H that commutes with the one-site shift
// (no S_z conservation asked: the transverse-field Ising ring, XYZ rings); real types take m = 0 and m = n_sites / 2 only
template <typename T>
void create_pauli_momentum_full(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out);
// n = D: the block (momentum, parity, inversion) of a ring — of all 2^n_sites states (n_down = -1) or of the sector n_down —
// for an H that commutes with the shift and with the reflection / the global flip where parity / inversion != 0
template <typename T>
void create_pauli_symmetric(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity, int32_t inversion,
                            int64_t n_terms, const ll_pauli_term* terms, ll_operator** out);
// n = D: the block (m_x, m_y) of an Lx x Ly torus (site (x, y) = bit x + Lx y) under its Lx Ly translations — of all 2^(Lx Ly)
// states (n_down = -1) or of the sector n_down — for an H that commutes with both one-site translations
template <typename T>
void create_pauli_torus(ll_context* ctx, int32_t lx, int32_t ly, int32_t n_down, int32_t mx, int32_t my, int64_t n_terms,
                        const ll_pauli_term* terms, ll_operator** out);
// a host callback (every one under the void* signature: same ABI, only the pointee types differ) or a device callback
template <typename T>
void create_cb(ll_context* ctx, int64_t n, ll_host_mv_mul_z host_fn, ll_dev_mv_mul dev_fn, void* user, ll_operator** out);
// ll_op_set_accuracy: the images of a CSR operator take the forms of the accuracy class; op_accuracy: the class of the kernel
// selected now (LL_ACCURACY_NORMWISE / _COMPONENTWISE).  Both follow operators.cpp image_forms.
void set_op_accuracy(ll_operator* op, int accuracy);
int op_accuracy(const ll_operator* op);

// ---------------------------------------------------------------- kernel launchers
// Operator kernels: op_kernels.hip (CSR-stream, column split, dense, lattice), spmv_pb.hip, spmv_tiled.hip, spmv_image_build.hip, spmv_sym.hip, pauli.hip, pauli_basis.hpp (through pauli_sector.hip, pauli_momentum.hip, pauli_momentum_full.hip, pauli_symmetric.hip, pauli_torus.hip), pauli_expect.hip, pauli_expect_block.hip, pauli_block_embed.hip, pauli_block_transfer.hip, pauli_rdm.hip, pauli_rdm_tiled.hip; everything
// from launch_reduce_cols down: kernels.hip, except the pair form (gs_pair.hip; launch_pair_sweep_small, pair_small_fits and
// launch_maxpy_folding: gs_small.hip) and the two-pass recurrence (launch_recur_*: recur.hip).
// All launchers enqueue on `s` and return immediately.

// Deferred normalisation (a8 folded into the next a1; single-GPU whole-loop drivers, operators that gather x themselves):
// the operator kernel is handed the UNNORMALISED vector w_k together with the `nparts` partial sums of ||w_k||^2.  Every
// workgroup folds them in the same fixed order, works with u_k = w_k / ||w_k|| (the operator is linear: the factor is
// applied to the row sums and to x_i), writes u_k to u_out (the basis slot: every later reader wants it normalised) and
// workgroup 0 stores ||w_k||^2 to *c1_out and iteration k's four scalars to the pinned host slot — the work of
// scale_publish_kernel without its launch and without its read of w.
template <typename T> struct ScaleIn {
  const double* partials = nullptr;  // null: x is already normalised (everything below is ignored)
  int nparts = 0;
  double* c1_out = nullptr;
  const double* alpha = nullptr;
  const double* c0 = nullptr;
  double* host = nullptr;
  T* u_out = nullptr;
};

// y = A x_full(cols) + offset * x_local ; dot_partials (nullable): one double per workgroup, Re<x_local, y>.
// Returns the number of partials written.
// part: 0 = the whole image (op.csr); 1 / 2 = the own-column / other-columns half of a column-split image (op.csr_own / csr_rem).
template <typename T>
int launch_spmv(const ll_operator& op, const T* x_full, const T* x_local, T* y, double offset, double* dot_partials,
                hipStream_t s, const ScaleIn<T>* sc = nullptr, int part = 0);
// build helpers of the column split (op_kernels.hip): own-column entries per row; scatter into the two halves
template <typename T> void launch_csr_count_own(const ll_operator& op, int32_t* own_cnt, hipStream_t s);
template <typename T> void launch_csr_split(const ll_operator& op, const CsrImage& own, const CsrImage& rem, hipStream_t s);
// Same contract, propagation-blocked kernels (op.spmv_kind == LL_SPMV_PB; spmv_pb.hip): phase 1 over the own-column
// blocks (x slices from x_own: the local shard readable up to the shard stride), then over every gather chunk's remote blocks (x slices from x_gathered, laid out
// per op.gather), then phase 2.  The pieces are exposed so that the sharded driver can run the own-column part under
// the all-gather and each chunk's part as soon as that chunk has arrived.
// xnorm2 (nullable device scalar): x is an UNNORMALISED vector w with ||w||^2 = *xnorm2; the kernels work with w / ||w||
// (lagged Gram-Schmidt, kernels.hip / gs_pair.hip).
template <typename T>
int launch_spmv_pb(const ll_operator& op, const T* x_gathered, const T* x_own, const T* x_local, T* y, double offset,
                   double* dot_partials, hipStream_t s, const double* xnorm2 = nullptr);
template <typename T>
void launch_pb_phase1(const ll_operator& op, int blk_first, int blk_count, const T* xsrc, hipStream_t s,
                      const double* xnorm2 = nullptr);
template <typename T>
int launch_pb_phase2(const ll_operator& op, const T* x_local, T* y, double offset, double* dot_partials, hipStream_t s,
                     const double* xnorm2 = nullptr);
// forms of PB phase 2 (Tuning::pb_phase2, PbImage::phase2)
constexpr int LL_PB_ATOMIC = 0, LL_PB_ORDERED = 1, LL_PB_FIXED = 4;
// Build the propagation-blocked image on the device from the operator's CSR arrays (spmv_image_build.hip), phase 2 in the form
// `phase2` (LL_PB_*,
// resolved by operators.cpp image_forms); false: shape not supported.
template <typename T> bool pb_build_device(ll_operator* op, int phase2);
// The 2-D tiled kernel for matrices with column locality (spmv_tiled.hip; its image: spmv_image_build.hip): same contract as
// launch_spmv on a single GPU
// (x = the whole vector); build returns false when the matrix is not eligible (too many column tiles per row block).
template <typename T> bool tl_build_device(ll_operator* op);
template <typename T>
int launch_spmv_tiled(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                      const double* xnorm2 = nullptr);
// Sharded form (engine.cpp): own-shard maximum, then the two launches (own-column row blocks under the all-gather, the rest behind it).
template <typename T> void launch_tl_xmax_local(const ll_operator& op, const T* x_own, hipStream_t s);
int tl_xmax_local_slot();
template <typename T>
int launch_spmv_tiled_pass(const ll_operator& op, int pass, const T* x, int64_t col0, int64_t col_end, const T* x_local, T* y,
                           double offset, double* dot_partials, hipStream_t s, const double* xnorm2, int n_xmax);
// Column range check + max absolute row sum of the local rows (sets op->inf_norm), on the device (spmv_image_build.hip).
template <typename T> void csr_check_device(ll_operator* op);
// maxima of |x| over n elements, one per workgroup, into parts [kXmaxParts]; returns how many were written (tl_xmax_kernel)
template <typename T> int launch_x_max(int64_t n, const T* x, double* parts, hipStream_t s);
// The one-triangle kernel (spmv_sym.hip).  sym_rows_for: rows per row block for a triangle of that half-bandwidth, 0 when
// the triangle is not eligible.  sym_build: the image from the HOST triangle into im (op->n, im.halo, im.rb_rows set; the row
// exponents are filled by the caller).  launch_spmv_sym: y = A x + offset x on a single GPU, same contract as launch_spmv.
template <typename T> int sym_rows_for(int64_t n, int64_t halo);
// the x window's halo for a triangle: the smallest h that leaves at most 1/16 of the entries with |i - j| > h (-1: none <= 32767)
int64_t sym_halo_for(const int64_t* rp, const int32_t* ci, int64_t n);
template <typename T> void sym_build(const ll_operator& op, SymImage& im, const int64_t* rp, const int32_t* ci, const T* va);
template <typename T>
int launch_spmv_sym(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                    const double* xnorm2);
// Same contract for the dense row block (op.kind == DENSE).
template <typename T>
int launch_dense_mv(const ll_operator& op, const T* x_full, const T* x_local, T* y, double offset, double* dot_partials,
                    hipStream_t s, const ScaleIn<T>* sc = nullptr, int part = 0);
// Lattice operator (op.kind == STENCIL): site li of the shard reads x at li + off, |off| <= op.st_halo, from
// halo_lo[st_halo + j] for j < 0, x_local[j] for 0 <= j < n_local and halo_hi[j - n_local] beyond.
template <typename T>
int launch_stencil(const ll_operator& op, const T* x_local, const T* halo_lo, const T* halo_hi, T* y, double offset,
                   double* dot_partials, hipStream_t s, const ScaleIn<T>* sc = nullptr);
// Sum of Pauli strings (op.kind == PAULI; pauli.hip): x = the whole vector, same contract as launch_stencil on one GPU.
template <typename T>
int launch_pauli(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                 const ScaleIn<T>* sc = nullptr);
// The five indexed-basis kernels (pauli_basis.hpp) take 2^b indices per workgroup block: the context's key if set (at most
// 2^30), else the kernel's default
inline int pauli_block_bits(const ll_operator& op, int ll::Tuning::*key, int dflt) {
  const int forced = op.ctx ? op.ctx->tune.*key : -1;
  return forced >= 0 ? std::min(forced, 30) : dflt;
}
// The same on one S_z sector (op.kind == PAULI_SECTOR; pauli_sector.hip): x, y hold C(n_sites, n_down) elements.
template <typename T>
int launch_pauli_sector(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                        const ScaleIn<T>* sc = nullptr);
// One momentum block of that sector (op.kind == PAULI_MOMENTUM; pauli_momentum.hip): x, y hold D_m elements.
template <typename T>
int launch_pauli_momentum(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                          const ScaleIn<T>* sc = nullptr);
// One momentum block of the full space (op.kind == PAULI_MOMENTUM_FULL; pauli_momentum_full.hip): x, y hold D_m elements.
template <typename T>
int launch_pauli_momentum_full(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                               const ScaleIn<T>* sc = nullptr);
// One momentum / reflection / spin-inversion block (op.kind == PAULI_SYMMETRIC; pauli_symmetric.hip): x, y hold D elements.
template <typename T>
int launch_pauli_symmetric(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                           const ScaleIn<T>* sc = nullptr);
// One translation block of a torus (op.kind == PAULI_TORUS; pauli_torus.hip): x, y hold D elements.
template <typename T>
int launch_pauli_torus(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                       const ScaleIn<T>* sc = nullptr);
template <typename T>  // whichever of the six op.kind names (pauli_operators.cpp): what Engine::apply calls
int launch_pauli_op(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s, const ScaleIn<T>* sc);
// string j of a list of terms or observables (`what`): its masks below n_sites, its coefficient finite (pauli_operators.cpp)
void check_pauli_string(const char* what, int64_t j, const ll_pauli_term& q, int n_sites);
// The host side that the four measuring entry points below share: pauli_measure.hpp.
// ll_pauli_expect (pauli_expect.hip; planned by pauli_expect_plan.hpp): every check, then the sweeps on the operator's storage type
void pauli_expect(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs, const void* psi, double* out,
                  int64_t* sweeps_out);
// ll_pauli_expect_block (pauli_expect_block.hip; planned by pauli_expect_block_plan.hpp): the same on a ring's symmetry block,
// psi = the coefficients on the block's representatives
void pauli_expect_block(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs, const void* psi, double* out,
                        int64_t* sweeps_out);
// ll_pauli_block_expand / ll_pauli_block_project (pauli_block_embed.hip; planned by pauli_block_embed_plan.hpp): every check, then
// Psi = B c (expand) or c = B^H Psi (project) on the operators' storage type
void pauli_block_embed(ll_context* ctx, const ll_operator* block, const ll_operator* target, bool expand, const void* in, void* out);
// ll_pauli_block_transfer (pauli_block_transfer.hip; planned by pauli_block_transfer_plan.hpp): every check, then
// out = B_t^H (sum of the strings) B_s c on the operators' storage type
void pauli_block_transfer(ll_context* ctx, const ll_operator* source, const ll_operator* target, int64_t n_terms,
                          const ll_pauli_term* terms, const void* c, void* out, double* norm2_out);
// ll_pauli_rdm (pauli_rdm.hip; planned by pauli_rdm_plan.hpp): every check, then the one sweep on the operator's storage type
void pauli_rdm(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites, const void* psi, double* out,
               int64_t* sweeps_out);
// ll_pauli_rdm_tiled (pauli_rdm_tiled.hip; planned by pauli_rdm_tiled_plan.hpp): every check, then the rank-K update on the f64
// matrix cores and its finishing kernel on the operator's storage type; out is host or device memory
void pauli_rdm_tiled(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites, const void* psi, void* out,
                     int64_t* sweeps_out);
// y += offset * x ; partials of Re<x,y> (post-pass for callback operators).
template <typename T>
int launch_offset_dot(int64_t n, const T* x, T* y, double offset, double* dot_partials, hipStream_t s);

// out[j] = sum_b partials[b*ncols + j], j < ncols (deterministic tree, fixed order).
// last_out (nullable) redirects the last column.
void launch_reduce_cols(const double* partials, int nparts, int ncols, double* out, double* last_out, hipStream_t s);
void launch_copy_scalar(double* dst, const double* src, hipStream_t s);
// reduce_one + publish in one launch: out[0] = sum(partials); host[0..4) = {*alpha, sum, *c0, sum} (alpha, c0 nullable)
void launch_reduce_publish(const double* partials, int nparts, double* out, const double* alpha, const double* c0,
                           double* host_mapped, hipStream_t s);
void launch_set_scalar(double* dst, double value, hipStream_t s);
// *c1 = max(0, *c0 - sum_i h[i]^2)  (one workgroup, fixed order)
// c0 = *c0_src (||w||^2 before the pass, from the all-reduced buffer), c1 = max(c0 - sum_i h_i^2, 0); host_mapped (nullable):
// the iteration's four scalars (alpha, c1, c0, c1) go to the pinned host slot in the same launch.
void launch_derive_norm(const double* c0_src, const double* h, int count, double* c0, double* c1, const double* alpha,
                        double* host_mapped, hipStream_t s);

// Multi-dot with optional fused three-term update.
//   if (three_term) w = w - beta*u_prev - alpha*u_cur   (u_prev nullable; alpha = *alpha_dev; beta = beta_from(norms_prev))
//   partial columns: for every basis vector j (segments in order): <u_j, w> (1 or 2 doubles), then ||w||^2.
// pred (nullable): the launch is a no-op unless the second pass is due according to *pred.
// Returns grid size (= number of partial rows); ncols = reals*nb + 1.
template <typename T> struct ThreeTerm {
  const T* u_prev;      // nullable (k == 1)
  const T* u_cur;       // nullable => no three-term update
  const double* alpha;  // device scalar
  NormRefs prev;        // norms of the previous iteration: beta = sqrt(final norm^2)
  // Deferred alpha (single-GPU whole-loop drivers): alpha has NOT been folded yet; every workgroup of the multi-dot
  // sums the operator kernel's `alpha_nparts` partials itself (same fixed order everywhere) and workgroup 0 stores the
  // result to alpha_out for the consumers that follow (publish).  One launch per iteration less.
  const double* alpha_partials = nullptr;
  int alpha_nparts = 0;
  double* alpha_out = nullptr;
  static ThreeTerm none() { return ThreeTerm{nullptr, nullptr, nullptr, NormRefs{nullptr, nullptr, nullptr, 0}}; }  // no update
};
// small_bytes: vectors shorter than this many bytes take the small-vector geometry (Tuning::blas_small_bytes).
template <typename T>
int launch_mdot(int64_t n, T* w, const BasisSegs<T>& segs, const ThreeTerm<T>& tt, const NormRefs* pred,
                double* partials, int64_t small_bytes, hipStream_t s);
// Lagged block Gram-Schmidt (kernels.hip, lagged_kernel): one sweep that applies the previous iteration's update to
// r -> u_out, forms w = w - alpha r/beta - beta u_prev minus the compensation of the perturbed operator input, and all
// coefficients <u_j, .> (segments, then u_out) + ||w||^2.  Partial columns: reals * (nb + 1) + 1 per workgroup.
// tt.u_cur is ignored.  g: reals * nb coefficients of r, t: reals * (nb + 1) + 1 values, both from launch_lagged_fold.
// LDS: 4 ncols doubles (the waves' partial columns; g and t are read through the scalar cache), 160 KB per workgroup:
// reals * nb <= kLaggedMaxCols.  Streaming geometry only.
constexpr int kLaggedMaxCols = 5000;
template <typename T> struct Lagged {
  const T* r;
  T* u_out;
  const double* g;
  const double* t;
  const double* beta2;
};
// pieces: 0 = pick the strip geometry from the vector length (16-byte pieces per lane: 4 from kLaggedFullStrips 16 KiB
// strips up, else 2); 2 / 4 force it (key lagged_pieces).
constexpr int kLaggedFullStrips = 200;
template <typename T>
int launch_lagged(int64_t n, T* w, const BasisSegs<T>& segs, const Lagged<T>& lg, const ThreeTerm<T>& tt, double* partials,
                  int pieces, int64_t small_limit, hipStream_t s);  // vectors below small_limit bytes: lagged_small_kernel
// The pair form (two iterations per sweep; gs_pair.hip; tools/pair_gs_model.py is the executable specification).
// Streaming geometry only; 2 * reals * K + 5 * reals + 1 <= kLaggedMaxCols columns per workgroup (K stored columns).
constexpr double kPairGate = 1e-8;  // largest relative coefficient the pair form accepts in double precision (second-order terms
                                    // stay below 1e-16; float storage: 2e-4, lanczos_loop.hpp)
// The guard of the block form's blocks of EIGHT.  Fresh rounding along a converged Ritz direction grows by r = (theta - alpha) / beta
// per operator application and is measured only by the next sweep: a block of m reaches about eps r^(m-1), so a gate value g
// published by blocks of four predicts g (g / eps)^(4/3) at eight — a factor 10 under kPairGate for g <= 1.6e-13, IF r is stationary.
// While a Ritz value is still converging it is not (an outlier: 5e-16, 1e-13, 1e-12 in the first three blocks of four), so eight are
// taken only after kBlock8Quiet consecutive collected iterations published a gate value <= kBlock8Tau; kBlock8Tau lies between what
// blocks of four publish without a converged outlier (<= 2.3e-14) and with one (1e-13 .. 5e-12).  tools/block_gs_model.py
// (run_guarded; TAU, QUIET) and profiles/block8_model.txt: no block of eight in 24 outlier runs, where ONE block <= 1.6e-13 admitted
// one in every run.  kPairGate stays the safety net behind it.
constexpr double kBlock8Tau = 5e-14;
constexpr int kBlock8Quiet = 12;
template <typename T>
int launch_pair_three_term(int64_t n, T* y, const T* x, const T* p, double* e, const double* e_partials, int e_nparts,
                           const double* cx2, const double* cp2, double* partials, bool colmajor,
                           hipStream_t s);  // y <- y - (e / sqrt(cx2)) x - sqrt(cx2 / cp2) p; partials [grid][1 + reals] (colmajor:
                                            // [1 + reals][grid]): |y|^2, <p, y>; e_partials (nullable): the operator kernel's
                                            // partial sums of e, folded here into *e
// P Lanczos vectors behind L locked eigenvectors (eigenvalues lambda[0..L) of the operator the loop applies): K = L + P columns
void launch_pair_predict(int P, int L, int reals, const double* g1, const double* g2, const double* rho1sq, const double* rho2sq,
                         const double* gam, double* n3sq, const double* d13_partials, int d13_nparts, const double* e1, double* e2,
                         const double* e2_partials, int e2_nparts, const double* hist_alpha, const double* hist_beta,
                         const double* lambda, double* p3, double* p4, hipStream_t s);
// r4 holds y2 = A (r3 / |r3|) on entry; the sweep forms r4 = y2 - (e2 / |r3|) r3 - (|r3| / rho2) r2 on the fly
// One workgroup keeps 4 x (2 reals Pl + 5 reals + 1) columns in LDS: a sweep over more stored vectors than that is split into
// launches over consecutive groups of them (same results bit for bit, gs_pair.hip); part4: scratch n-vector for the hand-over
// (touched only when there is more than one group).
constexpr int kPairFirst = 1, kPairLast = 2;
template <typename T> constexpr int pair_sweep_max_vecs() {
  return (kLaggedMaxCols - 5 * scalar_traits<T>::reals - 1) / (2 * scalar_traits<T>::reals);
}
template <typename T>
int launch_pair_sweep(int64_t n, const std::vector<BasisSegs<T>>& groups, int P, const T* r1, const T* r2, const T* r3, T* r4,
                      T* uP_out, T* uQ_out, T* part4, const double* g1, const double* g2, const double* gam, const double* p4,
                      const double* rho1sq, const double* rho2sq, const double* e2, const double* n3sq, double* partials, int pieces,
                      hipStream_t s, const T* const* vtab = nullptr,  // vtab (device; column c -> pointer of stored vector c): the software-
                      bool force_pipeline = false);                   // pipelined kernel on streaming vectors (force: on any); null: the reference kernel
// The same sweep in the small-vector geometry (pair_small_kernel: four waves per 1 KiB strip split the stored vectors; vectors of
// 320 KiB .. 1 MiB).  One launch over ONE group of segments; false when the columns do not fit one workgroup's LDS (nothing launched).
template <typename T>
bool launch_pair_sweep_small(int64_t n, const BasisSegs<T>& segs, int P, const T* r1, const T* r2, const T* r3, T* r4, T* uP_out,
                             T* uQ_out, const double* g1, const double* g2, const double* gam, const double* p4, const double* rho1sq,
                             const double* rho2sq, const double* e2, const double* n3sq, double* partials, int* grid_out,
                             hipStream_t s);
template <typename T> bool pair_small_fits(int P);  // P stored columns fit the small-geometry sweep's LDS
// tab[start + i] = base + i * ld, i < count (the pointer table of the pipelined sweeps; one launch per slab)
template <typename T> void launch_fill_ptrs(const T** tab, int start, int count, const T* base, int64_t ld, hipStream_t s);
void launch_pair_fold(const double* m, int P, int L, int reals, const double* lambda, const double* p4, const double* g2, const double* gam,
                      const double* rho2sq, const double* n3sq, const double* e1, const double* e2, double* rec3, double* rec4,
                      double* nxt, double* hist_alpha, double* hist_beta, double* scratch, double* host_a, double* host_b,
                      double* gate_a, double* gate_b, hipStream_t s, hipEvent_t stop = nullptr);
// The block form (up to eight iterations per sweep over a RAW basis; gs_block.hip; tools/block_gs_model.py is the executable
// specification).  Streaming geometry, double and complex double, no locked columns.  The form keeps reals * K^2 / 2 coefficients
// for a pass of K vectors and leaving it costs one multi-axpy per raw vector, so it is bounded by a vector count and only taken by
// passes that cannot outgrow it (LoopState::enqueue_block).
constexpr int kBlockMaxVecs = 1024;
constexpr int kBlockMaxM = 8;  // iterations per block at most (eight: real double only, behind the guard, kBlock8Tau)
struct BlockScalars {
  const double* e[kBlockMaxM];    // <x, A x> of the block's operator applications
  const double* nsq[kBlockMaxM];  // |b_s|^2 of the raw three-term vectors
};
struct BlockHost {
  double* slot[kBlockMaxM];  // host slots of the block's iterations (alpha, beta^2, ||w||^2 before, after)
  double* gate[kBlockMaxM];  // ... and their gate values
};
template <typename T> struct BlockVecs {
  T* b[kBlockMaxM];  // the new vectors in their basis slots; the sweep rewrites the last two
  T* part[2];  // hand-over vectors of a split sweep (touched only when there is more than one launch)
};
template <typename T> constexpr int block_sweep_max_vecs(int m) {  // stored vectors per launch: 4 x (m reals Wl + Gram) doubles of LDS
  return (kLaggedMaxCols - (scalar_traits<T>::reals * m * (m - 1) / 2 + m)) / (m * scalar_traits<T>::reals);
}
void launch_block_enter(int k, int reals, const double* g, const double* c1, double* rho2, double* cpk, hipStream_t s);
void launch_block_predict(int k, int m, int reals, const BlockScalars& sc, const double* rho2, const double* cpk, double* hist_alpha,
                          const double* hist_beta, double* dk, double* p, int pstride, double* prA, double* prB, hipStream_t s);
// vtab: column c -> pointer of stored vector c (W of them); per_launch: at most that many stored vectors per launch
template <typename T>
int launch_block_sweep(int64_t n, const T* const* vtab, int W, int m, const BlockVecs<T>& bv, const double* prA, const double* prB,
                       double* partials, int pieces, int per_launch, hipStream_t s);
void launch_block_fold(const double* cols, int k, int m, int reals, const BlockScalars& sc, const double* p, int pstride, double* rho2,
                       double* cpk, double* hist_alpha, double* hist_beta, double* raw0, double* raw1, const BlockHost& host, hipStream_t s,
                       hipEvent_t stop = nullptr);
// Fold of a lagged iteration (K = L + k columns: L locked eigenvectors with eigenvalues lambda[0..L), then k Lanczos
// vectors; m: reals * K folded columns, *c0 = ||w||^2, copied to *c0_out): compensated coefficients in place,
// *c1 = *c0 - |g|^2, t_out (reals * (K + 1) + 1) for the next sweep, alpha / beta appended to hist_*[k - 1], *alpha
// replaced by its corrected value, the iteration's four scalars published.  prev_* = nullptr after a clean iteration.
void launch_lagged_fold(double* m, int K, int L, int reals, double* t_out, const double* c0, double* c0_out, double* c1,
                        double* alpha, const double* prev_g, const double* prev_t, const double* prev_c1,
                        double* hist_alpha, double* hist_beta, const double* lambda, double* host_mapped, hipStream_t s, hipEvent_t stop = nullptr);
// w -= sum_j h_j u_j over the segments; partial ||w||^2 per workgroup. h: reals*nb doubles on the device.
template <typename T>
int launch_maxpy(int64_t n, T* w, const BasisSegs<T>& segs, const double* h, const NormRefs* pred, double* partials,
                 int64_t small_bytes, hipStream_t s);
// The same update with the fold of the multi-dot's partials ([mparts][reals*nb + 1]) done inside the kernel (small-vector
// geometry, small grids): h_out receives the coefficients, *c0_out (nullable) the ||w||^2 column; `partials` (the norm
// partials of the result) must not alias mdot_partials.  false: not applicable, nothing was launched.
template <typename T>
bool launch_maxpy_folding(int64_t n, T* w, const BasisSegs<T>& segs, const double* mdot_partials, int mparts, double* h_out,
                          double* c0_out, double* partials, int64_t small_bytes, int* grid_out, hipStream_t s);
// v *= factor, factor = a (host value) when norms == nullptr, else 1/sqrt(final norm^2).
template <typename T> void launch_scale(int64_t n, T* v, double a, const NormRefs* norms, hipStream_t s);
// scale fused with the fold of the post-pass norm and the publish step (single-GPU whole-loop drivers): every workgroup
// folds the `nparts` norm partials in the same fixed order, v *= 1/sqrt(sum); workgroup 0 stores the sum to *out and the
// iteration's four scalars (alpha, sum, c0, sum) to the pinned host slot.
// a8 fused with launch_derive_norm (sharded whole-loop drivers): v *= 1 / sqrt(max(*c0_src - sum_i h_i^2, 0)).
template <typename T>
void launch_scale_derive(int64_t n, T* v, const double* c0_src, const double* h, int count, double* c0, double* c1,
                         const double* alpha, double* host_mapped, hipStream_t s);
// src (nullable): read the unnormalised vector from there instead of from v (out of place).
template <typename T>
int launch_scale_publish(int64_t n, T* v, const double* partials, int nparts, double* out, const double* alpha,
                         const double* c0, double* host_mapped, hipStream_t s, const T* src = nullptr);
// Plain three-term update with host scalars (primitive API).
template <typename T>
void launch_three_term(int64_t n, T* w, const T* u_prev, const T* u_cur, double beta, double alpha, hipStream_t s);
// The two-pass recurrence without a stored basis (recur.hip; recurrence.hpp and its two drivers).  rec: one record of kRecurRec
// doubles per iteration k on the device — alpha_k, a_k, b_k, c_k = ||r_k||^2.
constexpr int kRecurRec = 4;
// pass 1: y <- y - a x - b p (p nullable) with alpha folded from the operator kernel's partials, a = alpha / sqrt(c_k),
// b = sqrt(c_k / c_{k-1}) (normalised: x and p were scaled to unit norm in place: a = alpha, b = sqrt(c_k)); (alpha, a, b) ->
// rec[k]; partials[workgroup] = its share of ||y||^2.  Returns the grid.
template <typename T>
int launch_recur_step(int64_t n, T* y, const T* x, const T* p, const double* alpha_partials, int alpha_nparts, double* rec,
                      int64_t k, bool normalised, double* partials, hipStream_t s);
// ... folded by one workgroup: rec[k + 1].c = sum; host_mapped[0..4) = {alpha_k, sum, 0, sum}
void launch_recur_fold(const double* partials, int nparts, double* rec, int64_t k, double* host_mapped, hipStream_t s);
// The coefficient of pass 2's accumulate: a double on real vectors (the Ritz vector's s_k, a real exp(a T_m) e_1), zc on complex
// ones.  of(): from the host scalar.
template <typename T> struct RecurCoeff {
  typedef double type;
  static double of(double g) { return g; }
};
template <> struct RecurCoeff<zc> {
  typedef zc type;
  static zc of(std::complex<double> g) { return zc{g.real(), g.imag()}; }
};
template <> struct RecurCoeff<cf> : RecurCoeff<zc> {};
// pass 2: the same update with (a, b) read from rec[k] (rec == nullptr: the values a, b), then psi += g y with g = gvec[k + 1]
// (gvec == nullptr: the value g).  alpha_partials (nullable, needs rec): workgroup 0 folds them and adds 1 to *mismatches
// when the sum differs as bits from rec[k].alpha.  G = double (every T), or zc (T = zc, cf only): gvec then holds (re, im) pairs, g
// is rounded to T and the product g y is the complex one.  The update of y is the same code, so a replay with either coefficient
// type reproduces pass 1's vectors.
template <typename T, typename G>
void launch_recur_accum(int64_t n, T* y, const T* x, const T* p, T* psi, const double* rec, const G* gvec, int64_t k, double a,
                        double b, G g, const double* alpha_partials, int alpha_nparts, long long* mismatches, hipStream_t s);
// ... for up to kRecurMultiMax accumulators in one sweep (the multi-time Exponentiator): y is updated once, then psi[j] += g_j y for
// j < count with the coefficient type of the storage type (double on d / s, zc on z / c) and g_j = gtab[row[j] * ldg + k + 1]
// (gtab == nullptr: g[j]).  The argument struct travels by value; the host compacts the active accumulators into it per launch.
constexpr int kRecurMultiMax = 16;
constexpr int kRecurMultiBatch = 2;  // accumulators loaded before the first is stored: 1, 2 or 4 (recur.hip)
template <typename T, typename G> struct RecurMultiArgs {
  T* psi[kRecurMultiMax];
  G g[kRecurMultiMax];
  int row[kRecurMultiMax];
  int count;
};
template <typename T>
void launch_recur_accum_multi(int64_t n, T* y, const T* x, const T* p, const RecurMultiArgs<T, typename RecurCoeff<T>::type>& acc,
                              const double* rec, const typename RecurCoeff<T>::type* gtab, int64_t ldg, int64_t k, double a,
                              double b, const double* alpha_partials, int alpha_nparts, long long* mismatches, hipStream_t s);
// psi = g x, out of place, with the product of the accumulate above: the first term of pass 2's sum (G = RecurCoeff<T>::type)
template <typename T, typename G> void launch_recur_seed(int64_t n, T* psi, const T* x, G g, hipStream_t s);
// partials of <a,b> (reals per workgroup). Returns grid.
template <typename T> int launch_dot(int64_t n, const T* a, const T* b, double* partials, hipStream_t s);
// out_r = sum_{k=m-1..0} coeff[r*m+k] * u_k, r < nout; coeff on device, type acc_t<T>; the sums are carried in acc_t<T> and
// rounded to T once.  scratch: nout * n values of acc_t<T> for the partial sums between launches (float types with nlaunch > 1;
// nullable otherwise).
template <typename T>
void launch_gemv_basis(int64_t n, int64_t m, const BasisSegs<T>* segs, int nlaunch, int nout, const acc_t<T>* coeff, T* out,
                       int64_t ld_out, acc_t<T>* scratch, hipStream_t s);
// small helpers
// h_acc += h_add when the second pass ran
void launch_accumulate_h(double* h_acc, const double* h_add, int count, const NormRefs* pred, hipStream_t s);
// out_host_visible[0] = *alpha (0 if null), [1] = final norm^2, [2] = c0, [3] = c1  (pinned, device-mapped memory)
void launch_publish(double* out_mapped, const double* alpha, const NormRefs& norms, hipStream_t s);

// streaming kernels of ll_bandwidth_probe (kernels.hip): a read-only sum and a copy, 16-byte accesses
void launch_bw_read(const void* a, size_t bytes, double* out, int grid, hipStream_t s);
void launch_bw_copy(const void* a, void* b, size_t bytes, int grid, hipStream_t s);

// ---------------------------------------------------------------- host tridiagonal solver (tridiag_host.cpp)
// Flat-array implicit-shift QR; same arithmetic as the reference's (TRI:151-343) so that
// convergence decisions coincide.  q (nullable) row-major m x m, row j = eigenvector j.
int64_t tridiag_qr(int64_t m, const double* alpha, const double* beta, double* ev, double* q);
// Unit eigenvectors for nw given eigenvalues by inverse iteration (O(m) each); out = nw rows of m entries.
void tridiag_inverse_iteration(int64_t m, const double* alpha, const double* beta, int64_t nw, const double* lambdas,
                               double* out);
// k-th smallest eigenvalue by Sturm bisection (TRI:22-88).
double tridiag_bisect(int64_t m, const double* alpha, const double* beta, int64_t k);
// The same for nk roots at once (bit-identical to nk calls of tridiag_bisect; interleaved recurrences, ~5x faster).
void tridiag_bisect_multi(int64_t m, const double* alpha, const double* beta, int nk, const int64_t* ks, double* out);

}  // namespace ll
