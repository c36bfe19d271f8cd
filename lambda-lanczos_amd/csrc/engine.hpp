// Host drivers of the device-resident Lanczos loop (templated on the scalar type; Engine, Basis and RunList are instantiated
// in engine.cpp, the whole-loop drivers in lanczos_run.cpp, expo_run.cpp, two_pass_run.cpp and expo_two_pass_multi_run.cpp).  See
// DESIGN.md for the data flow.
#pragma once

#include <chrono>
#include <complex>
#include <functional>
#include <map>
#include <system_error>
#include <thread>
#include <variant>

#include "ll_internal.hpp"

namespace ll {

// Device scalar area (ctx->scal, 128 doubles):
//   [0..16)   alpha ring (slot = k % 16: kRingSlots, loop_support.hpp)
//   [16..64)  norm triples (c0,c1,c2) ring, slot s at 16 + 3*s
//   [64..67)  scratch triple for one-off orthogonalisations (start vector, primitives)
//   [72]      spare scalar (dot results)
//   [127]     constant 0
constexpr int kScalAlpha = 0, kScalNorms = 16, kScalScratch = 64, kScalSpare = 72, kScalZero = 127, kScalCount = 128;

// ---------------------------------------------------------------- host helpers shared by Engine and the whole-loop drivers
inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// Whole-loop entry points accept host OR device memory for their n-sized inputs and outputs (start vector, Ritz
// vectors, Exponentiator input/output): a device pointer keeps the vector in HBM (no PCIe crossing, no staging).
inline bool is_device_ptr(const void* p) {
  if (p == nullptr) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // plain (unregistered) host memory
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}
// n-sized copies between two HOST buffers at the reference's std::vector boundary (pinned staging buffer -> the caller's vector):
// one thread moves 8-10 GB/s, which made this copy the longest single item of a run's epilogue (80 MB: 9 ms); four threads
// share it from 8 MiB up.
inline void host_copy(void* dst, const void* src, size_t bytes) {
  constexpr size_t kParallelFrom = (size_t)8 << 20;
  constexpr int kThreads = 4;
  if (bytes < kParallelFrom) {
    std::memcpy(dst, src, bytes);
    return;
  }
  const size_t piece = ((bytes / kThreads) + 4095) & ~(size_t)4095;
  std::thread th[kThreads - 1];
  int started = 0;
  for (int t = 1; t < kThreads; ++t) {
    const size_t off = std::min(bytes, (size_t)t * piece), len = std::min(bytes, (size_t)(t + 1) * piece) - off;
    try {
      th[t - 1] = std::thread([=] {
        if (len) std::memcpy((char*)dst + off, (const char*)src + off, len);
      });
      ++started;
    } catch (const std::system_error&) {
      // no thread to be had (thread limit, cgroup pids): this and the remaining ranges are copied here — never std::terminate
      // out of a joinable thread's destructor, never an error for what is only a slower copy
      const size_t rest = std::min(bytes, (size_t)t * piece);
      std::memcpy((char*)dst + rest, (const char*)src + rest, bytes - rest);
      break;
    }
  }
  std::memcpy(dst, src, std::min(bytes, piece));
  for (int t = 0; t < started; ++t) th[t].join();
}
// LDS budget of mdot / lagged_kernel: 4 waves x ncols doubles in the 160 KB of a CU (one workgroup per CU then, which is
// how the streaming kernels run on long vectors anyway)  =>  reals * nb <= 5000
template <typename T> inline int max_vecs_per_launch() { return kLaggedMaxCols / scalar_traits<T>::reals; }

// ---------------------------------------------------------------- chunked device slab for the Krylov basis
// The reference keeps one heap std::vector per Lanczos vector (LL:221,250; reserve(200) LL:181).  Here the basis
// lives in HBM as a few large slabs of `chunk_vecs` vectors with a common leading dimension (multiple of 256
// elements => every vector is 2 KiB aligned); slabs are appended on demand and reused across restart passes,
// nothing is allocated per iteration.
template <typename T> struct Basis {
  ll_context* ctx = nullptr;
  int64_t n_local = 0, ld = 0;
  int64_t chunk_vecs = 0;
  std::vector<T*> chunks;
  ~Basis();
  void init(ll_context* c, int64_t n_local_, int64_t ld_, int64_t chunk_vecs_);
  T* vec(int64_t k);  // pointer to vector k, growing the slab list if needed
};

// A list of (base, count) runs with a common ld, packed into kernel-argument groups.
template <typename T> struct RunList {
  std::vector<std::pair<const T*, int>> runs;
  int64_t ld = 0;
  int total() const {
    int t = 0;
    for (auto& r : runs) t += r.second;
    return t;
  }
  void add(const T* base, int64_t count) {
    if (count > 0) runs.emplace_back(base, (int)count);
  }
  void add_basis(Basis<T>& b, int64_t count) {  // vectors [0, count)
    ld = b.ld;
    for (int64_t k = 0; k < count; k += b.chunk_vecs) add(b.vec(k), std::min(b.chunk_vecs, count - k));
  }
  // launch groups of at most kMaxSegs runs and max_vecs vectors each (runs are split when needed)
  std::vector<BasisSegs<T>> groups(int max_vecs) const;
};

template <typename T> inline BasisSegs<T> no_segs(int64_t ld) {  // no basis vectors (a launch without Gram-Schmidt columns)
  BasisSegs<T> none;
  none.nseg = 0;
  none.ld = ld;
  return none;
}

// What an operator image takes as its input x besides a normalised vector: the one statement that Engine::apply and the
// loops' choice of form (can_scale_input, can_defer_scale) read.  Every device operator can take its input unnormalised
// (sharded contexts gather / exchange the unnormalised shards): the PB, tiled and one-triangle kernels take ||w||^2
// themselves (norm2), the others scale the finished row sum through a ScaleIn, to which apply hands ||w||^2 as a
// one-element list of partials (scale_in).  Only the ScaleIn kernels can normalise their input on the fly with all that
// goes with it (defer: write u_k, publish), and only on a single GPU: sharded contexts gather the normalised vector.  The
// PB kernels keep the separate normalisation (they want max|u_k| from it); callbacks hand x to user code.
struct InputCaps {
  bool norm2 = false, scale_in = false, defer = false;
};
inline InputCaps input_caps(int kind, int spmv_kind, bool sharded) {
  InputCaps c;
  if (kind == ll_operator::CSR && spmv_kind != LL_SPMV_CSR_STREAM) c.norm2 = true;
  else if (kind == ll_operator::CSR || kind == ll_operator::STENCIL || kind == ll_operator::DENSE || ll_operator::is_pauli(kind))
    c.scale_in = true;
  c.defer = c.scale_in && !sharded;
  return c;
}

template <typename T> struct Engine {
  ll_context* ctx;
  ll_operator* op;  // may be null for pure BLAS-1 use
  int64_t n_local;
  static constexpr int R = scalar_traits<T>::reals;

  Engine(ll_context* c, ll_operator* o, int64_t n_local_) : ctx(c), op(o), n_local(n_local_) {}
  InputCaps input_caps() const { return op ? ll::input_caps(op->kind, op->spmv_kind, ctx->comm != nullptr) : InputCaps{}; }

  double* S(int i) const { return ctx->scal.get() + i; }
  NormRefs plain_norm(double* c1) const { return NormRefs{S(kScalZero), c1, c1, 0}; }

  // y = A x + offset x ; Re<x,y> -> *d_alpha (device scalar, all-reduced over ranks); d_alpha nullable.
  // x_padded: x_local is readable up to the padded shard length n_shard (true for basis vectors).
  // defer (nullable): the caller's multi-dot will fold alpha itself (ThreeTerm::alpha_partials); apply then only leaves
  // the partials behind and reports them here.  Honoured on unsharded contexts only (a communicator needs the folded
  // scalar for its all-reduce): check defer->nparts > 0 afterwards.
  struct DeferredAlpha {
    const double* partials = nullptr;
    int nparts = 0;
  };
  // sc (nullable): deferred normalisation — x_local is the unnormalised w_k (ScaleIn, ll_internal.hpp); only where
  // can_defer_scale() holds.
  // xnorm2 (nullable device scalar; device operators): x_local is an unnormalised vector w with
  // ||w||^2 = *xnorm2 and the operator works with w / ||w|| (lagged Gram-Schmidt, LoopState in lanczos_loop.hpp).
  void apply(const T* x_local, T* y, double offset, double* d_alpha, bool x_padded = false, DeferredAlpha* defer = nullptr,
             const ScaleIn<T>* sc = nullptr, const double* xnorm2 = nullptr);
  bool can_scale_input() const { return input_caps().norm2 || input_caps().scale_in; }  // xnorm2 is accepted
  bool can_defer_scale() const { return input_caps().defer; }                           // sc is accepted
  // The exchange step of a sharded context: x_local's shard all-gathered (chunk by chunk for PB).  own_first: the image has
  // work on its own columns to run under the gather (only then is the gather issued on the communication stream).
  struct Gathered {
    const T* x_own;   // the rank's shard, readable up to the shard stride n_shard
    const T* x_full;  // the gathered vector: chunk-major by op->pb.gather for PB, in global order otherwise
    bool overlap;     // issued on comm_stream: consumers wait on the events below (otherwise they are in stream order)
    hipEvent_t xmax;  // the tiled kernel's max|x| has arrived (null: not gathered, or no overlap)
    const hipEvent_t* chunk_ev;
    int nchunks;
    hipEvent_t chunk(int c) const { return overlap ? chunk_ev[c] : nullptr; }  // chunk c has arrived
    hipEvent_t whole() const { return chunk(nchunks - 1); }                     // the whole vector has arrived
  };
  Gathered gather_x(const T* x_local, bool x_padded, bool own_first);
  void wait(hipEvent_t e) {  // the compute stream waits for e (null: nothing to wait for)
    if (e) LL_HIP(hipStreamWaitEvent(ctx->stream, e, 0));
  }
  // the operator images (apply); each returns the number of alpha partials it left in dotp
  typedef int (*RowLauncher)(const ll_operator&, const T*, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*, int);
  int apply_rows(RowLauncher launch, bool split, const T* x, bool x_padded, T* y, double offset, double* dotp,
                 const ScaleIn<T>* sc);
  int apply_lattice(const T* x, T* y, double offset, double* dotp, const ScaleIn<T>* sc);
  int apply_pb(const T* x, bool x_padded, T* y, double offset, double* dotp, const double* xnorm2);
  int apply_tiled(const T* x, bool x_padded, T* y, double offset, double* dotp, const double* xnorm2);
  int apply_callback(const T* x, T* y, double offset, double* dotp);
  // ---- Gram-Schmidt in two sweeps (multi-dot, multi-axpy) with an optional fused three-term update; c = device triple for the norms
  // The complete call (the primitive ll_orth_block_*, a restart pass's start vector): orthogonalise w against the runs in `mode`,
  // the second pass of the CGS modes decided on the device.  Returns the NormRefs every consumer must use for ||w|| afterwards.
  // h_total (device, nullable): R*nb doubles.
  NormRefs orth(T* w, const RunList<T>& runs, int mode, const ThreeTerm<T>& tt, double* c, double* h_total);
  // What a whole-loop iteration asks of its pass: where the iteration's four scalars go.
  struct PassRequest {
    double* host = nullptr;         // pinned, device-mapped slot of 4 doubles
    const double* alpha = nullptr;  // device scalar
    bool caller_normalises = false; // the caller scales w right after the pass and can carry the norm's fold + the publish step there
  };
  // How a pass ended: exactly one of four.
  struct Published {};        // c[1] holds the norm, the four scalars are on their way to the host
  struct Folded {};           // c[1] holds the all-reduced norm; the caller publishes
  struct PartialsPending {    // no fold launched: the caller's normalisation kernel folds and publishes (launch_scale_publish, ScaleIn)
    const double* partials;
    int nparts;
    const double* c0;  // ||w||^2 before the pass (null: a pass without Gram-Schmidt has none)
    double* c1;
  };
  struct DerivePending {  // sharded: the caller's normalisation kernel forms ||w'||^2 = *c0_src - sum h_i^2 and publishes (launch_scale_derive)
    const double* c0_src;
    const double* h;
    int count;
    double* c0_out;  // c0_out / c1 receive the two norms
    double* c1;
  };
  typedef std::variant<Published, Folded, PartialsPending, DerivePending> PassEnding;
  struct PassEnd {
    NormRefs refs;
    PassEnding how;
  };
  // The loop's pass (LoopState::enqueue; req nullable: second_pass).  LL_ORTH_CGS_DGKS, and any mode without basis vectors: pass 1
  // only, ending in whichever of the four ways the request and the context allow; the final norm of refs is c1, and the driver
  // evaluates the DGKS test on the host from the published (c0, c1) one iteration later and runs the rare second pass itself
  // (second_pass below) — no predicated no-op launches or collectives per iteration.  LL_ORTH_MGS and LL_ORTH_CGS2 against basis
  // vectors: the complete call, which ends Folded.
  PassEnd orth_pass(T* w, const RunList<T>& runs, int mode, const ThreeTerm<T>& tt, double* c, const PassRequest* req);
  // The deferred second pass on the already normalised vector u = w1/||w1||: orthogonalise against `runs` once more,
  // renormalise, and return ||u'||^2 (the factor by which beta^2 shrinks).  Synchronises the stream.
  double second_pass(T* u, const RunList<T>& runs);
  // the pieces of orth / orth_pass: the three-term update alone (no basis vectors), the sequential sweep of LL_ORTH_MGS, the two
  // passes of the CGS modes (derive: the norm after pass 1 follows from the all-reduced coefficients, loop passes on sharded
  // contexts), and how a pass ends given the partial sums of its norm and what the caller asked for
  PassEnd three_term_only(T* w, int64_t ld, const ThreeTerm<T>& tt, double* c, const PassRequest* req);
  NormRefs mgs_sweep(T* w, const RunList<T>& runs, const ThreeTerm<T>& tt, double* c, double* h_total);
  PassEnd cgs_first_pass(T* w, const std::vector<BasisSegs<T>>& groups, int nb, const ThreeTerm<T>& tt, double* c, bool derive,
                         const PassRequest* req);
  void cgs_second_pass(T* w, const std::vector<BasisSegs<T>>& groups, int nb, const NormRefs* pred, double* c);
  PassEnding close_pass(const double* partials, int nparts, const double* c0, double* c, const PassRequest* req);
  // ||v||^2 -> *d_out (device, all-reduced)
  void norm2_dev(const T* v, double* d_out);
  // <a,b> -> d_out[0..R) (device, all-reduced)
  void dot_dev(const T* a, const T* b, double* d_out);
  void all_reduce(double* d, size_t count);
  // device-time stamps around an exchange step on stream cs (no-ops unless ctx->profiling)
  void comm_timer_begin(hipStream_t cs);
  void comm_timer_end(hipStream_t cs);
  // read `count` doubles from the device scalar area (synchronises the stream)
  void fetch(const double* d, double* host, size_t count);
  // out_r = sum_k coeff[r*m+k] u_k  (coeff host, type T)
  void gemv(const RunList<T>& basis, int64_t m, int nout, const T* coeff_host, T* out, int64_t ld_out);
  // the same with coefficients in acc_t<T> (the float entry points take them as doubles, like every scalar)
  void gemv_acc(const RunList<T>& basis, int64_t m, int nout, const acc_t<T>* coeff_host, T* out, int64_t ld_out);
};

template <typename T> struct host_scalar;
template <> struct host_scalar<double> { typedef double type; };
template <> struct host_scalar<zc> { typedef std::complex<double> type; };
// float storage: the k-sized host math (tridiagonal step, exp(a T_k) e_1, coefficients) stays in double
template <> struct host_scalar<float> { typedef double type; };
template <> struct host_scalar<cf> { typedef std::complex<double> type; };

// LambdaLanczos<T>::run_iteration (LL:216-322) as a mode of lanczos_run: ONE pass with `nroot` Ritz pairs,
// Gram-Schmidt against n_orth caller-provided vectors (the reference's orthogonalizeTo; host, vector j at
// orth_host + j*n_local), every computed pair returned in comparator order without EigenPairManager filtering.
template <typename T> struct IterationSpec {
  int64_t nroot;
  int64_t n_orth;
  const T* orth_host;
};

// Vectors per basis slab of a run, and the bytes of one slab of a default run on an operator of this shape (engine.cpp)
int64_t pick_chunk_vecs(int64_t initial_vector_size, int64_t max_iteration, int64_t vec_bytes, int64_t cap_bytes);
int64_t default_slab_bytes(int64_t n, int64_t n_local, int64_t n_shard, int elem_bytes, const Tuning& tune);

// Whole-loop drivers (lanczos_run.cpp; expo_run.cpp; two_pass_run.cpp; expo_two_pass_multi_run.cpp)
template <typename T>
void lanczos_run(ll_context* ctx, ll_operator* op, const ll_lanczos_params& P, double* eigvals, T* eigvecs,
                 int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,
                 ll_run_stats* stats, const IterationSpec<T>* spec = nullptr);
// The extreme eigenpair without a stored basis: three (no eigenvector, or eigvec in device memory) or four n-sized work vectors
// whatever the iteration count; eigvec (host or device, nullable), residual_out, alpha_out, beta_out nullable.
template <typename T>
void two_pass_run(ll_context* ctx, ll_operator* op, const ll_lanczos_params& P, double* eigval_out, T* eigvec,
                  int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats);
template <typename T>
void expo_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P, typename host_scalar<T>::type a,
              const T* input, T* output, int64_t* itern_out, ll_run_stats* stats);
// expo_run without a stored basis (expo_two_pass_multi_run.cpp, as a list of one time): three n-sized work vectors whatever the
// iteration count, four when the output is host memory; the plain recurrence only (full_orthogonalize is refused), every operator
// application twice.
template <typename T>
void expo_two_pass_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P, typename host_scalar<T>::type a,
                       const T* input, T* output, int64_t* itern_out, ll_run_stats* stats);
// ... for n_times values of a on ONE Krylov space: pass 1 once with a stop test per a_j, pass 2 once
// with one accumulator per output; outputs[j] (host or device memory, decided per pointer) and itern_out[j] (nullable array) are
// what expo_two_pass_run gives for a[j]; three work vectors plus one per output in host memory.
template <typename T>
void expo_two_pass_multi_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P, int64_t n_times,
                             const typename host_scalar<T>::type* a, const T* input, T* const* outputs, int64_t* itern_out,
                             ll_run_stats* stats);
template <typename T>
void taylor_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P, typename host_scalar<T>::type a,
                const T* input, T* output, int64_t* nterms_out);

}  // namespace ll
