// extern "C" surface of liblanczos_hip.so: declared in include/lanczos_hip.h, which documents every entry point
// and cites the reference interface it replaces.  Here: operators, primitives, the tridiagonal solvers and the whole loops
// (everything about the context itself: context.cpp).
#include <cmath>
#include <complex>
#include <limits>

#include "engine.hpp"

using namespace ll;

// ---------------------------------------------------------------- the four storage types of a typed entry point
// M(suffix, storage type T, pointee type of the public data pointers, host-callback type).  Every family ll_<family>_{d,z,s,c}
// is defined ONCE below, as a macro LL_DEF_<FAMILY>(sfx, T, P, H) over this list; the declarations of include/lanczos_hip.h
// stay written out, so a definition that disagrees with its declaration does not compile.  The pointer casts (const T*)x are
// identities for _d / _s.  The body of a family is one call of a template on T; whatever it checks is in that template.
#define LL_CAPI_REAL(M) M(d, double, double, ll_host_mv_mul_d) M(s, float, float, ll_host_mv_mul_s)
#define LL_CAPI_COMPLEX(M) M(z, zc, void, ll_host_mv_mul_z) M(c, cf, void, ll_host_mv_mul_z)
#define LL_CAPI_TYPES(M) LL_CAPI_REAL(M) LL_CAPI_COMPLEX(M)
#define LL_TYPED(family, sfx, params, ...) \
  int ll_##family##_##sfx params { return guarded([&] { __VA_ARGS__; }); }

// ---------------------------------------------------------------- what the typed entry points call
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
template <typename T> void scal_impl(ll_context* ctx, int64_t n, double a, T* v) {
  use(ctx);
  launch_scale<T>(n, v, a, nullptr, ctx->stream);
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
void three_term_impl(ll_context* ctx, int64_t n, T* w, const T* up, const T* uc, double beta, double alpha) {
  use(ctx);
  LL_REQUIRE(w && uc, "null vector");
  launch_three_term<T>(n, w, up, uc, beta, alpha, ctx->stream);
}
template <typename T>
void recur_accum_impl(ll_context* ctx, int64_t n, T* y, const T* x, const T* p, double a, double b, double g, T* psi) {
  use(ctx);
  LL_REQUIRE(n >= 0 && y && x && psi, "null vector");
  launch_recur_accum<T, double>(n, y, x, p, psi, nullptr, nullptr, 0, a, b, g, nullptr, 0, nullptr, ctx->stream);
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
  double* d_htot = nullptr;
  if (h_out && nb > 0) LL_HIP(hipMalloc((void**)&d_htot, (size_t)R * nb * sizeof(double)));
  const DevArray<double> htot(d_htot);
  const NormRefs refs = E.orth(w, runs, mode, ThreeTerm<T>::none(), E.S(kScalScratch), d_htot);
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
template <typename T>
void lanczos_run_impl(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals, T* eigvecs, int64_t* n_found,
                      int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
  lanczos_run<T>(ctx, op, *p, eigvals, eigvecs, n_found, iter_counts, iter_cap, alpha_out, beta_out, stats);
}
template <typename T>
void run_iteration_impl(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot, int64_t n_orth,
                        const T* orth, double* eigvals, T* eigvecs, int64_t* n_found, int64_t* itern, double* alpha_out,
                        double* beta_out, ll_run_stats* stats) {
  LL_REQUIRE(ctx && p && eigvals && n_found, "null argument");
  ll_lanczos_params q = *p;
  q.num_eigs = 1;  // unused by the single-pass mode; keep the range check of the common driver happy
  const IterationSpec<T> spec{nroot, n_orth, orth};
  int64_t count = 0;
  lanczos_run<T>(ctx, op, q, eigvals, eigvecs, n_found, &count, 1, alpha_out, beta_out, stats, &spec);
  if (itern) *itern = count;
}
template <typename T>
void two_pass_impl(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, T* eigvec, int64_t* itern,
                   double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  LL_REQUIRE(ctx && p && eigval, "null argument");
  two_pass_run<T>(ctx, op, *p, eigval, eigvec, itern, residual, alpha_out, beta_out, stats);
}
// a: the real types' double, or the complex types' (a_re, a_im)
template <typename T>
void expo_run_impl(ll_context* ctx, ll_operator* op, const ll_expo_params* p, typename host_scalar<T>::type a, const T* input,
                   T* output, int64_t* itern, ll_run_stats* stats) {
  LL_REQUIRE(ctx && p && input && output && itern, "null argument");
  expo_run<T>(ctx, op, *p, a, input, output, itern, stats);
}
template <typename T>
void taylor_run_impl(ll_context* ctx, ll_operator* op, const ll_expo_params* p, typename host_scalar<T>::type a, const T* input,
                     T* output, int64_t* nterms) {
  LL_REQUIRE(ctx && p && input && output && nterms, "null argument");
  taylor_run<T>(ctx, op, *p, a, input, output, nterms);
}
// (re, im) as the host scalar of T's runs; a non-zero imaginary part on real storage is refused with the caller's text
template <typename T> typename host_scalar<T>::type host_scalar_of(double re, double im, const char* refusal) {
  if constexpr (scalar_traits<T>::is_complex) {
    return std::complex<double>(re, im);
  } else {
    LL_REQUIRE(im == 0.0, refusal);
    return re;
  }
}
constexpr const char* kRealTime = "a_im must be 0 with a real operator";
constexpr const char* kRealCoeff = "g_im must be 0 for the real storage types 'd' and 's'";
template <typename T>
void recur_accum_scaled_impl(ll_context* ctx, int64_t n, void* y, const void* x, const void* p, double a, double b, double g_re,
                             double g_im, void* psi) {
  typedef typename RecurCoeff<T>::type G;
  LL_REQUIRE(n >= 0 && y && x && psi, "null vector");
  const G g = RecurCoeff<T>::of(host_scalar_of<T>(g_re, g_im, kRealCoeff));
  launch_recur_accum<T, G>(n, (T*)y, (const T*)x, (const T*)p, (T*)psi, nullptr, nullptr, 0, a, b, g, nullptr, 0, nullptr, ctx->stream);
}
// the storage type is the operator's
template <typename T>
void expo_two_pass_impl(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im, const void* input,
                        void* output, int64_t* itern, ll_run_stats* stats) {
  expo_two_pass_run<T>(ctx, op, *p, host_scalar_of<T>(a_re, a_im, kRealTime), (const T*)input, (T*)output, itern, stats);
}
template <typename T>
void expo_two_pass_multi_impl(ll_context* ctx, ll_operator* op, const ll_expo_params* p, int64_t n_times, const double* a_reim,
                              const void* input, void* const* outputs, int64_t* itern, ll_run_stats* stats) {
  typename host_scalar<T>::type a[kRecurMultiMax];
  for (int64_t j = 0; j < n_times; ++j) a[j] = host_scalar_of<T>(a_reim[2 * j], a_reim[2 * j + 1], kRealTime);
  expo_two_pass_multi_run<T>(ctx, op, *p, n_times, a, (const T*)input, (T* const*)outputs, itern, stats);
}
template <typename T>
void recur_accum_multi_impl(ll_context* ctx, int64_t n, void* y, const void* x, const void* p, double a, double b, int64_t n_acc,
                            const double* g_reim, void* const* psi) {
  typedef typename RecurCoeff<T>::type G;
  LL_REQUIRE(n >= 0 && y && x && g_reim && psi, "null vector");
  RecurMultiArgs<T, G> acc = {};
  for (int64_t j = 0; j < n_acc; ++j) {
    LL_REQUIRE(psi[j] != nullptr, "null vector");
    acc.psi[j] = (T*)psi[j];
    acc.g[j] = RecurCoeff<T>::of(host_scalar_of<T>(g_reim[2 * j], g_reim[2 * j + 1], kRealCoeff));
  }
  acc.count = (int)n_acc;
  launch_recur_accum_multi<T>(n, (T*)y, (const T*)x, (const T*)p, acc, nullptr, nullptr, 0, 0, a, b, nullptr, 0, nullptr, ctx->stream);
}
}  // namespace

extern "C" {

// ---------------------------------------------------------------- operators (operators.cpp, pauli_operators.cpp build them)
#define LL_DEF_OP_CREATE_CSR(sfx, T, P, H)                                                                                 \
  LL_TYPED(op_create_csr, sfx, (ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci, \
                               const P* va, ll_operator** out),                                                            \
                               create_csr<T>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(false), out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_CSR)
#define LL_DEF_OP_CREATE_CSR_DEV(sfx, T, P, H)                                                                                 \
  LL_TYPED(op_create_csr_dev, sfx, (ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci, \
                                   const P* va, ll_operator** out),                                                            \
                                   create_csr<T>(ctx, nr, nc, rb, rp, ci, va, csr_options_default(true), out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_CSR_DEV)
#define LL_DEF_OP_CREATE_CSR_OPT(sfx, T, P, H)                                                                                 \
  LL_TYPED(op_create_csr_opt, sfx, (ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci, \
                                   const P* va, const ll_csr_options* opt, ll_operator** out),                                 \
                                   create_csr<T>(ctx, nr, nc, rb, rp, ci, va, opt ? *opt : csr_options_default(false), out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_CSR_OPT)
#define LL_DEF_OP_CREATE_CSR_SYM(sfx, T, P, H)                                                                               \
  LL_TYPED(op_create_csr_sym, sfx, (ll_context* ctx, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const P* va, \
                                   const ll_csr_options* opt, ll_operator** out),                                            \
                                   create_csr_sym<T>(ctx, n, uplo, rp, ci, va, opt, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_CSR_SYM)
#define LL_DEF_OP_CREATE_COO(sfx, T, P, H)                                                                         \
  LL_TYPED(op_create_coo, sfx, (ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows, const int32_t* cols, \
                               const P* vals, ll_operator** out),                                                  \
                               create_coo<T>(ctx, n, nnz, rows, cols, vals, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_COO)
#define LL_DEF_OP_CREATE_DENSE(sfx, T, P, H)                                                                           \
  LL_TYPED(op_create_dense, sfx, (ll_context* ctx, int64_t nr, int64_t nc, int64_t rb, const P* a, ll_operator** out), \
                                 create_dense<T>(ctx, nr, nc, rb, a, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_DENSE)
#define LL_DEF_OP_CREATE_STENCIL(sfx, T, P, H)                                                            \
  LL_TYPED(op_create_stencil, sfx, (ll_context* ctx, const ll_stencil_desc* desc, int64_t rb, int64_t nl, \
                                   const double* onsite, ll_operator** out),                              \
                                   create_stencil<T>(ctx, desc, rb, nl, onsite, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_STENCIL)
#define LL_DEF_OP_CREATE_PAULI(sfx, T, P, H)                                                                     \
  LL_TYPED(op_create_pauli, sfx, (ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, \
                                 ll_operator** out),                                                             \
                                 create_pauli<T>(ctx, n_sites, n_terms, terms, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_PAULI)
#define LL_DEF_OP_CREATE_PAULI_SECTOR(sfx, T, P, H)                                                         \
  LL_TYPED(op_create_pauli_sector, sfx, (ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, \
                                        const ll_pauli_term* terms, ll_operator** out),                     \
                                        create_pauli_sector<T>(ctx, n_sites, n_down, n_terms, terms, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_PAULI_SECTOR)
#define LL_DEF_OP_CREATE_PAULI_MOMENTUM(sfx, T, P, H)                                                          \
  LL_TYPED(op_create_pauli_momentum, sfx, (ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, \
                                          int64_t n_terms, const ll_pauli_term* terms, ll_operator** out),     \
                                          create_pauli_momentum<T>(ctx, n_sites, n_down, momentum, n_terms, terms, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_PAULI_MOMENTUM)
#define LL_DEF_OP_CREATE_PAULI_MOMENTUM_FULL(sfx, T, P, H)                                                           \
  LL_TYPED(op_create_pauli_momentum_full, sfx, (ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms, \
                                               const ll_pauli_term* terms, ll_operator** out),                       \
                                               create_pauli_momentum_full<T>(ctx, n_sites, momentum, n_terms, terms, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_PAULI_MOMENTUM_FULL)
#define LL_DEF_OP_CREATE_PAULI_SYMMETRIC(sfx, T, P, H)                                                                     \
  LL_TYPED(op_create_pauli_symmetric, sfx, (ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum,            \
                                           int32_t parity, int32_t inversion, int64_t n_terms, const ll_pauli_term* terms, \
                                           ll_operator** out),                                                             \
                                           create_pauli_symmetric<T>(ctx, n_sites, n_down, momentum, parity, inversion,    \
                                               n_terms, terms, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_PAULI_SYMMETRIC)
// untyped: the storage type is named by a character, as the untyped primitives name it
int ll_op_create_pauli_torus(ll_context* ctx, int32_t storage, int32_t lx, int32_t ly, int32_t n_down, int32_t mx, int32_t my,
                             int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  return guarded([&] {
    for_storage_char(storage, [&](auto t) { create_pauli_torus<decltype(t)>(ctx, lx, ly, n_down, mx, my, n_terms, terms, out); });
  });
}
// every host callback is stored under the void* signature (same ABI, only the pointee types differ): an identity cast for _z / _c
#define LL_DEF_OP_CREATE_HOST(sfx, T, P, H)                                                        \
  LL_TYPED(op_create_host, sfx, (ll_context* ctx, int64_t n, H fn, void* user, ll_operator** out), \
                                create_cb<T>(ctx, n, reinterpret_cast<ll_host_mv_mul_z>(fn), nullptr, user, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_HOST)
#define LL_DEF_OP_CREATE_DEVICE(sfx, T, P, H)                                                                    \
  LL_TYPED(op_create_device, sfx, (ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out), \
                                  create_cb<T>(ctx, n, nullptr, fn, user, out))
LL_CAPI_TYPES(LL_DEF_OP_CREATE_DEVICE)
int ll_csr_options_default(ll_csr_options* opt) {
  return guarded([&] {
    LL_REQUIRE(opt != nullptr, "null options");
    std::memset(opt, 0, sizeof(*opt));
    opt->accuracy = LL_ACCURACY_DEFAULT;
    opt->kernel = -1;
  });
}
int ll_op_device_bytes(const ll_operator* op, int64_t* bytes) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && bytes != nullptr, "null argument");
    if (op->ctx) LL_HIP(hipSetDevice(op->ctx->device));
    *bytes = op->device_bytes();
  });
}
int ll_op_inf_norm(const ll_operator* op, double* out) {
  return guarded([&] {
    LL_REQUIRE(op != nullptr && out != nullptr, "null argument");
    LL_REQUIRE(op->inf_norm >= 0.0, "the infinity norm is only known for CSR/COO/dense/lattice operators created from host data");
    *out = op->inf_norm;
  });
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
#define LL_DEF_SPMV(sfx, T, P, H)                                                                       \
  LL_TYPED(spmv, sfx, (ll_context* ctx, ll_operator* op, const P* x, P* y, double offset, double* dot), \
                      spmv_impl<T>(ctx, op, (const T*)x, (T*)y, offset, dot))
LL_CAPI_TYPES(LL_DEF_SPMV)
#define LL_DEF_DOT(sfx, T, P, H)                                                        \
  LL_TYPED(dot, sfx, (ll_context* ctx, int64_t n, const P* a, const P* b, double* out), \
                     dot_impl<T>(ctx, n, (const T*)a, (const T*)b, out))
LL_CAPI_TYPES(LL_DEF_DOT)
#define LL_DEF_NRM2(sfx, T, P, H)                                            \
  LL_TYPED(nrm2, sfx, (ll_context* ctx, int64_t n, const P* v, double* out), \
                      nrm2_impl<T>(ctx, n, (const T*)v, out))
LL_CAPI_TYPES(LL_DEF_NRM2)
#define LL_DEF_SCAL(sfx, T, P, H)                                   \
  LL_TYPED(scal, sfx, (ll_context* ctx, int64_t n, double a, P* v), \
                      scal_impl<T>(ctx, n, a, (T*)v))
LL_CAPI_TYPES(LL_DEF_SCAL)
#define LL_DEF_NORMALIZE(sfx, T, P, H)                                           \
  LL_TYPED(normalize, sfx, (ll_context* ctx, int64_t n, P* v, double* norm_out), \
                           normalize_impl<T>(ctx, n, (T*)v, norm_out))
LL_CAPI_TYPES(LL_DEF_NORMALIZE)
#define LL_DEF_THREE_TERM(sfx, T, P, H)                                                                              \
  LL_TYPED(three_term, sfx, (ll_context* ctx, int64_t n, P* w, const P* up, const P* uc, double beta, double alpha), \
                            three_term_impl<T>(ctx, n, (T*)w, (const T*)up, (const T*)uc, beta, alpha))
LL_CAPI_TYPES(LL_DEF_THREE_TERM)
#define LL_DEF_RECUR_ACCUM(sfx, T, P, H)                                                                                       \
  LL_TYPED(recur_accum, sfx, (ll_context* ctx, int64_t n, P* y, const P* x, const P* p, double a, double b, double g, P* psi), \
                             recur_accum_impl<T>(ctx, n, (T*)y, (const T*)x, (const T*)p, a, b, g, (T*)psi))
LL_CAPI_TYPES(LL_DEF_RECUR_ACCUM)
#define LL_DEF_ORTH_BLOCK(sfx, T, P, H)                                                                          \
  LL_TYPED(orth_block, sfx, (ll_context* ctx, int64_t n, int64_t nb, const P* basis, int64_t ld, P* w, int mode, \
                            double* norm_out, double* h_out),                                                    \
                            orth_impl<T>(ctx, n, nb, (const T*)basis, ld, (T*)w, mode, norm_out, h_out))
LL_CAPI_TYPES(LL_DEF_ORTH_BLOCK)
// coefficients arrive as doubles (re,im pairs for the complex types) like every scalar of the API: acc_t<T>, which is T for _d / _z
#define LL_DEF_GEMV_BASIS(sfx, T, P, H)                                                                                   \
  LL_TYPED(gemv_basis, sfx, (ll_context* ctx, int64_t n, int64_t m, const P* basis, int64_t ld, int64_t nout,             \
                            const double* coeff, P* out, int64_t ld_out),                                                 \
                            gemv_impl<T, acc_t<T>>(ctx, n, m, (const T*)basis, ld, nout, (const acc_t<T>*)coeff, (T*)out, \
                                ld_out))
LL_CAPI_TYPES(LL_DEF_GEMV_BASIS)
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

#define LL_DEF_LANCZOS_RUN(sfx, T, P, H)                                                                                      \
  LL_TYPED(lanczos_run, sfx, (ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals, P* eigvecs,      \
                             int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,   \
                             ll_run_stats* stats),                                                                            \
                             lanczos_run_impl<T>(ctx, op, p, eigvals, (T*)eigvecs, n_found, iter_counts, iter_cap, alpha_out, \
                                 beta_out, stats))
LL_CAPI_TYPES(LL_DEF_LANCZOS_RUN)
#define LL_DEF_LANCZOS_RUN_ITERATION(sfx, T, P, H)                                                                            \
  LL_TYPED(lanczos_run_iteration, sfx, (ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,          \
                                       int64_t n_orth, const P* orth, double* eigvals, P* eigvecs, int64_t* n_found,          \
                                       int64_t* itern, double* alpha_out, double* beta_out, ll_run_stats* stats),             \
                                       run_iteration_impl<T>(ctx, op, p, nroot, n_orth, (const T*)orth, eigvals, (T*)eigvecs, \
                                           n_found, itern, alpha_out, beta_out, stats))
LL_CAPI_TYPES(LL_DEF_LANCZOS_RUN_ITERATION)
#define LL_DEF_LANCZOS_TWO_PASS(sfx, T, P, H)                                                                                  \
  LL_TYPED(lanczos_two_pass, sfx, (ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval, P* eigvec,    \
                                  int64_t* itern, double* residual, double* alpha_out, double* beta_out, ll_run_stats* stats), \
                                  two_pass_impl<T>(ctx, op, p, eigval, (T*)eigvec, itern, residual, alpha_out, beta_out,       \
                                      stats))
LL_CAPI_TYPES(LL_DEF_LANCZOS_TWO_PASS)
// the scalar a is one double for the real types and (a_re, a_im) for the complex ones: these two families have two forms each
#define LL_DEF_EXPO_RUN_REAL(sfx, T, P, H)                                                                                 \
  LL_TYPED(expo_run, sfx, (ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const P* input, P* output, \
                          int64_t* itern, ll_run_stats* stats),                                                            \
                          expo_run_impl<T>(ctx, op, p, a, (const T*)input, (T*)output, itern, stats))
LL_CAPI_REAL(LL_DEF_EXPO_RUN_REAL)
#define LL_DEF_EXPO_RUN_COMPLEX(sfx, T, P, H)                                                                                \
  LL_TYPED(expo_run, sfx, (ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,              \
                          const P* input, P* output, int64_t* itern, ll_run_stats* stats),                                   \
                          expo_run_impl<T>(ctx, op, p, std::complex<double>(a_re, a_im), (const T*)input, (T*)output, itern, \
                              stats))
LL_CAPI_COMPLEX(LL_DEF_EXPO_RUN_COMPLEX)
#define LL_DEF_EXPO_TAYLOR_RUN_REAL(sfx, T, P, H)                                                                      \
  LL_TYPED(expo_taylor_run, sfx, (ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const P* input, \
                                 P* output, int64_t* nterms),                                                          \
                                 taylor_run_impl<T>(ctx, op, p, a, (const T*)input, (T*)output, nterms))
LL_CAPI_REAL(LL_DEF_EXPO_TAYLOR_RUN_REAL)
#define LL_DEF_EXPO_TAYLOR_RUN_COMPLEX(sfx, T, P, H)                                                                           \
  LL_TYPED(expo_taylor_run, sfx, (ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,         \
                                 const P* input, P* output, int64_t* nterms),                                                  \
                                 taylor_run_impl<T>(ctx, op, p, std::complex<double>(a_re, a_im), (const T*)input, (T*)output, \
                                     nterms))
LL_CAPI_COMPLEX(LL_DEF_EXPO_TAYLOR_RUN_COMPLEX)

// ---------------------------------------------------------------- untyped additions within minor 5 (the storage type is an argument)
int ll_expo_two_pass(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im, const void* input,
                     void* output, int64_t* itern_out, ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && op && p && input && output && itern_out, "null argument");
    for_storage_type(*op, [&](auto t) { expo_two_pass_impl<decltype(t)>(ctx, op, p, a_re, a_im, input, output, itern_out, stats); });
  });
}
int ll_recur_accum_scaled(ll_context* ctx, int storage, int64_t n, void* y, const void* x, const void* p, double a, double b,
                          double g_re, double g_im, void* psi) {
  return guarded([&] {
    use(ctx);
    for_storage_char(storage, [&](auto t) { recur_accum_scaled_impl<decltype(t)>(ctx, n, y, x, p, a, b, g_re, g_im, psi); });
  });
}
int ll_expo_two_pass_multi(ll_context* ctx, ll_operator* op, const ll_expo_params* p, int64_t n_times, const double* a_reim,
                           const void* input, void* const* outputs, int64_t* itern_out, ll_run_stats* stats) {
  return guarded([&] {
    LL_REQUIRE(ctx && op && p && a_reim && input && outputs, "null argument");
    LL_REQUIRE(n_times >= 1 && n_times <= kRecurMultiMax, "n_times must be between 1 and 16");
    for_storage_type(*op, [&](auto t) {
      expo_two_pass_multi_impl<decltype(t)>(ctx, op, p, n_times, a_reim, input, outputs, itern_out, stats);
    });
  });
}
int ll_recur_accum_multi(ll_context* ctx, int storage, int64_t n, void* y, const void* x, const void* p, double a, double b,
                         int64_t n_acc, const double* g_reim, void* const* psi) {
  return guarded([&] {
    use(ctx);
    LL_REQUIRE(n_acc >= 1 && n_acc <= kRecurMultiMax, "n_acc must be between 1 and 16");
    for_storage_char(storage, [&](auto t) { recur_accum_multi_impl<decltype(t)>(ctx, n, y, x, p, a, b, n_acc, g_reim, psi); });
  });
}
int ll_pauli_expect(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs_host, const void* psi,
                    double* out_host, int64_t* sweeps_out) {
  return guarded([&] { pauli_expect(ctx, op, n_obs, obs_host, psi, out_host, sweeps_out); });
}
int ll_pauli_expect_block(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs_host, const void* psi,
                          double* out_host, int64_t* sweeps_out) {
  return guarded([&] { pauli_expect_block(ctx, op, n_obs, obs_host, psi, out_host, sweeps_out); });
}
int ll_pauli_block_expand(ll_context* ctx, const ll_operator* block, const ll_operator* target, const void* c, void* psi_out) {
  return guarded([&] { pauli_block_embed(ctx, block, target, true, c, psi_out); });
}
int ll_pauli_block_project(ll_context* ctx, const ll_operator* block, const ll_operator* target, const void* psi, void* c_out) {
  return guarded([&] { pauli_block_embed(ctx, block, target, false, psi, c_out); });
}
int ll_pauli_block_transfer(ll_context* ctx, const ll_operator* source, const ll_operator* target, int64_t n_terms,
                            const ll_pauli_term* terms_host, const void* c, void* out, double* norm2_out) {
  return guarded([&] { pauli_block_transfer(ctx, source, target, n_terms, terms_host, c, out, norm2_out); });
}
int ll_pauli_rdm(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites_host, const void* psi,
                 double* out_host, int64_t* sweeps_out) {
  return guarded([&] { pauli_rdm(ctx, op, n_sub, sites_host, psi, out_host, sweeps_out); });
}
int ll_pauli_rdm_tiled(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites_host, const void* psi, void* out,
                       int64_t* sweeps_out) {
  return guarded([&] { pauli_rdm_tiled(ctx, op, n_sub, sites_host, psi, out, sweeps_out); });
}

}  // extern "C"
