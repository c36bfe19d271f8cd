/*
 * lanczos_hip.h — C ABI of the MI355X-native Lanczos hot path (liblanczos_hip.so).
 *
 * This is the drop-in boundary.  The reference (mrcdr/lambda-lanczos) is a
 * header-only C++ template library, so its "FFI" is the template API itself; templates cannot cross a
 * C ABI, therefore every entry point exists per scalar type with the BLAS-style suffixes
 *     _d  = double                  (reference T = double)
 *     _z  = double complex          (reference T = std::complex<double>, interleaved re,im)
 *     _s  = float                   (reference T = float)
 *     _c  = float complex           (reference T = std::complex<float>, interleaved re,im)
 *   (the _s/_c declarations are at the end of this file: same arguments as _d/_z with float data pointers; every
 *   scalar — offsets, eps, alpha, eigenvalues, norms — is passed as double (ll_spmv_s/_c apply the offset rounded to float,
 *   see ACCURACY below), and all reductions are accumulated in double,
 *   which is at least the accuracy of the reference's float arithmetic.  long double has no device counterpart.)
 * and the C++ facade include/lambda_lanczos_hip/{lambda_lanczos,exponentiator}.hpp re-creates
 * lambda_lanczos::LambdaLanczos<T> / Exponentiator<T> on top by tag dispatch.
 *
 * Reference citations (paths relative to the reference repository root):
 *   LL  = include/lambda_lanczos/lambda_lanczos.hpp
 *   EX  = include/lambda_lanczos/exponentiator.hpp
 *   LA  = include/lambda_lanczos/util/linear_algebra.hpp
 *   TRI = include/lambda_lanczos/lambda_lanczos_tridiagonal_impl.hpp
 *
 * Conventions
 *   - every function returns an int status: 0 = LL_OK, otherwise an LL_ERR_* code; ll_last_error()
 *     returns a thread-local human readable message for the last failure.  (The reference has no error
 *     channel at all: asserts only, LA:31, EX:88 — this is additive.)
 *   - pointers named *_dev are device (HBM) pointers owned by the caller (ll_malloc or any HIP
 *     allocation on the context's device); pointers named *_host are host memory.
 *   - all device work is enqueued on the context's HIP stream; primitive calls are asynchronous unless
 *     they return a host scalar, whole-loop calls (ll_lanczos_run_*, ll_expo_run_*) are synchronous.
 *   - a context is not re-entrant; one context per host thread (the reference is single threaded and has
 *     no globals, SURVEY 8b "Threading").
 *   - no CPU fallback exists: without a HIP device every call that touches the device fails with
 *     LL_ERR_HIP.
 */
#ifndef LANCZOS_HIP_H_
#define LANCZOS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LL_VERSION_MAJOR 0
#define LL_VERSION_MINOR 5  /* 2: ll_lanczos_params.init_vector_dev, device pointers accepted for n-sized buffers
                             * 3: ll_run_stats.lagged_iterations + reserved tail (the struct grew: code compiled against a
                             *    minor-2 header must be rebuilt — ll_abi_check refuses it), ll_ctx_reload_env, ll_abi_check
                             * 4: additive — ll_csr_options / ll_op_create_csr_opt_*, ll_op_set_accuracy, ll_op_accuracy, the tiled
                             *    SpMV kernel id; no struct changed, callers built against minor 3 keep working
                             * 5: additive — ll_ctx_set_tuning (the test hooks and geometry overrides left the environment),
                             *    ll_comm_transport, ll_bandwidth_probe, ll_op_tiled_layout; no struct changed;
                             *    also additive under minor 5 — ll_op_create_csr_sym_* (one stored triangle), the one-triangle
                             *    SpMV kernel id, ll_op_device_bytes; no struct changed;
                             *    also additive under minor 5 — ll_op_create_pauli_sector_* (one S_z sector; the minor stays 5:
                             *    no struct changed, and callers that need these entry points find them by name);
                             *    also additive under minor 5, with the same note — ll_op_create_pauli_momentum_* (one momentum block
                             *    of an S_z sector of a ring) and ll_op_create_pauli_momentum_full_* (one momentum block of the full
                             *    2^n_sites space of a ring: no S_z conservation asked);
                             *    also additive under minor 5, with the same note — ll_op_create_pauli_symmetric_* (momentum,
                             *    reflection and spin-inversion blocks of a ring);
                             *    also additive under minor 5, with the same note — ll_expo_two_pass (the Exponentiator without a
                             *    stored Krylov basis) and ll_recur_accum_scaled (its replayed step with a complex coefficient): two
                             *    UNTYPED entry points, the storage type comes from the operator / from an argument; ll_run_stats
                             *    keeps its size (workspace_vectors and replay_mismatches are filled by ll_expo_two_pass too);
                             *    also additive under minor 5, with the same note — ll_expo_two_pass_multi (several times a from one
                             *    Krylov space) and ll_recur_accum_multi (its replayed step with several accumulators): untyped too;
                             *    also additive under minor 5, with the same note — ll_pauli_expect (expectation values of Pauli
                             *    strings on a state of the basis of (6) or (7)): untyped, the storage type is the operator's;
                             *    also additive under minor 5, with the same note — ll_pauli_rdm (the reduced density matrix of up
                             *    to six sites of such a state, in one sweep): untyped, the storage type is the operator's;
                             *    also additive under minor 5, with the same note — ll_pauli_expect_block (expectation values of
                             *    Pauli strings on a state of a symmetry block (8) - (10)): untyped, the storage type is the operator's;
                             *    also additive under minor 5, with the same note — ll_pauli_block_expand and ll_pauli_block_project
                             *    (a state between a symmetry block (8) - (10) and the basis of (6) or (7)): untyped;
                             *    also additive under minor 5, with the same note — ll_pauli_block_transfer (a sum of Pauli strings
                             *    applied between two momentum blocks (8) or (9)): untyped;
                             *    also additive under minor 5, with the same note — ll_pauli_rdm_tiled (the reduced density matrix of
                             *    4 to 13 sites as a rank-K update on the f64 matrix cores, into host or device memory): untyped;
                             *    also additive under minor 5, with the same note — ll_op_create_pauli_torus (the translation blocks
                             *    of an Lx x Ly torus, kind (11)): ONE untyped entry point, the storage type is an argument;
                             *    ll_pauli_expect_block accepts its operators */

enum {
  LL_OK = 0,
  LL_ERR_INVALID = 1, /* bad argument */
  LL_ERR_HIP = 2,     /* a HIP runtime call failed (or no device) */
  LL_ERR_RCCL = 3,    /* RCCL missing or a collective failed */
  LL_ERR_ALLOC = 4,   /* out of device or host memory */
  LL_ERR_CALLBACK = 5 /* a user callback reported failure */
};

typedef struct ll_context ll_context; /* device + stream + workspace (+ RCCL communicator) */
typedef struct ll_operator ll_operator; /* the mv_mul plugin: device CSR, host callback or device callback */

/* ------------------------------------------------------------------ library / context */

/* Thread-local message of the last failing call on this thread ("" if none). */
const char* ll_last_error(void);
/* LL_VERSION_MAJOR * 1000 + LL_VERSION_MINOR */
int ll_version(void);
/* ABI handshake: pass the LL_VERSION_* the CALLER was compiled with and sizeof(ll_run_stats) / sizeof(ll_lanczos_params) as
 * the caller sees them.  LL_OK when the loaded library lays the structs out the same way; LL_ERR_INVALID (with a message
 * naming both versions) otherwise — the library fills ll_run_stats and reads the parameter structs by ITS layout, so a
 * stale binary would be overrun.  Minors that only ADD entry points accept older callers (any minor from 3 up to the library's
 * own, same struct sizes).  The handshake exists since minor 3: a binary built against an older header never calls it and is
 * not protected — it must be rebuilt.  The C++ facade (both Context constructors) and the Python binding call it once per
 * process. */
int ll_abi_check(int caller_major, int caller_minor, size_t sizeof_run_stats, size_t sizeof_lanczos_params);
#define LL_ABI_CHECK() ll_abi_check(LL_VERSION_MAJOR, LL_VERSION_MINOR, sizeof(ll_run_stats), sizeof(ll_lanczos_params))

/* Create a context on HIP device `device` with its own non-blocking stream. */
int ll_ctx_create(int device, ll_context** out);
/* Same, but enqueue on an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the
 * null stream.  The stream stays owned by the caller. */
int ll_ctx_create_on_stream(int device, void* hip_stream, ll_context** out);
int ll_ctx_destroy(ll_context* ctx);
/* The library's LL_* environment switches are read ONCE, when a context is created, and
 * copied into the operators created on it — never on a launch path.  This reads them again into an existing context
 * (test suites and tuning scripts that flip a switch inside one process); operators that already exist keep theirs. */
int ll_ctx_reload_env(ll_context* ctx);
/* UNSTABLE (tests, probes and A/B measurements; keys may change between minors): set one tuning field of THIS context by key,
 * on top of what the environment said.  The environment carries only the user-facing switches of INTEGRATION.md section 8; block
 * geometries, forced code paths and the hooks of the test suite ("pb_block", "pair_split", "lagged_min_bytes", "tl_force",
 * "force_rp64", ... — the list is INTEGRATION.md section 8, second table) exist only here, so that a stray variable in a user's
 * environment can never change the numerics path.  Every user-facing switch is also a key (its name in lower case without the
 * LL_ prefix: "spmv_kernel", "pair_gs", ...).  value NULL removes the setting again; an unknown key is LL_ERR_INVALID.  Like the
 * environment switches it takes effect for operators / runs created afterwards. */
int ll_ctx_set_tuning(ll_context* ctx, const char* key, const char* value);
/* hipStream_t of the context (for callers that enqueue their own work in between). */
int ll_ctx_stream(ll_context* ctx, void** hip_stream_out);
/* Block until the context's stream is idle. */
int ll_ctx_synchronize(ll_context* ctx);
/* The Krylov-basis slabs of a finished run stay cached in the context so that the next run does not pay
 * hipMalloc/hipFree of tens of GB; this returns them to the device (ll_ctx_destroy does it too). */
int ll_ctx_release_cache(ll_context* ctx);

/* Device-side stopwatch: HIP events recorded on the context's stream (what bench.py uses to time a kernel on the
 * stream it is launched on).  ll_timer_stop waits for the stream and returns the milliseconds since ll_timer_start. */
int ll_timer_start(ll_context* ctx);
int ll_timer_stop(ll_context* ctx, double* ms_out);
/* Streaming ceilings of the device at hand, measured now on the context's stream with two plain kernels over `bytes` (>= 1 MiB;
 * two scratch buffers of that size are allocated and freed): a read-only stream (GB/s of bytes read) and a copy (GB/s of bytes
 * read + written).  bench.py reports its roofline fractions against these next to the 8 TB/s spec peak (SURVEY 8d "Bound"). */
int ll_bandwidth_probe(ll_context* ctx, size_t bytes, double* read_GBps, double* copy_GBps);

/* ------------------------------------------------------------------ multi-GPU
 * One process per GPU.  Rows of A and every n-vector are partitioned 1-D and contiguously:
 * rank r owns rows [row_begin, row_begin + n_local).  The library talks RCCL directly on the context's
 * stream: one all-gather of the current Lanczos vector per SpMV and small all-reduces for the dot products.
 * librccl is loaded lazily (dlopen), single-GPU use needs no RCCL. */

#define LL_UNIQUE_ID_BYTES 128
/* Rank 0 creates the id and distributes the 128 bytes by any host mechanism (MPI, torch.distributed, file). */
int ll_comm_unique_id(void* id_out_128);
/* Collective over all ranks. After it, operators created on this context are row shards. */
int ll_comm_init(ll_context* ctx, const void* id_128, int rank, int n_ranks);
int ll_comm_rank(ll_context* ctx, int* rank, int* n_ranks);
/* ll_comm_init ends with a self-check (every rank's tag through an all-gather on the communication stream, a sum of
 * ones through an all-reduce on the compute stream) and fails with LL_ERR_RCCL when the communicator does not span
 * n_ranks ranks in rank order.  This returns how many rank tags arrived (== n_ranks after a successful init; 1 without
 * a communicator) so that a launcher can print it next to its results. */
int ll_comm_ranks_seen(ll_context* ctx, int* out);
/* Which transport answers this context's collectives, as text: "rccl" (the communicator ll_comm_init created with librccl),
 * "plugin:<path>" (the shared object LL_COMM_PLUGIN named), "attached" (ll_comm_attach) or "none" (no communicator).  A launcher
 * prints it next to ll_comm_ranks_seen: a rank count alone does not say that RCCL ran. */
int ll_comm_transport(ll_context* ctx, char* out, size_t cap);
/* The contiguous row range of `rank`: shards of ceil(n / n_ranks) rows (the last ones may be shorter or empty).
 * Sharded operators and vectors must use exactly these ranges (the all-gather relies on equal shard strides). */
int ll_partition(int64_t n, int n_ranks, int rank, int64_t* row_begin, int64_t* n_local);

/* ------------------------------------------------------------------ device memory helpers */

int ll_malloc(ll_context* ctx, size_t bytes, void** dev_out);
int ll_free(ll_context* ctx, void* dev);
int ll_memcpy_h2d(ll_context* ctx, void* dst_dev, const void* src_host, size_t bytes); /* synchronous */
int ll_memcpy_d2h(ll_context* ctx, void* dst_host, const void* src_dev, size_t bytes); /* synchronous */
int ll_memset(ll_context* ctx, void* dst_dev, int byte, size_t bytes);

/* ------------------------------------------------------------------ the operator plugin: mv_mul (LL:120-126, EX:35-41)
 *
 * Reference contract: std::function<void(const vector<T>& in, vector<T>& out)>, `out` zero-filled on entry,
 * accumulate or overwrite both legal, called once per Lanczos iteration with the unit-norm u[k-1]
 * (LL:242-243, EX:107-108).  Five realisations: */

/* (1) device-resident CSR (the reference ships no sparse format; this is the new operator of SURVEY 8a-a1).
 *     n_rows_local rows [row_begin, row_begin+n_rows_local) of a global n_cols x n_cols symmetric/Hermitian
 *     matrix; column indices are GLOBAL.  Single GPU: row_begin = 0, n_rows_local = n_cols.
 *     row_ptr_host has n_rows_local+1 entries starting at 0.  Host arrays stay owned by the caller and may be
 *     freed after the call; the library keeps device copies until ll_op_destroy. */
int ll_op_create_csr_d(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                       const int64_t* row_ptr_host, const int32_t* col_host, const double* val_host,
                       ll_operator** out);
int ll_op_create_csr_z(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                       const int64_t* row_ptr_host, const int32_t* col_host, const void* val_host /* re,im pairs */,
                       ll_operator** out);
/*     Same with arrays that already live on the device (e.g. built by a GPU generator). */
int ll_op_create_csr_dev_d(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                           const int64_t* row_ptr_dev, const int32_t* col_dev, const double* val_dev,
                           ll_operator** out);
int ll_op_create_csr_dev_z(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                           const int64_t* row_ptr_dev, const int32_t* col_dev, const void* val_dev,
                           ll_operator** out);

/*     {row, col, value} triplets, the format of the reference's sparse sample (src/samples/sample2_sparse.cpp:14-47):
 *     converted to CSR on the host (stable inside a row, duplicates kept as separate entries); single GPU only. */
int ll_op_create_coo_d(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows_host, const int32_t* cols_host,
                       const double* vals_host, ll_operator** out);
int ll_op_create_coo_z(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows_host, const int32_t* cols_host,
                       const void* vals_host, ll_operator** out);
/*     max_i sum_j |a_ij| over the LOCAL rows of a CSR/COO operator created from
 *     host arrays: a safe eigenvalue_offset bound, the idea of src/determine_eigenvalue_offset/
 *     determine_eigenvalue_offset.cpp:12-29 (which does not build upstream).  For "smallest" problems use
 *     eigenvalue_offset = -inf_norm so that the wanted Ritz value is large in magnitude. */
int ll_op_inf_norm(const ll_operator* op, double* out);

/* (2) unmodified user code: a host callback with exactly the reference semantics; costs one D2H + one H2D
 *     of an n-vector per iteration (SURVEY 8b "Operator contract").  Return non-zero from fn to abort. */
typedef int (*ll_host_mv_mul_d)(const double* in, double* out_zeroed, int64_t n, void* user);
typedef int (*ll_host_mv_mul_z)(const void* in, void* out_zeroed, int64_t n, void* user); /* also used by _c */
typedef int (*ll_host_mv_mul_s)(const float* in, float* out_zeroed, int64_t n, void* user);
int ll_op_create_host_d(ll_context* ctx, int64_t n, ll_host_mv_mul_d fn, void* user, ll_operator** out);
int ll_op_create_host_z(ll_context* ctx, int64_t n, ll_host_mv_mul_z fn, void* user, ll_operator** out);

/* (3) a device callback: fn enqueues out += A*in on `hip_stream` for device pointers (out zero-filled). */
typedef int (*ll_dev_mv_mul)(const void* in_dev, void* out_dev_zeroed, int64_t n_local, void* hip_stream,
                             void* user);
int ll_op_create_device_d(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out);
int ll_op_create_device_z(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out);

/* (4) dense row-major matrix, the operator of the reference's first sample and of its small known-answer tests
 *     (src/samples/sample1_simple.cpp:22-28; T1:130, T1:446-453): a_host holds n_rows_local x n_cols values of T,
 *     rows [row_begin, row_begin + n_rows_local) of the global matrix.  Sharded exactly like CSR (row block +
 *     all-gather of x).  One apply streams the matrix once: sizeof(T) * n_rows_local * n_cols bytes. */
int ll_op_create_dense_d(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                         const double* a_host, ll_operator** out);
int ll_op_create_dense_z(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                         const void* a_host, ll_operator** out);

/* (5) matrix-free lattice operator: the family of the reference's "dynamic matrix" sample and tests
 *     (src/samples/sample3_dynamic.cpp:17-22 and T1:265-273: open chain; T2:113-121: periodic ring; BASELINE
 *     config 2: 5-point Laplacian).  Sites of a row-major lattice dims[0] x .. x dims[ndim-1] (LAST index fastest,
 *     n = product of dims);
 *         (A x)(r) = (diag + onsite[r]) x(r) + sum_d ( t_d(r) x(r + e_d) + conj(t_d(r - e_d)) x(r - e_d) ),  t_d = hop[d]
 *     (times a position-dependent Peierls phase when phase_grad is set, see the struct)
 *     with open (periodic[d] = 0: the missing neighbour contributes nothing) or periodic boundaries per dimension.
 *     No matrix is stored: one apply moves 2 * sizeof(T) * n bytes (+ 8n for onsite) instead of the CSR image.
 *     Sharded contexts: flattened sites [row_begin, row_begin + n_local) per ll_partition; the exchange step is a
 *     HALO exchange of one lattice hyperplane (n / dims[0] sites) with the two neighbouring ranks instead of the
 *     all-gather of x; every shard must hold at least one hyperplane.
 *     hop_im must be 0 for the real types.  onsite_host_local: n_local real values, NULL = none; they are kept in the real
 *     type of T (rounded to float for _s / _c) and added to diag in double. */
typedef struct ll_stencil_desc {
  int32_t ndim;        /* 1..3 */
  int32_t periodic[3];
  int64_t dims[3];
  double diag;
  double hop_re[3];
  double hop_im[3];
  /* Peierls phases (complex types only; all 0 = none): the bond r -> r + e_d carries
   *   hop[d] * exp(i * sum_e phase_grad[d][e] * c_e(r)),   c(r) = lattice coordinates of the bond's lower site r,
   * and conj of that in the other direction.  Example (BASELINE config 5, Landau gauge on an N x N torus with dims =
   * {y, x}): hop = {-1, -1}, phase_grad[1][0] = 2 pi 3 / N. */
  double phase_grad[3][3];
} ll_stencil_desc;
int ll_op_create_stencil_d(ll_context* ctx, const ll_stencil_desc* desc, int64_t row_begin, int64_t n_local,
                           const double* onsite_host_local, ll_operator** out);
int ll_op_create_stencil_z(ll_context* ctx, const ll_stencil_desc* desc, int64_t row_begin, int64_t n_local,
                           const double* onsite_host_local, ll_operator** out);

/* (6) matrix-free spin-1/2 Hamiltonian, a sum of Pauli strings: H = sum_t coef_t P_t on n_sites spins, n = 2^n_sites — what the
 *     README's many-body user ("low-energy excitation of a quantum system", exp(-iH dt)) writes as an mv_mul plugin (LL:120-126),
 *     applied on the device from the list of terms instead of from a stored matrix.
 *     Basis state s, 0 <= s < 2^n_sites: BIT j OF s IS SITE j, bit = 0 is sigma_z = +1 (in a Kronecker product site 0 is the LAST
 *     factor).  A term (x_mask, z_mask, coef): site j carries X if only its x bit is set, Z if only its z bit, Y if both, the
 *     identity if none.  With nY = popcount(x_mask & z_mask):  P|s> = i^nY (-1)^popcount(s & z_mask) |s ^ x_mask>, so
 *         (H v)(s) = sum_t coef_t i^nY_t (-1)^popcount((s ^ x_t) & z_t) v(s ^ x_t).
 *     Every Pauli string is Hermitian and coef is real: H is Hermitian by construction.  The real types (_d, _s) take terms with an
 *     EVEN nY only (the matrix is then real symmetric); an odd nY there is LL_ERR_INVALID.  coef is a double for every T.
 *     Examples: a Heisenberg bond J S_j.S_k = (m, 0, J/4), (m, m, J/4), (0, m, J/4) with m = 2^j | 2^k; the transverse-field Ising
 *     chain -J sum Z_j Z_j+1 - h sum X_j = (0, 2^j | 2^(j+1), -J) and (2^j, 0, -h).
 *     n_terms == 0 is the zero operator; duplicate terms add; a term with both masks 0 is a multiple of the identity.
 *     LIMITS: 1 <= n_sites <= 30 (the library's local indices are signed 32-bit: n_local < 2^31 - 1); every mask bit below n_sites;
 *     finite coefficients; a SINGLE-GPU context (more than one rank is refused: the high bits of s would be the rank and flips of
 *     high bits pairwise exchanges — not built).
 *     One apply moves between 2 sizeof(T) n bytes (every partner tile found in cache) and (G + 2) sizeof(T) n, G = the distinct
 *     x masks that touch a site at or above the tile (2^12 states in fp64); the CSR image of the same matrix
 *     moves 12 nnz + 20 n.  The image is the term tables: ll_op_device_bytes is a few hundred bytes.
 *     ACCURACY: component-wise, like the dense and lattice operators — per state the signed coefficients of the terms that share an
 *     x mask are summed in double (masks ascending, a mask's terms in list order), each sum multiplies its partner value in a double
 *     fma (float inputs widened), one rounding to T.  The order is fixed: the same bits run to run and for every tile size.
 *     Queries: ll_op_info reports n = n_local = 2^n_sites and the number of TERMS as nnz_local; ll_op_inf_norm returns
 *     sum_t |coef_t|, an upper BOUND of every absolute row sum (a safe eigenvalue_offset magnitude), not the maximum itself;
 *     ll_op_set_accuracy / ll_op_select_spmv answer LL_ERR_INVALID (not a CSR operator), ll_op_accuracy the component-wise class. */
typedef struct ll_pauli_term {
  uint64_t x_mask, z_mask;
  double coef;
} ll_pauli_term;
int ll_op_create_pauli_d(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_z(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_s(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_c(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);

/* (7) the same sum of Pauli strings on ONE MAGNETISATION SECTOR, for an H that conserves total S_z (Heisenberg, XXZ, J1-J2,
 *     Dzyaloshinskii-Moriya, each with or without a z field) — the space an exact-diagonalisation code works in.
 *     Conventions of (6): bit j of s is site j, a SET bit is sigma_z = -1.  The sector (n_sites, n_down) is the set of states with
 *     popcount(s) = n_down in ASCENDING integer order: state number i is s_i, 0 <= i < D = C(n_sites, n_down), and the operator
 *     acts on vectors of length D,
 *         y(i) = sum_g w_g(s_i) v(rank(s_i ^ X_g)),   over the groups g (distinct x masks X_g) whose s_i ^ X_g lies in the sector,
 *     with the groups, the term order, the folded i^nY and the weights w_g of (6).  rank() is the inverse of i -> s_i.
 *     LIMITS: those of (6) — 1 <= n_sites <= 30, every mask bit below n_sites, finite coefficients, an even nY for the real types,
 *     a single-GPU context — and 0 <= n_down <= n_sites.
 *     CONSERVATION: an H that does not commute with total S_z is refused with LL_ERR_INVALID; the message names the x mask of the
 *     first offending group.  The rule, per group with X_g != 0: over every assignment of the sites the group touches (X_g and
 *     its z masks) for which flipping X_g changes the number of set bits, the weight w_g — summed in the kernel's order, in double —
 *     must be exactly 0.0.  That is exact for the models above (a Heisenberg bond gives c + (-c) on aligned spins) and refuses the
 *     transverse-field Ising chain, a lone XX term, J_x != J_y and every x mask with an odd number of bits that carries weight.  A
 *     group that touches more than 20 sites is refused too: the check visits 2^sites assignments and cannot be made.
 *     The image is the term tables, the D states (4 D bytes) and two rank tables of at most 2^15 entries each
 *     (rank(s) = lo_rank[low bits of s] + hi_rank[the other bits]); ll_op_device_bytes counts them.  One apply moves between
 *     (2 sizeof(T) + 4) D bytes (every gathered partner found in cache) and ((G + 2) sizeof(T) + 4) D, G = the x masks != 0.
 *     ACCURACY: as (6), and more: per state the same fma chain as (6) forms, without the groups that leave the sector (their weight
 *     is exactly 0) — applied to a vector embedded in 2^n_sites zeros, (6) gives the same bits.  The same bits run to run and
 *     for every block size.
 *     Queries: ll_op_info reports n = n_local = D and the number of TERMS as nnz_local; ll_op_inf_norm returns sum_t |coef_t|;
 *     ll_op_set_accuracy / ll_op_select_spmv answer LL_ERR_INVALID (not a CSR operator), ll_op_accuracy the component-wise class. */
int ll_op_create_pauli_sector_d(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms_host,
                                ll_operator** out);
int ll_op_create_pauli_sector_z(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms_host,
                                ll_operator** out);
int ll_op_create_pauli_sector_s(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms_host,
                                ll_operator** out);
int ll_op_create_pauli_sector_c(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms_host,
                                ll_operator** out);

/* (8) the same sum on ONE MOMENTUM BLOCK of one magnetisation sector of a RING, for an H that conserves total S_z and commutes with
 *     the one-site translation T — the next step of an exact-diagonalisation code: each sector splits into n_sites blocks of about
 *     D / n_sites states.  Conventions of (6) and (7).  L = n_sites, momentum = m with 0 <= m < L, that is k = 2 pi m / L.
 *     T rotates a basis state LEFT by one bit: site j goes to site (j + 1) mod L.  The orbit of s is {T^j s}; its length R_s divides
 *     L; its REPRESENTATIVE is its smallest integer.  The basis of block m is the set of representatives r of the sector with
 *     (m R_r) mod L = 0, in ASCENDING integer order, D_m of them, each standing for
 *         |r; m> = N_r^(-1/2) sum_{j=0}^{L-1} e^(-2 pi i m j / L) T^j |r>,     N_r = L^2 / R_r.
 *     With B the D x D_m matrix of these vectors in the basis of (7) — an isometry — THE OPERATOR IS B^H H_sector B, H_sector the
 *     operator of (7).  The sum over m of D_m is D and the union of the blocks' spectra is the sector's.  Equivalent gather form,
 *     which the kernel evaluates: for representative a (number i) and group g let p = a ^ X_g; if p stays in the sector write
 *     p = T^l b with b its representative; if b is in the block,
 *         y(i) += w_g(a) sqrt(R_a / R_b) e^(-2 pi i m l / L) v(number of b),
 *     with w_g the weight of (6) / (7), groups in ascending mask order.
 *     LIMITS: those of (7), and 0 <= momentum < n_sites.  The block is real symmetric only for a real H at 2 m = 0 (mod L): the
 *     real types (_d, _s) take m = 0 and, for even L, m = L / 2 (besides the even-nY rule); _z / _c take every m.
 *     REFUSALS (LL_ERR_INVALID, each naming its cause): momentum outside [0, L); a real type with 2 m mod L != 0; an H that leaves
 *     the sector (the message of (7)); an H that does not commute with T — after merging the coefficients of equal (x_mask, z_mask),
 *     rotating every term's masks by one site must map the term set onto itself with EXACTLY equal coefficients; the message names
 *     the (x_mask, z_mask) of the first term at fault (an open chain is refused this way); an empty block (D_m = 0: n = 0 is not an
 *     operator here); a context of more than one rank.
 *     The image is the term tables, the D_m representatives (4 D_m bytes) and their orbit lengths (D_m bytes), the two rank tables
 *     of (7), two small tables (sqrt(R_a / R_b): 8 KiB; the L phases) and orbit[D]: for EVERY state of the sector 4 bytes that pack
 *     (number of its representative << 5 | l), all ones where the block excludes the orbit — 4 D bytes, e.g. 10.8 MB at L = 24,
 *     n_down = 12 and 620 MB at L = 30, n_down = 15, for a block whose vectors are L times shorter.  ll_op_device_bytes counts all
 *     of it.  One apply moves between (2 sizeof(T) + 5) D_m bytes (every gather found in cache) and
 *     (2 sizeof(T) + 5 + G (sizeof(T) + 4)) D_m, G = the x masks != 0 (per group one orbit entry and one vector element).
 *     ACCURACY: component-wise, as (6): per state and group the weight w_g is summed in double as in (6), multiplied by
 *     sqrt(R_a / R_b) where the two orbit lengths differ (a table entry rounded once) and by the phase where m != 0 (a table entry,
 *     exact on the axes; a complex product in double), and enters the row by one double fma against the partner value (float
 *     inputs widened); one rounding to T.  An entry of the block therefore carries a few double roundings and is in general NOT a
 *     number of the storage type: the single-type contract "products rounded once to T" of the CSR kernels is not claimed here,
 *     only the component-wise class against the exact block.  The order is fixed: the same bits run to run and for every block
 *     size, grid and buffer alignment.
 *     Queries: ll_op_info reports n = n_local = D_m and the number of TERMS as nnz_local; ll_op_inf_norm returns sum_t |coef_t|,
 *     which bounds the 2-norm of H and so EVERY |EIGENVALUE| of the block (B is an isometry) — a safe eigenvalue_offset magnitude;
 *     it is not claimed as a bound of the block's absolute row sums.  ll_op_set_accuracy / ll_op_select_spmv answer LL_ERR_INVALID
 *     (not a CSR operator), ll_op_accuracy the component-wise class. */
int ll_op_create_pauli_momentum_d(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_momentum_z(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_momentum_s(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_momentum_c(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                                  const ll_pauli_term* terms_host, ll_operator** out);

/* (9) the same sum on ONE MOMENTUM BLOCK OF THE FULL 2^n_sites SPACE of a RING, for an H that commutes with the one-site
 *     translation T and need NOT conserve total S_z: the transverse-field Ising ring (the second example of (6), which (7) and (8)
 *     refuse), XYZ rings (J_x != J_y), transverse or tilted fields.  An H that does conserve S_z is accepted too; its block here is
 *     the direct sum over n_down of the blocks of (8).  Conventions of (6) and (8): bit j is site j, T rotates a state LEFT by one
 *     bit, the representative of an orbit is its smallest integer, L = n_sites, k = 2 pi m / L.  The basis of block m is the set of
 *     representatives r of ALL 2^L states with (m R_r) mod L = 0, in ASCENDING integer order, D_m of them (about 2^L / L), each
 *     standing for |r; m> = N_r^(-1/2) sum_{j=0}^{L-1} e^(-2 pi i m j / L) T^j |r>, N_r = L^2 / R_r.  With B the 2^L x D_m matrix of
 *     these vectors — an isometry — THE OPERATOR IS B^H H B, H the operator of (6).  The sum over m of D_m is 2^L and the union of
 *     the blocks' spectra is the spectrum of H.  Equivalent gather form, which the kernel evaluates: for representative a (number i)
 *     and EVERY group g (there is no sector to leave) write a ^ X_g = T^l b with b the representative; if b is in the block,
 *         y(i) += w_g(a) sqrt(R_a / R_b) e^(-2 pi i m l / L) v(number of b),
 *     with w_g the weight of (6), groups in ascending mask order.
 *     LIMITS: those of (6), and 0 <= momentum < n_sites.  The real types (_d, _s) take m = 0 and, for even L, m = L / 2 (besides
 *     the even-nY rule); _z / _c take every m.  D_m < 2^27 - 1 (D_m is about 3.6e7 at L = 30).
 *     REFUSALS (LL_ERR_INVALID, each naming its cause): those of (6); momentum outside [0, L); a real type with 2 m mod L != 0; a
 *     real type with an odd nY; an H that does not commute with T (the rule and the message of (8): the (x_mask, z_mask) of the
 *     first term at fault; an open chain is refused this way); a context of more than one rank.  There is no S_z check, and a block
 *     is never empty: the state 0..01 has R = L, which every m admits (L = 1 has m = 0 only).
 *     The image is O(D_m), with NO table over the 2^L states (the look-up table of (8) would be 4 * 2^L bytes: 4 GiB at L = 30 for
 *     vectors of 3.6e7 elements): the term tables, the D_m representatives (4 D_m bytes) and their orbit lengths (D_m bytes), the
 *     two small tables of (8), and a bucket table over the top bits of a representative — the number of representatives below each
 *     prefix, about D_m / 8 prefixes, at most D_m / 2 bytes.  ll_op_device_bytes counts all of it and stays below
 *     8 D_m + 64 KiB.  The kernel rotates a partner to its representative in registers (L - 1 rotate / compare steps, about 5 L
 *     integer operations per partner) and finds its number by a binary search inside the partner's bucket, whose length is fixed
 *     at creation from the LARGEST bucket (representatives crowd at small integers).  One apply moves between
 *     (2 sizeof(T) + 5) D_m bytes (every gather found in cache) and (2 sizeof(T) + 5 + G (sizeof(T) + 8 + 4 t)) D_m, G = the x
 *     masks != 0 and t the halvings of the search (per group one vector element, two bucket bounds, at most t representatives).
 *     ACCURACY: that of (8), word for word — component-wise against the exact block; w_g summed in double as in (6), times
 *     sqrt(R_a / R_b) where the orbit lengths differ, times the phase where m != 0 (exact on the axes), one double fma per group,
 *     one rounding to T; the same bits run to run and for every block size, grid and buffer alignment.
 *     Queries: ll_op_info reports n = n_local = D_m and the number of TERMS as nnz_local; ll_op_inf_norm returns sum_t |coef_t|, a
 *     bound of EVERY |EIGENVALUE| of the block (B is an isometry), not claimed as a bound of its absolute row sums;
 *     ll_op_set_accuracy / ll_op_select_spmv answer LL_ERR_INVALID (not a CSR operator), ll_op_accuracy the component-wise class. */
int ll_op_create_pauli_momentum_full_d(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_momentum_full_z(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_momentum_full_s(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_momentum_full_c(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms,
                                       const ll_pauli_term* terms_host, ll_operator** out);

/* (10) the same sum on ONE BLOCK OF A RING UNDER MOMENTUM, REFLECTION AND SPIN INVERSION — the state labels k, p, z of exact
 *     diagonalisation — of the full 2^n_sites space (n_down = -1) or of one S_z sector (0 <= n_down <= n_sites).  Conventions of
 *     (6) - (9): bit j is site j, L = n_sites, T rotates a state LEFT by one bit; P is the reflection j -> L - 1 - j (the L bits
 *     reversed); Z is the global flip prod_j X_j (s -> ~s & (2^L - 1)).  All three permute basis states without signs.
 *     parity and inversion are 0 ("this symmetry is not used"), +1 or -1.  The group G is generated by T, by P if parity != 0 and by
 *     Z if inversion != 0: |G| = L, 2 L or 4 L elements T^j P^rho Z^zeta, with the character
 *         chi(T^j P^rho Z^zeta) = e^(-2 pi i m j / L) parity^rho inversion^zeta.
 *     The representative of a G-orbit is its smallest integer; it is admitted iff chi(s) = 1 for every s of its stabiliser and, for
 *     n_down >= 0, iff its popcount is n_down.  The basis is the admitted representatives r in ASCENDING order, D of them, each
 *     standing for |r; chi> = N_r^(-1/2) sum_{g in G} chi(g) g |r>.  With B the matrix of these vectors — an isometry — THE
 *     OPERATOR IS B^H H B, H the operator of (6) (of (7) for n_down >= 0).  On top of momentum 0 or L / 2 the two symmetries cut
 *     the block of (9) by about 2 and 4, and the block stays real symmetric for a real H.  Equivalent gather form, which the kernel
 *     evaluates: for representative a (number i) and every group of terms with x mask X_g write a ^ X_g = g b with b the
 *     representative; if b is in the basis,
 *         y(i) += w_g(a) sqrt(R_a / R_b) chi(g) v(number of b),
 *     R = |G| / |stabiliser| the orbit length (at most 120), w_g the weight of (6), groups in ascending mask order.  With
 *     parity = inversion = 0 and n_down = -1 the result has the same bits as (9).
 *     LIMITS: those of (6); 0 <= momentum < n_sites; D < 2^27 - 1.  parity != 0 needs 2 m mod L = 0 for every type (the group of T
 *     and P has one-dimensional characters only there); the real types (_d, _s) need 2 m mod L = 0 too, besides the even-nY rule.
 *     REFUSALS (LL_ERR_INVALID, each naming its cause): those of (9); parity or inversion outside {0, +1, -1}; parity != 0 with
 *     2 m mod L != 0; an H that does not commute with P (with equal masks merged, reversing the L bits of every term's masks must
 *     map the term set onto itself with exactly equal coefficients: the first term at fault is named; a Dzyaloshinskii-Moriya ring
 *     is refused this way); an H that does not commute with Z (a merged term of odd popcount(z_mask) with a coefficient != 0: a
 *     longitudinal field); n_down outside [-1, L]; n_down >= 0 with an H that does not conserve S_z (the rule and the message of
 *     (7)); n_down >= 0 with inversion != 0 and 2 n_down != L; an EMPTY block (L = 4, m = 0, parity = -1 has D = 0, and so does
 *     L = 6, m = 0, parity = -1, inversion = +1); a context of more than one rank.
 *     The image is O(D), with no table over the 2^L states nor over the sector: the term tables, the D representatives (4 D
 *     bytes), their orbit lengths (D bytes), the bucket table of (9) (at most D / 2 bytes), sqrt(R_a / R_b) for every pair (121^2
 *     doubles) and the L phases.  ll_op_device_bytes counts all of it and stays below 8 D + 192 KiB.  Creation enumerates the
 *     binary necklaces as (9) does and, for each, walks the L rotations of rev(a), ~a and ~rev(a) — whichever are in use — to
 *     decide whether a is the smallest of its G-orbit, to collect its stabiliser and to apply the popcount filter: O(L) per
 *     necklace, O(2^L) steps overall on the host, also for n_down >= 0.  The kernel finds a partner's representative in registers
 *     — L steps over up to four streams, the rotations of p, ~p, rev(p) and ~rev(p): about 6 L integer operations per stream and
 *     partner —, counts the elements that reach it (the stabiliser's size, hence R_b, without a load), finds its number by the
 *     bounded search of (9) and takes it iff the entry found equals it; a partner outside the sector is not found (its weight
 *     is exactly 0 for a conserving H).  UNMEASURED: the apply time, creation time at large L, the block size of the kernel.
 *     ACCURACY: that of (8) and (9) — component-wise against the exact block; w_g summed in double as in (6), times
 *     sqrt(R_a / R_b) where the orbit lengths differ, times the phase where m != 0 (exact on the axes), a sign flip for
 *     parity^rho inversion^zeta = -1 (exact), one double fma per group, one rounding to T; the single-type storage-product contract
 *     is not claimed; the same bits run to run and for every block size, grid and buffer alignment.
 *     Queries: as (9) — ll_op_info reports n = n_local = D and the number of TERMS as nnz_local; ll_op_inf_norm returns
 *     sum_t |coef_t|, a bound of EVERY |EIGENVALUE| of the block; ll_op_set_accuracy / ll_op_select_spmv answer LL_ERR_INVALID,
 *     ll_op_accuracy the component-wise class. */
int ll_op_create_pauli_symmetric_d(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_symmetric_z(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_symmetric_s(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);
int ll_op_create_pauli_symmetric_c(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity,
                                   int32_t inversion, int64_t n_terms, const ll_pauli_term* terms_host, ll_operator** out);

/* (11) the same sum on ONE TRANSLATION BLOCK OF AN Lx x Ly TORUS — the first block outside the ring: square-lattice Heisenberg
 *     and J1-J2 clusters (4 x 4, 6 x 4, 6 x 5), the transverse-field Ising model on a torus — of the full 2^n space (n_down = -1)
 *     or of one S_z sector (0 <= n_down <= n), n = Lx Ly.  UNTYPED: storage is 'd', 'z', 's' or 'c' (the character codes of
 *     ll_recur_accum_scaled), with the meaning of the typed suffixes.  Conventions: site (x, y) is bit x + Lx y.  T_x rotates each
 *     of the Ly fields of Lx bits LEFT by one, site (x, y) -> ((x + 1) mod Lx, y); T_y rotates the n-bit word LEFT by Lx bits,
 *     site (x, y) -> (x, (y + 1) mod Ly).  The group is G = {T_x^a T_y^b}, |G| = n elements, with the character
 *         chi(T_x^a T_y^b) = e^(-2 pi i (mx a / Lx + my b / Ly)),        0 <= mx < Lx, 0 <= my < Ly.
 *     The representative of a G-orbit is its smallest integer; it is admitted iff chi(g) = 1 for every g of its stabiliser and, for
 *     n_down >= 0, iff its popcount is n_down — on a torus the orbit's length alone does not decide that (a stabiliser generated
 *     by a diagonal translation).  The basis is the admitted representatives r in ASCENDING order, D of them (about 2^n / n), each
 *     standing for |r; mx my> = N_r^(-1/2) sum_{g in G} chi(g) g |r>.  With B the matrix of these vectors — an isometry — THE
 *     OPERATOR IS B^H H B, H the operator of (6) (of (7) for n_down >= 0).  Equivalent gather form, which the kernel evaluates:
 *     for representative a (number i) and every group of terms with x mask X_g write a ^ X_g = h b with b the representative; if
 *     b is in the basis,
 *         y(i) += w_g(a) sqrt(R_a / R_b) chi(h) v(number of b),
 *     R = |G| / |stabiliser| the orbit length (at most 30), w_g the weight of (6), groups in ascending mask order.  With Ly = 1
 *     (or Lx = 1) the torus is the ring of (10): the result has the same bits as (10) with parity = inversion = 0, the same
 *     n_down and momentum = mx (my).
 *     LIMITS: lx, ly >= 1 and lx ly <= 30; D < 2^27 - 1.  The real types ('d', 's') need 2 mx mod Lx = 0 and 2 my mod Ly = 0,
 *     besides the even-nY rule; 'z' / 'c' take every (mx, my).
 *     REFUSALS (LL_ERR_INVALID, each naming its cause): those of (6); a storage code other than the four; lx or ly below 1, or
 *     lx ly above 30; mx outside [0, lx) or my outside [0, ly); a real type with 2 mx mod Lx != 0 or 2 my mod Ly != 0; n_down
 *     outside [-1, n]; n_down >= 0 with an H that does not conserve S_z (the rule and the message of (7)); an H that does not
 *     commute with T_x, or with T_y (with equal masks merged, moving every term's masks by one site must map the term set onto
 *     itself with exactly equal coefficients: the direction and the (x_mask, z_mask) of the first term at fault are named; open
 *     boundaries in either direction — an open cylinder — and a ring's Hamiltonian given as a torus are refused this way); an
 *     EMPTY block; a context of more than one rank.
 *     The image is O(D), with no table over the 2^n states nor over the sector: the term tables, the D representatives (4 D
 *     bytes), their orbit lengths (D bytes), the bucket table of (9) (at most D / 2 bytes), sqrt(R_a / R_b) for every pair (32^2
 *     doubles) and the n phases.  ll_op_device_bytes counts all of it and stays below 8 D + 192 KiB.  Creation visits the states
 *     of the space (or of the sector) on the host, on at most 16 threads, leaving each at the first image below it: O(2^n) steps.
 *     The kernel finds a partner's representative in registers — n steps, b outer and a inner, one masked two-shift rotation
 *     each, about 9 integer operations per image and partner —, counts the elements that reach it (the stabiliser's size, hence
 *     R_b, without a load), finds its number by the bounded search of (9) and takes it iff the entry found equals it.
 *     First apply and creation times (6 x 4 and 6 x 5 at half filling): DESIGN.md section 3.1; UNMEASURED: the block size of the
 *     kernel (key pauli_torus_block_bits).
 *     ACCURACY: that of (8) - (10) — component-wise against the exact block; w_g summed in double as in (6), times
 *     sqrt(R_a / R_b) where the orbit lengths differ, times the phase where (mx, my) != (0, 0) (one table entry e^(-2 pi i k / n),
 *     k = (mx a Ly + my b Lx) mod n, exact on the axes), one double fma per group, one rounding to T; the single-type
 *     storage-product contract is not claimed; the same bits run to run and for every block size, grid and buffer alignment.
 *     Queries: as (10) — ll_op_info reports n = n_local = D and the number of TERMS as nnz_local; ll_op_inf_norm returns
 *     sum_t |coef_t|, a bound of EVERY |EIGENVALUE| of the block; ll_op_set_accuracy / ll_op_select_spmv answer LL_ERR_INVALID,
 *     ll_op_accuracy the component-wise class.  ll_pauli_expect_block measures on the block; ll_pauli_block_expand,
 *     ll_pauli_block_project, ll_pauli_block_transfer and the density-matrix entry points answer LL_ERR_INVALID naming this kind
 *     (not built).  Point-group symmetries of the torus, spin inversion on top of it and tilted clusters are not built. */
int ll_op_create_pauli_torus(ll_context* ctx, int32_t storage /* 'd','z','s','c' */, int32_t lx, int32_t ly,
                             int32_t n_down /* -1: full space */, int32_t mx, int32_t my, int64_t n_terms,
                             const ll_pauli_term* terms_host, ll_operator** out);

/* EXPECTATION VALUES OF PAULI STRINGS on a state of the basis of (6) or (7), many per sweep over the state (an addition within
 * minor 5, untyped: the storage type is the operator's).  The kernels read psi and write scalars: no n-sized output vector.
 * With the conventions of (6), P|s> = i^nY (-1)^popcount(s & z) |s ^ x>, observable j = (x_j, z_j, coef_j) is answered
 *     out[j] = coef_j * sum_s Re[ conj(psi(s ^ x_j)) i^nY_j (-1)^popcount(s & z_j) psi(s) ]  =  coef_j Re <psi| P_j |psi>,
 * the sum over all 2^n_sites states for an operator of (6), over the states s_i of the sector whose partner s_i ^ x_j lies in the
 * sector for one of (7) (the partner is found through the operator's rank tables).  NOTHING IS DIVIDED BY <psi|psi>: the term
 * (0, 0, 1) returns ||psi||^2.
 *   op        : from ll_op_create_pauli_* (6) or ll_op_create_pauli_sector_* (7).  It defines the basis and the storage type; the
 *               Hamiltonian's own terms play no part.
 *   obs_host  : n_obs observables (host memory).  n_obs = 0 is valid and touches nothing.  Duplicates are allowed and answered
 *               independently.  Answered exactly +0.0 without a sweep: a string with an odd nY on a real storage type (_d, _s: it
 *               is imaginary and antisymmetric — not refused, unlike a Hamiltonian term of (6)), and in a sector an x mask with an
 *               odd popcount (s ^ x never stays in the sector).
 *   psi       : n_local values of the operator's storage type, host or device memory (decided per pointer, as the two-pass
 *               drivers do).  A device psi needs no n-sized workspace; a host psi is staged into one device vector.  Never modified.
 *   out_host  : n_obs doubles.  The call runs on the context's stream and returns with out_host filled.
 *   sweeps_out: nullable; the passes over psi that were launched: ceil(S / 32), S = the observables that are not identically zero
 *               (they are sorted by x mask and cut into batches of 32 accumulators; a run of equal x masks loads the partner once).
 * REFUSALS (LL_ERR_INVALID, each naming its cause): a null argument (ctx, op; obs_host, psi, out_host with n_obs > 0); a context
 * with a communicator; every other operator kind, named in the message — the symmetry blocks (8) - (10) too: they are measured
 * by ll_pauli_expect_block below; a mask bit at or above n_sites; a coefficient that is not finite.
 * BYTES per sweep, full space: between sizeof(T) n (every partner tile found in cache, or all observables diagonal) and
 * (1 + G_remote) sizeof(T) n, G_remote = the x masks of the batch that touch a bit at or above the tile (2^b states, the key
 * pauli_tile_bits of (6)); a sector: (sizeof(T) + 4) D up to (1 + G) sizeof(T) D + 4 D, G = the batch's x masks other than 0.
 * ACCURACY: every product conj(psi(s ^ x)) psi(s) is formed in double (float inputs widened, exact for _s) and every sum is
 * carried in double — per lane, then one block reduction per accumulator, then a fixed-order fold over the workgroups — so the
 * error is that of a double-accumulated dot product of n terms plus one rounding for coef_j; for a given tile / block size the
 * same bits run to run, for a host and a device psi and for every alignment of psi. */
int ll_pauli_expect(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs_host, const void* psi,
                    double* out_host, int64_t* sweeps_out);

/* ... ON A RING'S SYMMETRY BLOCK: the state is given by its n_local coefficients c on the representatives of a block operator of
 * (8) - (10) (an addition within minor 5, untyped: the storage type is the operator's).  With B the block's isometry and Psi = B c,
 *     out[j] = coef_j Re <Psi| P_j |Psi>          (NOTHING IS DIVIDED BY <c|c> = <Psi|Psi>: the term (0, 0, 1) returns ||c||^2)
 * without Psi ever being formed: Psi transforms by a one-dimensional character of the block's group G (the one-site shift; the
 * reflection iff parity != 0; the global flip iff inversion != 0), so P_j is replaced by its average over G,
 * Pbar_j = (1 / |G|) sum_h h P_j h^-1 — images: both masks rotated / bit-reversed / the sign (-1)^popcount(z) — which commutes
 * with G; the kernel forms sum_a Re[conj(c_a) (Pbar_j c)(a)] with the gather of the operator's own apply, in registers: no n-sized
 * workspace for a device psi, up to 32 observables per sweep over c.
 *   op        : from ll_op_create_pauli_momentum_* (8), _momentum_full_* (9), _symmetric_* (10) or ll_op_create_pauli_torus (11).  It
 *               defines the basis, the group and the storage type; the Hamiltonian's own terms play no part.  For (11) G is the
 *               Lx Ly translations of the torus: both masks moved by the same T_x^a T_y^b, no signs, nothing cancels.
 *   obs_host, psi, out_host: as ll_pauli_expect.  Answered exactly +0.0 without a sweep: an observable all of whose images cancel
 *               (the flip is in use and popcount(z) is odd), an odd nY on a real storage type, and with a fixed S_z sector an x
 *               mask with an odd popcount.  A string that leaves the sector or the block needs no special case.
 *   sweeps_out: nullable; ceil(S / 32), S = the observables that are not identically zero, in the caller's order.
 * REFUSALS (LL_ERR_INVALID, each naming its cause): those of ll_pauli_expect; every operator kind but (8) - (11), named in the
 * message — for (6) and (7) the message points to ll_pauli_expect.
 * ACCURACY: all arithmetic in double (float inputs widened): per state one fma per distinct image string and group, then
 * Re[conj(c_a) .], summed per wave, workgroup and grid in an order that depends on the block size (the tuning key of the
 * operator's apply) and the grid alone: the same bits run to run, for a host and a device psi, for every alignment of psi and
 * wherever an observable stands in the call. */
int ll_pauli_expect_block(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs_host, const void* psi,
                          double* out_host, int64_t* sweeps_out);

/* A STATE BETWEEN A RING'S SYMMETRY BLOCK AND THE FULL SPACE (an addition within minor 5, untyped: the storage type is the
 * operators').  B is the isometry of a block operator of (8) - (10): the row of the state t = g b — b a representative of the
 * block with an orbit of R_b states, g an element of the block's group G — holds val(t) = chi(g) / sqrt(R_b) in the column of b
 * (chi(T^j P^rho Z^zeta) = e^(-2 pi i momentum j / n_sites) parity^rho inversion^zeta); the row of a state whose orbit the block
 * excludes is empty.
 *     ll_pauli_block_expand :  psi_out[t] = val(t) c[col(t)]                                            Psi = B c
 *     ll_pauli_block_project:  c_out[a]   = sum over the orbit of representative a of conj(val(t)) psi[t]     c = B^H Psi
 * project is B^H Psi for ANY Psi, in the block or not: ||c_out||^2 is the weight of Psi in the block, and project(expand(c)) = c.
 * With expand every facility of the full space applies to a block state (ll_pauli_rdm, ll_pauli_expect, an operator that breaks
 * the symmetry); with project a symmetric state of the full space is taken into the block.
 *   block  : from ll_op_create_pauli_momentum_* (8), _momentum_full_* (9) or _symmetric_* (10): the representatives, the group,
 *            the character and the storage type.  Its Hamiltonian's terms play no part.
 *   target : from ll_op_create_pauli_* (6) or ll_op_create_pauli_sector_* (7): the basis of Psi — all 2^n_sites states, or the
 *            states of the sector ascending (its states[] and rank tables are used).  Its terms play no part.
 *            Same context, n_sites and storage type as block.  A sector target needs a block of that n_down ((8), or (10) with
 *            n_down >= 0).  A full-space target takes every block: for a sector block every state outside the sector is written
 *            +0.0 by expand and is not read by project.
 *   c, c_out     : block->n_local values;   psi, psi_out : target->n_local values.  Host or device memory, decided per pointer; a
 *            host buffer is staged through one device vector.  Inputs are never modified.  Every element of the output is written
 *            (a state whose orbit the block excludes: exactly +0.0).  The call returns with the output filled.
 * REFUSALS (LL_ERR_INVALID, each naming its cause, before the device is touched): a null argument; a context with a communicator;
 * a wrong kind for block or target, named in the message; differing contexts, n_sites or storage types; a full-space block ((9),
 * or (10) with n_down < 0) with a sector target; differing n_down; input and output that overlap.
 * ACCURACY: all arithmetic in double (float inputs widened, exact), one rounding to the storage type at the end.
 *   expand : c[col] times the host-formed double 1.0 / sqrt((double)R) (one rounding per component), then times the phase where
 *            momentum != 0 (table entries cos, -sin of the host, exact on the axes), then the sign (exact).  REAL CHARACTER
 *            (2 momentum = 0 mod n_sites: the phases are exactly +-1): one double product, bit for bit (double)c * (+-1 / sqrt(R))
 *            rounded to T.  COMPLEX PHASES: per element |error| <= 16 eps_d |val c| plus the storage rounding, independent of
 *            n_sites — per component the factor (sqrt and division: 2 u, u = eps_d / 2), the scaling (u), the table entry (2 u),
 *            the product (u) and the sum of two (u) make 7 u |val c|, sqrt(2) times that for the modulus: 10 u; a reference that
 *            forms val = phase / sqrt(R) and the complex product in double carries 9 u of its own: 19 u < 32 u = 16 eps_d.
 *   project: the |G| = n_sites (x 2 with parity, x 2 with inversion) terms conj(chi(g)) psi[g a] are formed (a complex phase: two
 *            products and a sum) and summed in double in the order rho, zeta, j of g = T^j P^rho Z^zeta, then multiplied by the
 *            host-formed double sqrt((double)R_a) / (double)|G|: the error of a double-accumulated sum of |G| terms
 *            (2 (|G| + 8) eps_d sum |terms| covers it) plus 4 eps_d for the factor and its product, plus the storage rounding.  With
 *            a real character and a psi of integers the sum S is an exact integer and the result is bit for bit
 *            (double)S * (sqrt((double)R_a) / (double)|G|) rounded to T.
 * No atomics; the same bits run to run, for host and device buffers, for every alignment and for every block size and grid.
 * BYTES: expand writes sizeof(T) N and reads c through a cached gather (plus 4 N of states for a sector target, 4 N of orbit table
 * for (8), about search_trips representatives per state for (9), (10)); project reads sizeof(T) N gathered and writes sizeof(T) D.
 * TIMES: DESIGN.md 3.7 (measured: expand is bound by its integer search, not by bytes).  Block sizes: the unstable tuning keys pauli_block_expand_block_bits (2^b output indices
 * per workgroup block, default 10) and pauli_block_project_block_bits (2^b representatives, default 8). */
int ll_pauli_block_expand(ll_context* ctx, const ll_operator* block, const ll_operator* target, const void* c, void* psi_out);
int ll_pauli_block_project(ll_context* ctx, const ll_operator* block, const ll_operator* target, const void* psi, void* c_out);

/* A SUM OF PAULI STRINGS BETWEEN TWO MOMENTUM BLOCKS OF A RING (an addition within minor 5, untyped: the storage type is the
 * operators').  With B_s, B_t the isometries of two block operators of (8), or of (9) (see ll_pauli_block_expand),
 *     out = B_t^H (sum_j coef_j P_j) B_s c
 * without a vector of the full space: phi = O psi for an operator O that carries momentum q = m_t - m_s (mod n_sites) — the
 * start of a dynamical correlation function (ll_lanczos_two_pass_* with eigvec = NULL, init_vector_dev = phi, eps = 0 and
 * max_iteration = M returns the M-step tridiagonal of (H_target, phi); lambda_lanczos_hip/spectral.hpp holds the continued
 * fraction) and, by its norm, a static structure factor.  THE STRINGS NEED NOT COMMUTE WITH THE TRANSLATION: projecting onto the
 * target block selects their momentum-q component, Z_0 stands for (1 / n_sites) sum_r e^(-2 pi i q r / n_sites) Z_r.
 *   source, target : both from ll_op_create_pauli_momentum_* (8) with equal n_sites and n_down, or both from
 *            ll_op_create_pauli_momentum_full_* (9) with equal n_sites; same context and storage type; source == target is allowed
 *            (q = 0).  Their Hamiltonians' terms play no part.
 *   terms_host : n_terms strings (x_mask, z_mask, real coef), as at creation.  n_terms == 0: out is exactly +0.0, nothing is
 *            launched.  In a sector (8) a string with an odd popcount(x_mask) contributes nothing (no partner stays in the sector).
 *   c : source->n_local values, never modified;  out : target->n_local values, every element written.  Host or device memory,
 *            decided per pointer; a host buffer is staged through one device vector.
 *   norm2_out : nullable; sum |out|^2 of the rounded output in double, formed in the kernel's epilogue (one partial per workgroup,
 *            folded in a fixed order).
 * REFUSALS (LL_ERR_INVALID, each naming its cause, before the device is touched): a null argument; n_terms < 0; a context with a
 * communicator; a block of (10) (a momentum-q operator does not commute with the reflection: that needs semi-momentum states);
 * every other kind; mixed kinds; differing contexts, n_sites, n_down or storage types; a mask bit at or above n_sites or a
 * coefficient that is not finite; a real storage type with a string of an odd number of Y; out overlapping c.
 * ACCURACY: the host merges the images of the strings into weights (the phase e^(2 pi i q j / n_sites), exact on the axes, times
 * coef / period: two roundings per component, and one per merged addition); the kernel forms per x mask the signed sum of the
 * weights, times sqrt(R_a / R_b) where the lengths differ, times the source's phase where m_s != 0, one double fma per x mask in
 * ascending mask order, one rounding to the storage type.  The same bits run to run, for host and device buffers and for every
 * alignment; norm2_out depends on the block size and the grid alone.
 * BYTES and TIMES: DESIGN.md 3.8.  Block sizes: the keys of the target's own apply (pauli_momentum_block_bits,
 * pauli_momentum_full_block_bits). */
int ll_pauli_block_transfer(ll_context* ctx, const ll_operator* source, const ll_operator* target, int64_t n_terms,
                            const ll_pauli_term* terms_host, const void* c, void* out, double* norm2_out);

/* REDUCED DENSITY MATRIX of up to six sites of a state of the basis of (6) or (7), in ONE sweep over the state (an addition
 * within minor 5, untyped: the storage type is the operator's).  The kernels read psi once and write 4^m numbers.
 *     rho[a][a'] = sum_e psi(a, e) conj(psi(a', e)),     m = n_sub, a, a' in [0, 2^m),
 * bit k of the subsystem index a is site sites_host[k]; e runs over the configurations of the other sites (for an operator of (7):
 * over those that leave the state in the sector).  NOTHING IS DIVIDED BY <psi|psi>: the trace is ||psi||^2, as ll_pauli_expect
 * answers the identity.  Tomography through ll_pauli_expect needs 4^m observables = ceil(4^m / 32) sweeps for the same numbers.
 *   op        : from ll_op_create_pauli_* (6) or ll_op_create_pauli_sector_* (7).  It defines the basis and the storage type; the
 *               Hamiltonian's terms play no part.
 *   sites_host: n_sub DISTINCT sites in [0, n_sites), in any order; 1 <= n_sub <= min(6, n_sites).
 *   psi       : n_local values of the operator's storage type, host or device memory (decided per pointer).  A device psi needs
 *               no n-sized workspace; a host psi is staged into one device vector.  Never modified.
 *   out_host  : 2 * 4^m doubles, row-major rho[a][a'] with interleaved (re, im).  The call runs on the context's stream and returns
 *               with out_host filled.  EXACTLY HERMITIAN: the kernels compute a <= a' and the library mirrors — out[a'][a] has the
 *               bits of out[a][a'] in its real part and the negated imaginary part, and every zero imaginary part is +0.0 on both
 *               sides; the diagonal's imaginary parts are +0.0; for real storage (_d, _s) every imaginary part is +0.0.  For an
 *               operator of (7): every entry with popcount(a) != popcount(a') is +0.0 by rule, and so is every row a with
 *               n_down - popcount(a) outside [0, n_sites - m] (no configuration of the other sites completes it).
 *   sweeps_out: nullable; 1 when a kernel ran.  Untouched by a refused call.
 * REFUSALS (LL_ERR_INVALID, each naming its cause, all before the device is touched): a null argument (ctx, op, sites_host, psi,
 * out_host); a context with a communicator; every other operator kind, named in the message — the symmetry blocks (8) - (10)
 * too; n_sub outside 1 .. 6 or above n_sites; a site outside [0, n_sites); a repeated site (the message names its index).
 * BYTES per call, full space: sizeof(T) n — every element of psi is read from memory once, whatever the sites — plus the
 * partials, 8 P G bytes written and read once: P = 3, 10, 40, 160, 576, 2176 doubles per workgroup for m = 1 .. 6 (twice that for
 * complex storage) and G <= 2048 workgroups, lowered so that 8 P G <= 8 MiB (m = 5: 1820 / 910, m = 6: 481 / 240 workgroups for
 * real / complex storage).  A sector: sizeof(T) D gathered through the operator's rank tables (two 4-byte look-ups per element,
 * tables of 4 * 2^(n_sites / 2) bytes: cached) plus the same partials; the 2^(n_sites - m) configurations are enumerated, the
 * empty ones skipped.  The LDS holds 2^t consecutive states times the 2^h tiles that differ in the h subsystem sites at or above t
 * (32 KiB at most; the unstable key pauli_rdm_tile_bits forces t; a sector: 2^b configurations, key pauli_rdm_block_bits).
 * ACCURACY: every product psi(a, e) conj(psi(a', e)) is formed in double (float inputs widened, exact for _s, _c) inside an fma
 * and every sum is carried in double — per thread over the workgroup's rows, then a fixed-order fold inside the workgroup where
 * one entry has several partial owners (m <= 5: 85, 25, 25, 25, 7 row slices), then a fixed-order fold over the workgroups — so
 * each part of each entry meets the bound of a double-accumulated dot product of its two fibres psi(a, .), psi(a', .).  No
 * atomics: for a given tile / block size the same bits run to run, for a host and a device psi and for every alignment of psi. */
int ll_pauli_rdm(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites_host, const void* psi,
                 double* out_host, int64_t* sweeps_out);

/* REDUCED DENSITY MATRIX of 4 to 13 sites — the half chain of a ring of 20 to 26 sites — as a Hermitian rank-K update on the f64
 * matrix cores (an addition within minor 5, untyped: the storage type is the operator's).  The same numbers as ll_pauli_rdm,
 *     rho[a][a'] = sum_e psi(a, e) conj(psi(a', e)),     m = n_sub, a, a' in [0, 2^m),  bit k of a = site sites_host[k],
 * formed as rho = F F^H with F the 2^m x 2^(n_sites - m) matrix of fibres: rho is cut into macro-tiles of 64 x 64, one workgroup
 * per tile of the upper triangle and slice of K stages KC environment configurations at a time in LDS and multiplies them with
 * v_mfma_f64_16x16x4_f64; a finishing kernel folds the slices and writes both triangles.  NOTHING IS DIVIDED BY <psi|psi>.
 *   op        : from ll_op_create_pauli_* (6) or ll_op_create_pauli_sector_* (7), as for ll_pauli_rdm.
 *   sites_host: n_sub DISTINCT sites in [0, n_sites), in any order; 4 <= n_sub <= min(13, n_sites) — from 4 sites on 2^m is a multiple
 *               of the 16-row MFMA tile (m = 4, 5, 6 overlap ll_pauli_rdm on purpose: a cross-check; one macro-tile, zero-padded at
 *               m = 4, 5).  WHY 13: out is 1 GiB there, and above it the eigen-decomposition of rho (O(8^m) on the host) limits the
 *               workflow, not this kernel; half chains of 28 to 30 sites need the singular values of F instead.
 *   psi       : n_local values of the operator's storage type, host or device memory (decided per pointer).  Never modified.
 *   out       : 2 * 4^m doubles, row-major rho[a][a'] with interleaved (re, im), HOST OR DEVICE memory (decided per pointer; a host
 *               out is staged in a device buffer of the same size).  The call returns with out filled.  EXACTLY HERMITIAN, as
 *               ll_pauli_rdm: only a <= a' is computed, out[a'][a] has the bits of out[a][a'] in its real part and the negated
 *               imaginary part, every zero is +0.0; the diagonal's imaginary parts and, for real storage, all of them are +0.0.
 *               For an operator of (7): every entry with popcount(a) != popcount(a') is +0.0 by rule, and so is every row a with
 *               n_down - popcount(a) outside [0, n_sites - m].
 *   sweeps_out: nullable; 1 when the kernels ran.  Untouched by a refused call.
 * REFUSALS (LL_ERR_INVALID, each naming its cause, all before the device is touched): a null argument (ctx, op, sites_host, psi,
 * out); a context with a communicator; every other operator kind, named in the message — the symmetry blocks (8) - (10) with the
 * advice to expand the state (ll_pauli_block_expand) and measure on the target; n_sub outside 4 .. 13 or above n_sites; a site
 * outside [0, n_sites); a repeated site (the message names its index).
 * BYTES per call, full space: psi is read once per macro-tile row and column it enters, nb + 1 times with nb = 2^max(0, m - 6)
 * blocks per side (mostly from the caches: a K-step of a block is read by its nb + 1 tiles at about the same time), plus the
 * partials, 8 P T S bytes written and read once — P = 4096 doubles per macro-tile (8192 for complex storage), T = nb (nb + 1) / 2
 * macro-tiles, S = ksplit slices — plus 32 * 4^m bytes of out.  WORKSPACE: the partials, allocated for the call from the context's
 * buffer cache: S is the smallest power of two with T S >= 512 (twice the CUs) that the K-steps allow and that keeps 8 P T S
 * within 64 MiB (the unstable key pauli_rdm_tiled_ksplit forces S); with S = 1 the partials are the upper triangle of rho, up to
 * 516 MiB at m = 13 in complex storage.  A host psi or out adds its staged copy.  LDS: 4 planes (2 for real storage) of KC x 80
 * doubles, 40 KiB at the default KC = 16 (key pauli_rdm_tiled_kc: 4, 8 or 16).  A sector gathers through the operator's rank
 * tables; the 2^(n_sites - m) configurations are enumerated and the states outside the sector multiplied as zeros.
 * ACCURACY: float inputs are widened to double (exact); every product and sum is formed in double by the matrix core, four
 * environment configurations per instruction, KC per K-step, the K-steps of a slice in ascending order, and the slices are folded
 * in slice order — each part of each entry is held to the bound of a double-accumulated dot product of its two fibres psi(a, .),
 * psi(a', .) by tests/test_gpu_pauli_rdm_tiled.py.  No atomics: for a given (KC, ksplit) the same bits run to run, for a host and
 * a device psi, for a host and a device out and for every alignment of psi. */
int ll_pauli_rdm_tiled(ll_context* ctx, const ll_operator* op, int32_t n_sub, const int32_t* sites_host, const void* psi, void* out,
                       int64_t* sweeps_out);

/* Which SpMV kernel a CSR operator uses (both are bit-reproducible run to run; their results agree to rounding IN THE
 * NORM-WISE SENSE stated below):
 *   LL_SPMV_CSR_STREAM  plain CSR, products staged in LDS; best when the x gathers hit L1/L2 (stencils, narrow bands).
 *   LL_SPMV_PB          propagation blocking: the same matrix re-ordered once at upload (on the device) so that one
 *                       SpMV is two fully coalesced streaming sweeps with x and y slices in LDS and no global gather;
 *                       best for matrices without column locality (BASELINE config 3).  On sharded contexts its
 *                       own-column part runs under the all-gather.
 *   LL_SPMV_TILED       2-D tiling for matrices WITH column locality (bands, stencils, lattices — the operators the reference
 *                       itself ships, sample3_dynamic.cpp:17-22): one workgroup per row block keeps the y slice AND, tile by
 *                       tile, the x slice in LDS and streams 12 B per nonzero (fp64) — no global gather, no product buffer.
 *                       Built only when the row blocks touch few column tiles (a random matrix is not eligible).  Sharded
 *                       contexts launch it twice per product: the row blocks whose tiles all lie inside the rank's own columns
 *                       run under the all-gather, the others when the vector has arrived (ll_op_tiled_layout reports the
 *                       split); the ranks' maxima of |x| travel in an 8-byte all-gather in front of the vector's, so the
 *                       shards stitch to the bits of the single-GPU product.  By default it sums in fixed point like LL_SPMV_PB's default form (same integers: the result does
 *                       not depend on the tiling), i.e. the NORM-wise accuracy class below; with LL_ACCURACY_COMPONENTWISE the same
 *                       image is summed in floating point, the waves of a workgroup adding in turn (a fixed order).
 * ll_op_create_csr_{d,z} and _csr_dev_ build the images, time them on the device with the actual matrix (sharded
 * contexts: summed over the ranks, so every rank takes the same decision), keep the fastest and RELEASE the others
 * (for BASELINE config 3 that returns 1.8 GB of CSR arrays).  Environment: LL_SPMV_KERNEL=csr|pb|tiled skips the timing,
 * LL_SPMV_KEEP_BOTH=1 keeps every image so that ll_op_select_spmv can switch later (A/B timing, tests).
 *
 * ACCURACY of y = A x (this is what replaces the user's fp64 mv_mul, LL:243 / EX:108):
 *   LL_SPMV_CSR_STREAM, and LL_SPMV_PB / LL_SPMV_TILED with floating-point sums (LL_ACCURACY_COMPONENTWISE; LL_PB_PHASE2=ordered|atomic):
 *     |y_i - (A x)_i| <= ~nnz_i * eps * sum_j |a_ij| |x_j|             (COMPONENT-wise, like a plain fp64 row loop).
 *   LL_SPMV_PB and LL_SPMV_TILED in their default form (LL_PB_PHASE2=fixed) round every product to a per-row fixed-point grid and add
 *   64-bit integers (order-independent: same bits for every launch, block geometry and partition of the matrix):
 *     |y_i - (A x)_i| <= 2 eps * sum_j |a_ij| |x_j|  +  nnz_i * 2^-60 * (sum_j |a_ij|) * max_k |x_k|   (NORM-wise)
 *   where max_k runs over the WHOLE input vector and |.| of a complex number is |re| + |im|.  The factor 2 counts the roundings
 *   outside the grid: each product rounded to T (a complex product: up to eps (|ar xr| + |ai xi|) per part), the integer sum
 *   converted back (eps/2), and the first diagonal entry's product, kept outside the streams and added in floating point (eps/2).  For vectors whose entries are of comparable size (Lanczos vectors of
 *   extended states, random vectors) the second term is 2^7 or more times below the first.  For a vector with a huge dynamic
 *   range (x = e_0, a strongly localised state, an entry of 1e20 next to O(1) entries) rows whose terms are all far
 *   below (sum_j |a_ij|) max|x| lose RELATIVE accuracy: their absolute error stays below nnz_i 2^-60 ||A||_inf ||x||_inf, which
 *   is what the Lanczos recurrence and the Exponentiator need (tests/test_gpu_round3.py asserts both bounds and whole
 *   runs from x = e_0 against the real reference), but it is not the component-wise accuracy of an fp64 row loop.
 *   Callers who need that on such vectors ask for LL_ACCURACY_COMPONENTWISE (ll_csr_options.accuracy / ll_op_set_accuracy below;
 *   3-5 % slower); the environment's LL_PB_PHASE2=ordered or LL_SPMV_KERNEL=csr does the same for every operator of a context.
 *   Rows that meet an Inf / NaN are reported as NaN.  float / complex float storage: the product a_ij x_j is rounded to
 *   the storage type once (exactly what a float multiply gives; complex float: each of the four real products and their
 *   difference / sum rounded to float) before it is summed in fixed point / double.  Exceptions, which form every product
 *   EXACTLY in double (fma of the widened operands): CSR-stream's rows of more than 1024 entries (one workgroup strides over
 *   the row), the dense operator (4) and the lattice operator (5).  The row sum is then rounded to T once.
 *   COLUMN-SPLIT FORMS — the one exception to "rounded once".  On a sharded context the CSR-stream operator, and the dense
 *   operator on a rank whose column range starts and ends on 16-byte pieces of the rows, multiply the rank's OWN columns under
 *   the all-gather and add the other ranks' columns in a second kernel (LL_CSR_SPLIT=0: gather first, one kernel, the rule
 *   above).  A row is then TWO partial sums, S_own over the own columns and S_rem over the others, each accumulated in double,
 *   each rounded to T once, and added in T:  y_i = fl_T( fl_T( fl_T(S_own) + fl_T(offset * x_i) ) + fl_T(S_rem) )
 *   — one narrowing and one addition in T more than the unsplit form.  The component-wise class bound above holds unchanged
 *   in every type; for float / complex float the result differs from the unsplit one by up to an ulp of T of the partial
 *   sums (the two forms agree within the class bound, not bit for bit).  CSR-stream's "more than 1024 entries" rule goes by
 *   the row's length in EACH part: a row of 3000 entries with 900 of them over own columns forms those 900 products in the
 *   storage type and the 2100 others exactly.  PB, tiled and lattice operators have no such form: sharded, they round a row
 *   once, and the fixed-point forms stitch to the bits of the single-GPU product (tests/test_gpu_sharded_contracts.py checks
 *   all of this against tests/exact_ref.py, split_storage_bound).
 *   The offset (a2) and alpha (a3) of ll_spmv_*: y_i = fl_T(row sum) + fl_T(offset * x_i), added in T — for float / complex
 *   float the offset is rounded to float first (an offset such as 0.1 is not exact there) and the product and the addition
 *   round in float; alpha = Re<x, y> of the RETURNED (already rounded) y, accumulated in double, so that
 *   |alpha - exact Re<x, y>| <= ~n eps_double sum_i |x_i||y_i| in every type (tests/test_gpu_accuracy_contracts.py checks
 *   these against an exact host reference, tests/exact_ref.py). */
enum { LL_SPMV_CSR_STREAM = 0, LL_SPMV_PB = 1, LL_SPMV_TILED = 2, LL_SPMV_SYM = 3 /* ll_op_create_csr_sym_* only, see below */ };
/* The ACCURACY CLASS above as a per-operator choice of the caller (who knows whether the vectors are localised), not of
 * the environment:
 *   LL_ACCURACY_DEFAULT        what the context's environment says (LL_PB_PHASE2; norm-wise when unset)
 *   LL_ACCURACY_NORMWISE       the order-independent fixed-point sums where the PB kernel is selected (fastest, bit-identical
 *                              for every partition of the matrix); CSR-stream operators are component-wise anyway
 *   LL_ACCURACY_COMPONENTWISE  floating-point sums in a fixed order in every kernel: the accuracy of the user's own fp64
 *                              row loop (LL:120-126), still bit-reproducible run to run, 3-5 % slower on PB operators
 * ll_csr_options carries it (and the kernel choice, and where the arrays live) into ll_op_create_csr_opt_*; an existing
 * operator is moved between the classes by ll_op_set_accuracy (same image, another phase-2 kernel: no rebuild);
 * ll_op_accuracy reports the class of the kernel that is selected now (never LL_ACCURACY_DEFAULT). */
enum { LL_ACCURACY_DEFAULT = 0, LL_ACCURACY_NORMWISE = 1, LL_ACCURACY_COMPONENTWISE = 2 };
typedef struct ll_csr_options {
  int32_t accuracy;          /* LL_ACCURACY_* */
  int32_t kernel;            /* -1: the environment decides (timing of the candidates unless LL_SPMV_KERNEL); LL_SPMV_CSR_STREAM / LL_SPMV_PB /
                              * LL_SPMV_TILED (an error when the matrix is not eligible or has no entries: never a silent fallback) */
  int32_t arrays_on_device;  /* 0: row_ptr / col / val are host arrays (copied); 1: device arrays as in ll_op_create_csr_dev_* */
  int32_t reserved[5];       /* zero */
} ll_csr_options;
int ll_csr_options_default(ll_csr_options* opt); /* {LL_ACCURACY_DEFAULT, -1, 0, zeros}: then identical to ll_op_create_csr_* */
int ll_op_create_csr_opt_d(ll_context* ctx, int64_t n_rows, int64_t n_cols, int64_t row_begin, const int64_t* row_ptr,
                           const int32_t* col, const double* val, const ll_csr_options* opt, ll_operator** out);
int ll_op_create_csr_opt_z(ll_context* ctx, int64_t n_rows, int64_t n_cols, int64_t row_begin, const int64_t* row_ptr,
                           const int32_t* col, const void* val, const ll_csr_options* opt, ll_operator** out);
int ll_op_create_csr_opt_s(ll_context* ctx, int64_t n_rows, int64_t n_cols, int64_t row_begin, const int64_t* row_ptr,
                           const int32_t* col, const float* val, const ll_csr_options* opt, ll_operator** out);
int ll_op_create_csr_opt_c(ll_context* ctx, int64_t n_rows, int64_t n_cols, int64_t row_begin, const int64_t* row_ptr,
                           const int32_t* col, const void* val, const ll_csr_options* opt, ll_operator** out);
/* A symmetric (real types) or Hermitian (complex types) matrix given as ONE stored triangle T (n x n, CSR, global indices):
 *   A = T + T^T - diag(T)   (real),      A = T + T^H - diag(T)   (complex; the diagonal entries are used as given, as the
 *                                                                  full-storage kernels use them).
 * uplo = LL_UPPER: every entry has col >= row; LL_LOWER: col <= row.  An entry on the wrong side of the diagonal, a column out
 * of range or another uplo is LL_ERR_INVALID.  Duplicates are kept (as in the CSR path); rows may be empty.  opt may be NULL
 * (= ll_csr_options_default); arrays_on_device = 1 takes device arrays.
 * Kernel choice (opt->kernel):
 *   -1            LL_SPMV_SYM when the triangle is eligible and the norm-wise class applies (LL_ACCURACY_COMPONENTWISE, or the
 *                 environment's LL_PB_PHASE2=ordered|atomic, asks for floating-point sums, which LL_SPMV_SYM does not have);
 *                 otherwise the full matrix is expanded and created exactly like ll_op_create_csr_opt_* (timing or LL_SPMV_KERNEL).
 *   LL_SPMV_SYM   an error when the triangle is not eligible or the component-wise class is asked for: never a silent fallback.
 *   LL_SPMV_CSR_STREAM / _PB / _TILED: the expanded full matrix with that kernel.
 * LL_SPMV_SYM: one workgroup per row block keeps y of its rows in LDS (64-bit fixed point, the NORM-wise class below: y is
 *   bit-identical to LL_SPMV_PB / LL_SPMV_TILED on the expanded matrix) and streams every stored entry with an end in its rows
 *   — a_ij x_j into row i, conj(a_ij) x_i into row j — with the x window of its rows +- h staged in LDS, where h is the
 *   half-bandwidth of all but at most 1/16 of the entries (the others, e.g. the corners of a periodic band, read x from memory).
 *   ELIGIBLE: h is at most the row block — the largest power of two <= 16384 rows whose accumulators and x window (rows + 2 h
 *   elements) fit the LDS — and h <= 2048, or h <= n / 4, or one row block holds the whole matrix.  Every triangle of
 *   half-bandwidth <= 2048 is eligible for all four types (float: 8192-row blocks, double and complex float: 4096, complex
 *   double: 2048); a random matrix is not.  n is limited to 2^31 - 2 like every CSR operator (32-bit column indices).
 * Creation reads the triangle on the host (device arrays are copied down); for LL_SPMV_SYM the row exponents and ll_op_inf_norm
 * of A are summed there in the order of the expanded rows (increasing column order when the triangle's rows are sorted) and
 * only the one-triangle image goes to the device (about half the full matrix: ll_op_device_bytes); the other kernels get the
 * matrix expanded on the host.
 * Queries: ll_op_info reports the STORED entries as nnz_local; ll_op_inf_norm is the max absolute row sum of A;
 * ll_op_selected_spmv reports LL_SPMV_SYM or the kernel of the expanded image; ll_op_select_spmv can only keep the kernel
 * that was selected (the other images are not built); ll_op_tiled_layout reports (0, 0) and ll_op_autotune_ms_of(LL_SPMV_SYM)
 * -1 (not timed) for a LL_SPMV_SYM operator; ll_op_set_accuracy(LL_ACCURACY_COMPONENTWISE) on it is LL_ERR_INVALID.
 * SHARDED contexts (more than one rank) are refused: a rank's rows of the triangle do not hold its rows of A — create the full
 * matrix with ll_op_create_csr_* there. */
enum { LL_UPPER = 0, LL_LOWER = 1 };
int ll_op_create_csr_sym_d(ll_context* ctx, int64_t n, int uplo, const int64_t* row_ptr, const int32_t* col, const double* val,
                           const ll_csr_options* opt, ll_operator** out);
int ll_op_create_csr_sym_z(ll_context* ctx, int64_t n, int uplo, const int64_t* row_ptr, const int32_t* col, const void* val,
                           const ll_csr_options* opt, ll_operator** out);
int ll_op_create_csr_sym_s(ll_context* ctx, int64_t n, int uplo, const int64_t* row_ptr, const int32_t* col, const float* val,
                           const ll_csr_options* opt, ll_operator** out);
int ll_op_create_csr_sym_c(ll_context* ctx, int64_t n, int uplo, const int64_t* row_ptr, const int32_t* col, const void* val,
                           const ll_csr_options* opt, ll_operator** out);
/* Device bytes the operator's images hold (what its creation allocated and still holds; the context's caches are not counted). */
int ll_op_device_bytes(const ll_operator* op, int64_t* bytes);
int ll_op_set_accuracy(ll_operator* op, int accuracy);        /* LL_ACCURACY_NORMWISE | LL_ACCURACY_COMPONENTWISE */
int ll_op_accuracy(const ll_operator* op, int* accuracy_out);
int ll_op_select_spmv(ll_operator* op, int kind);
int ll_op_selected_spmv(const ll_operator* op, int* kind_out);
/* Milliseconds the creation-time timing measured per kernel on this rank (-1: that kernel was not timed). */
int ll_op_autotune_ms(const ll_operator* op, double* csr_stream_ms, double* pb_ms);
int ll_op_autotune_ms_of(const ll_operator* op, int kind /* LL_SPMV_* */, double* ms);
/* The tiled image's row blocks (0: no tiled image) and how many of them need no column of another rank (all of them on one GPU). */
int ll_op_tiled_layout(const ll_operator* op, int* row_blocks, int* own_column_row_blocks);
int ll_op_destroy(ll_operator* op);
/* Global dimension n, local rows, nnz held locally (0 for callbacks; the number of terms for a sum of Pauli strings). */
int ll_op_info(const ll_operator* op, int64_t* n, int64_t* n_local, int64_t* nnz_local);

/* ------------------------------------------------------------------ hot-path primitives
 * Exposed so that every kernel can be parity-checked on its own.  Vectors are LOCAL shards (n_local elements);
 * scalar results are already all-reduced over ranks when a communicator is attached. */

/* a1+a2+a3: y = A x + offset*x ; if dot_host != NULL also returns Re<x, y> (LL:243-248, EX:108-110).
 * x_dev is the LOCAL shard (the library all-gathers it when sharded). */
int ll_spmv_d(ll_context* ctx, ll_operator* op, const double* x_dev, double* y_dev, double offset,
              double* dot_host);
int ll_spmv_z(ll_context* ctx, ll_operator* op, const void* x_dev, void* y_dev, double offset, double* dot_host);

/* a3: <a,b> = sum conj(a_i) b_i (LA:29-51; conjugate-linear in the FIRST argument).  out_host: 1 double (_d) or
 * re,im (_z). */
int ll_dot_d(ll_context* ctx, int64_t n_local, const double* a_dev, const double* b_dev, double* out_host);
int ll_dot_z(ll_context* ctx, int64_t n_local, const void* a_dev, const void* b_dev, double* out_host_reim);
/* a7: sqrt(Re<v,v>), unscaled (LA:56-60). */
int ll_nrm2_d(ll_context* ctx, int64_t n_local, const double* v_dev, double* out_host);
int ll_nrm2_z(ll_context* ctx, int64_t n_local, const void* v_dev, double* out_host);
/* a8: v *= a (LA:65-72) with a real factor; normalize = nrm2 + scal(1/nrm2) (LA:77-80). */
int ll_scal_d(ll_context* ctx, int64_t n_local, double a, double* v_dev);
int ll_scal_z(ll_context* ctx, int64_t n_local, double a, void* v_dev);
int ll_normalize_d(ll_context* ctx, int64_t n_local, double* v_dev, double* norm_host /* nullable */);
int ll_normalize_z(ll_context* ctx, int64_t n_local, void* v_dev, double* norm_host /* nullable */);
/* a4: w = w - beta*u_prev - alpha*u_cur (LL:251-257, EX:112-118); u_prev_dev may be NULL (k == 1). */
int ll_three_term_d(ll_context* ctx, int64_t n_local, double* w_dev, const double* u_prev_dev,
                    const double* u_cur_dev, double beta, double alpha);
int ll_three_term_z(ll_context* ctx, int64_t n_local, void* w_dev, const void* u_prev_dev, const void* u_cur_dev,
                    double beta, double alpha);
/* One replayed step of the two-pass recurrence (ll_lanczos_two_pass_*), for tests and for callers who write their own loops:
 * y = y - a*x - b*p, then psi = psi + g*y, in one sweep; p_dev may be NULL (first step: y = y - a*x).  a, b, g are real. */
int ll_recur_accum_d(ll_context* ctx, int64_t n_local, double* y_dev, const double* x_dev, const double* p_dev, double a,
                     double b, double g, double* psi_dev);
int ll_recur_accum_z(ll_context* ctx, int64_t n_local, void* y_dev, const void* x_dev, const void* p_dev, double a, double b,
                     double g, void* psi_dev);
/* The same step with a COMPLEX g = g_re + i g_im (the replayed step of ll_expo_two_pass; an addition within minor 5, untyped):
 * storage is 'd', 'z', 's' or 'c' and says what y, x, p and psi hold.  On 'z' and 'c' g is rounded to the storage type and g*y is
 * the complex product; on 'd' and 's' g_im must be 0 (LL_ERR_INVALID otherwise) and the call is ll_recur_accum_d / _s. */
int ll_recur_accum_scaled(ll_context* ctx, int storage, int64_t n_local, void* y_dev, const void* x_dev, const void* p_dev,
                          double a, double b, double g_re, double g_im, void* psi_dev);
/* ... with n_acc accumulators (1 .. LL_EXPO_MULTI_MAX) in the same sweep (the replayed step of ll_expo_two_pass_multi; an addition
 * within minor 5, untyped): y = y - a*x - b*p once, then psi_dev[j] = psi_dev[j] + g_j*y for every j, g_j = g_reim[2j] + i g_reim[2j+1]
 * (imaginary parts must be 0 on 'd' and 's').  Every psi_dev[j] receives the bits ll_recur_accum_scaled gives it on its own.  The
 * accumulators must not overlap each other, y, x or p. */
enum { LL_EXPO_MULTI_MAX = 16 };
int ll_recur_accum_multi(ll_context* ctx, int storage, int64_t n_local, void* y_dev, const void* x_dev, const void* p_dev,
                         double a, double b, int64_t n_acc, const double* g_reim /* host, 2*n_acc */,
                         void* const* psi_dev /* host array of n_acc device pointers */);
/* a5+a6+a7: orthogonalise w against nb orthonormal vectors stored row-major with leading dimension ld
 * (vector j at basis_dev + j*ld elements) and return ||w|| afterwards (LA:132-144 at LL:259-262, EX:121,145).
 * mode: LL_ORTH_CGS_DGKS (default, block classical Gram-Schmidt + a second pass when the norm drops below
 * 1/sqrt(2)), LL_ORTH_CGS2 (always two passes), LL_ORTH_MGS (sequential dot->axpy per vector: the reference's
 * operation order, 2*nb launches). h_host (nullable) receives the nb projection coefficients summed over passes
 * (re,im pairs for _z).  Elements [n_local, ld) of a row, and rows beyond nb, are neither read nor written: they may hold
 * anything (NaN included). */
enum { LL_ORTH_CGS_DGKS = 0, LL_ORTH_CGS2 = 1, LL_ORTH_MGS = 2 };
int ll_orth_block_d(ll_context* ctx, int64_t n_local, int64_t nb, const double* basis_dev, int64_t ld,
                    double* w_dev, int mode, double* norm_host, double* h_host);
int ll_orth_block_z(ll_context* ctx, int64_t n_local, int64_t nb, const void* basis_dev, int64_t ld, void* w_dev,
                    int mode, double* norm_host, double* h_host);
/* a9+a10: out_r = sum_{k=m-1..0} coeff[r*m + k] * basis_k for r < nout in ONE pass over the basis
 * (the sums are carried in double / complex double for every type and rounded to T once; the _s / _c coefficients stay double)
 * (LL:51-57: Ritz vectors, real coefficients; EX:166-170: exp(aA)v, coefficients of type T).
 * coeff_host: nout*m values of type T (re,im pairs for _z).  out_dev: nout vectors, leading dimension ld_out.
 * Elements [n_local, ld) of a basis row, and rows beyond m, are neither read nor written (they may hold anything, NaN
 * included); elements [n_local, ld_out) of an output row are not written. */
int ll_gemv_basis_d(ll_context* ctx, int64_t n_local, int64_t m, const double* basis_dev, int64_t ld, int64_t nout,
                    const double* coeff_host, double* out_dev, int64_t ld_out);
int ll_gemv_basis_z(ll_context* ctx, int64_t n_local, int64_t m, const void* basis_dev, int64_t ld, int64_t nout,
                    const double* coeff_host_reim, void* out_dev, int64_t ld_out);

/* a11 (host, TRI:290-361): all eigenvalues (ascending) and optionally eigenvectors (q_host row-major m*m,
 * row j = eigenvector j, nullable) of the symmetric tridiagonal T(alpha[0..m), beta[0..m-1)).
 * Returns the reference's "unconverged" count through unconverged_out (nullable). */
int ll_tridiag_eig(int64_t m, const double* alpha_host, const double* beta_host, double* ev_host, double* q_host,
                   int64_t* unconverged_out);
/* k-th smallest eigenvalue (k = 0 .. m-1) by Sturm bisection (TRI:22-88, find_mth_eigenvalue); what
 * LL_TRIDIAG_BISECT / LL_TRIDIAG_AUTO use for the per-iteration stop test. */
int ll_tridiag_bisect(int64_t m, const double* alpha_host, const double* beta_host, int64_t k, double* out);
/* The same for nk roots ks[0..nk) in one call: bit-identical to nk calls of ll_tridiag_bisect, but the Sturm recurrences
 * of the roots run interleaved (the recurrence is bound by the latency of its division), ~5x faster.  This is what the
 * per-iteration stop test of LL_TRIDIAG_AUTO uses for the nroot tracked Ritz values. */
int ll_tridiag_bisect_multi(int64_t m, const double* alpha_host, const double* beta_host, int64_t nk,
                            const int64_t* ks, double* out_nk);
/* Unit eigenvectors for nw given eigenvalues by inverse iteration, O(m) each (out_host: nw rows of m entries); what
 * LL_TRIDIAG_AUTO uses for the final Ritz step when m > 256 instead of accumulating all m vectors (LL:44, O(m^3)). */
int ll_tridiag_eigvecs(int64_t m, const double* alpha_host, const double* beta_host, int64_t nw,
                       const double* lambdas_host, double* out_host);

/* ------------------------------------------------------------------ whole-loop entry points */

/* Start-vector hook (LL:133 init_vector): fill the LOCAL shard vec_host[0..n_local) holding global rows
 * [row_begin, row_begin+n_local) (re,im pairs for _z).  Called once per restart pass (LL:231-232).
 * NULL = the reference's default: nondeterministic uniform [-1,1] (LL:70-104). */
typedef void (*ll_init_vector_fn)(void* vec_host, int64_t n_local, int64_t row_begin, void* user);

/* LL_TRIDIAG_QR: the reference's implicit-shift QR of all k Ritz values every iteration (O(k^2), TRI:290-361).
 * LL_TRIDIAG_BISECT: Sturm bisection of the nroot wanted values only (O(k), TRI:22-88).
 * LL_TRIDIAG_AUTO: QR up to k = 64, bisection beyond, and the reference's QR arithmetic decides whenever a root's
 *   change comes within 4*eps of the stop threshold: same iteration counts and eigenvalues as LL_TRIDIAG_QR; few Ritz
 *   vectors by inverse iteration once k > 256.  Recommended for runs of more than a few hundred iterations. */
enum { LL_TRIDIAG_QR = 0, LL_TRIDIAG_BISECT = 1, LL_TRIDIAG_AUTO = 2 };

typedef struct ll_lanczos_params {
  /* --- the reference's public fields, same meaning and defaults (LL:126-181) --- */
  int64_t matrix_size;            /* LL:136  global n */
  int64_t max_iteration;          /* LL:138,206  default n */
  double eps;                     /* LL:150  default 1e3 * DBL_EPSILON */
  int32_t find_maximum;           /* LL:153 */
  int32_t reserved0;
  int64_t num_eigs;               /* LL:156  default 1 */
  double eigenvalue_offset;       /* LL:165  default 0 */
  int64_t num_eigs_per_iteration; /* LL:173  default 5 */
  int64_t initial_vector_size;    /* LL:181  default 200 — initial capacity (vectors) of the device basis slab */
  /* --- additions (0 = reference-faithful behaviour) --- */
  int32_t tridiag_mode;           /* LL_TRIDIAG_*: how the per-iteration Ritz values (LL:267-268) are obtained */
  int32_t orth_mode;              /* LL_ORTH_* */
  ll_init_vector_fn init_vector;  /* LL:133 */
  void* init_user;
  const void* init_vector_dev;    /* non-NULL: the start vector (n_local elements) is already in DEVICE memory; used
                                   * instead of the hook in every pass, copied, never modified */
} ll_lanczos_params;

/* Fill *p with the reference defaults for an n x n problem (LL:200-208); tridiag_mode = LL_TRIDIAG_AUTO (same stop
 * decisions and values as the reference's per-iteration QR).  eps is the DOUBLE default 1e3 * DBL_EPSILON (LL:150 with
 * real_t<T> = double); the reference scales it with the epsilon of real_t<T>, so the _s / _c entry points replace
 * exactly that value by 1e3 * FLT_EPSILON (likewise ll_expo_params_default's 1e2 * DBL_EPSILON, EX:58) — a float run
 * left at the defaults converges like the reference's float instantiation instead of iterating to max_iteration. */
int ll_lanczos_params_default(ll_lanczos_params* p, int64_t n, int find_maximum, int64_t num_eigs);

typedef struct ll_run_stats {
  int64_t n_passes;         /* restart passes = getIterationCounts().size() (LL:412-414) */
  int64_t total_iterations; /* sum of the iteration counts */
  double seconds_total;     /* wall time of the call */
  double seconds_host_tridiag; /* host time spent in the tridiagonal eigen-solver (a11/a12) */
  double seconds_spmv;      /* device time inside the operator (HIP events; 0 unless ll_ctx_set_profiling) */
  double seconds_orth;      /* device time in three-term + orthogonalisation + norm + scale */
  int64_t last_alpha_len;   /* entries written to alpha_out/beta_out (last pass) */
  double seconds_host_enqueue; /* host time spent enqueuing device work inside the loop */
  double seconds_host_wait;    /* host time spent waiting for the per-iteration scalars */
  double seconds_setup;        /* start vector, locked vectors (per pass) */
  double seconds_finish;       /* Ritz step: tridiagonal eigenvectors, GEMV over the basis, copy back */
  int64_t second_passes;       /* iterations whose Gram-Schmidt was repeated (DGKS test decided on the host) */
  double seconds_comm_gather;    /* device time of the all-gathers / halo exchanges (their own stream; 0 unless profiling) */
  double seconds_comm_allreduce; /* device time of the all-reduces (0 unless profiling) */
  int64_t lagged_iterations;     /* iterations that ran in the one-sweep (lagged) Gram-Schmidt form */
  int64_t pair_iterations;       /* ... of which: iterations that shared ONE sweep over the basis with their neighbour (two
                                  * iterations per sweep; taken from the reserved tail: same struct size) */
  int64_t pair_gate_trips;       /* times a pass left the two-iterations-per-sweep form because a coefficient of a raw vector
                                  * exceeded its gate (exhausted Krylov space / breakdown): 0 in ordinary runs */
  int64_t workspace_vectors;     /* ll_lanczos_two_pass_*: n-sized device vectors the call allocated (3 or 4, whatever the iteration
                                  * count; taken from the reserved tail like the two above) */
  int64_t replay_mismatches;     /* ll_lanczos_two_pass_*: replayed iterations whose alpha differed, as bits, from the recorded
                                  * one: 0 unless the operator is not reproducible from call to call */
  int64_t reserved[4];           /* later statistics are taken from here, so the struct size stays what it is.  In use, unnamed:
                                  * [0] block_iterations: iterations that ran in the raw-basis block form (up to eight per sweep,
                                  * DESIGN.md 3.2; pair_iterations counts those of them that shared a sweep),
                                  * [1] block_flushed_vectors: raw vectors completed in place when a pass left that form (one
                                  * multi-axpy over the basis each; 0 in ordinary runs),
                                  * [2] block8_iterations: ... of block_iterations, those that ran eight to a sweep (real double, where the guard
                                  * of DESIGN.md 3.2 admitted them; 0 in complex double and with the tuning key block_gs_max = 4).  The rest is zero. */
} ll_run_stats;
int ll_ctx_set_profiling(ll_context* ctx, int enabled);

/* LambdaLanczos<T>::run(eigenvalues, eigenvectors) (LL:330-366): restart loop + EigenPairManager semantics.
 *   eigvals_host   : num_eigs doubles, comparator order (descending for find_maximum, else ascending; LL:362-365)
 *   eigvecs_host   : num_eigs * n_local values of T, row-major, LOCAL shard of each eigenvector (nullable).
 *                    Despite the name the buffer may live in HOST or in DEVICE memory (ll_malloc / hipMalloc); a
 *                    device buffer receives the Ritz vectors without crossing PCIe (with p->init_vector_dev the whole
 *                    call then moves nothing n-sized over the bus).  The same holds for ll_lanczos_run_iteration_*.
 *   n_found        : number of pairs returned (<= num_eigs)
 *   iter_counts    : capacity iter_cap entries (getIterationCounts, LL:412); nullable
 *   alpha_out/beta_out : optional traces of the LAST pass (capacity max_iteration each); nullable
 */
int ll_lanczos_run_d(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals_host,
                     double* eigvecs_host, int64_t* n_found, int64_t* iter_counts, int64_t iter_cap,
                     double* alpha_out, double* beta_out, ll_run_stats* stats);
int ll_lanczos_run_z(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals_host,
                     void* eigvecs_host, int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out,
                     double* beta_out, ll_run_stats* stats);

/* LambdaLanczos<T>::run_iteration(eigvalues, eigvecs, nroot, orthogonalizeTo) (LL:216-322): ONE Lanczos pass that
 * tracks `nroot` Ritz pairs, with every Lanczos vector orthogonalised against the caller's n_orth vectors first
 * (LL:233,259).  No restart loop, no EigenPairManager: every computed pair comes back, in comparator order.
 *   orth_host      : n_orth * n_local values of T (vector j at orth_host + j*n_local; LOCAL shards); NULL if n_orth = 0
 *   eigvals_host   : capacity nroot doubles;  eigvecs_host: capacity nroot * n_local values of T (nullable)
 *   n_found        : pairs returned = min(nroot, iterations done) (LL:264,312)
 *   itern_out      : the method's return value, the Lanczos-iteration count
 * p->num_eigs and p->num_eigs_per_iteration are ignored; every other field acts as in ll_lanczos_run_*. */
int ll_lanczos_run_iteration_d(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const double* orth_host, double* eigvals_host, double* eigvecs_host,
                               int64_t* n_found, int64_t* itern_out, double* alpha_out, double* beta_out,
                               ll_run_stats* stats);
int ll_lanczos_run_iteration_z(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const void* orth_host, double* eigvals_host, void* eigvecs_host,
                               int64_t* n_found, int64_t* itern_out, double* alpha_out, double* beta_out,
                               ll_run_stats* stats);

/* The extreme eigenpair WITHOUT a stored Krylov basis (two-pass Lanczos): pass 1 runs the plain three-term recurrence with the
 * stop and breakdown tests of ll_lanczos_run_* and records its coefficients; pass 2 replays it and accumulates the Ritz vector.
 * Device memory: 3 n-sized vectors (no eigenvector wanted, or eigvec in device memory: the Ritz vector is accumulated there) or 4,
 * whatever the iteration count, against one vector per iteration for ll_lanczos_run_*; every operator application runs twice.
 * There is no re-orthogonalisation, so only the EXTREME pair (lowest, or highest with find_maximum) is trustworthy:
 * p->num_eigs must be 1 (LL_ERR_INVALID otherwise); orth_mode, num_eigs_per_iteration and initial_vector_size are ignored.
 * Single rank only: a context with a communicator is refused with LL_ERR_INVALID.
 *   eigval_out     : the eigenvalue (eigenvalue_offset removed)
 *   eigvec         : n_local values of T in HOST or DEVICE memory; NULL: no eigenvector, no second pass
 *   itern_out      : Lanczos iterations of pass 1 (nullable)
 *   residual_out   : ||(A + offset) psi - theta psi|| from one more operator application (nullable; NaN without eigvec)
 *   alpha_out/beta_out : the tridiagonal (capacity max_iteration each); nullable
 * p->init_vector is called once per call; p->init_vector_dev is read twice and never modified. */
int ll_lanczos_two_pass_d(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval_out, double* eigvec,
                          int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats);
int ll_lanczos_two_pass_z(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval_out, void* eigvec,
                          int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats);

typedef struct ll_expo_params {
  /* the reference's public fields (EX:41-71) */
  int64_t matrix_size;         /* EX:44 */
  int64_t max_iteration;       /* EX:46,81  default n */
  double eps;                  /* EX:58  default 1e2 * DBL_EPSILON */
  int32_t full_orthogonalize;  /* EX:63  default false */
  int32_t orth_mode;           /* LL_ORTH_* used when full_orthogonalize */
  int64_t initial_vector_size; /* EX:71  default 200 */
} ll_expo_params;
int ll_expo_params_default(ll_expo_params* p, int64_t n);

/* Exponentiator<T>::run(a, input, output) (EX:87-173): output = exp(a*A) input; returns the iteration count
 * through itern_out.  input/output are LOCAL shards (n_local values of T) in HOST or in DEVICE memory (decided per
 * pointer): a time-evolution loop psi <- exp(a*A) psi that keeps psi in device buffers never crosses PCIe.  input and
 * output may be the same buffer.  The same holds for ll_expo_taylor_run_*. */
int ll_expo_run_d(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const double* input_host,
                  double* output_host, int64_t* itern_out, ll_run_stats* stats);
int ll_expo_run_z(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                  const void* input_host, void* output_host, int64_t* itern_out, ll_run_stats* stats);
/* Exponentiator<T>::taylor_run (EX:175-210). */
int ll_expo_taylor_run_d(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a,
                         const double* input_host, double* output_host, int64_t* nterms_out);
int ll_expo_taylor_run_z(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                         const void* input_host, void* output_host, int64_t* nterms_out);

/* Exponentiator<T>::run WITHOUT a stored Krylov basis (two-pass form; an addition within minor 5, untyped: the storage type is the
 * operator's, and a is always passed as (a_re, a_im) — a_im != 0 with a real operator is LL_ERR_INVALID).  With the reference's
 * default full_orthogonalize = false, EX:107-118 is the plain three-term recurrence: pass 1 runs it on three rotating vectors with
 * the stop rule of EX:124-158 and records its coefficients, pass 2 replays it bit for bit and accumulates
 * output = ||input|| sum_l coeff[l] u_l (EX:163-170) directly.  Device memory: 3 n-sized vectors when output is device memory
 * (output == input included), 4 when it is host memory, whatever the iteration count, against one vector per iteration plus one
 * for ll_expo_run_*; every operator application runs twice.  The results agree with ll_expo_run_* to rounding.
 *   p->full_orthogonalize != 0 is refused with LL_ERR_INVALID (there is no basis to orthogonalise against); orth_mode and
 *   initial_vector_size are ignored; max_iteration and eps act as in ll_expo_run_*.
 *   input / output : n_local values of the operator's storage type, HOST or DEVICE memory, decided per pointer; they may be the
 *                    same buffer; input is never modified unless it is also the output.
 *   stats          : nullable; n_passes = 1, total_iterations, workspace_vectors (3 or 4), replay_mismatches and the timing fields
 *                    ll_lanczos_two_pass_* fills.
 * Single rank only: a context with a communicator is refused with LL_ERR_INVALID. */
int ll_expo_two_pass(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im, const void* input,
                     void* output, int64_t* itern_out, ll_run_stats* stats);
/* ... for n_times values of a (1 .. LL_EXPO_MULTI_MAX) from ONE Krylov space (an addition within minor 5, untyped): outputs[j] =
 * exp(a_j A) input with a_j = a_reim[2j] + i a_reim[2j+1].  The Krylov space of (A, input) does not depend on a: pass 1 runs once,
 * with the stop rule of EX:124-158 applied to every a_j on its own; where a_j's test fires first, after m_j iterations, its
 * coefficients exp(a_j T_{m_j}) e_1 are frozen, and pass 1 ends when the last a_j has fired (or on breakdown, or at max_iteration,
 * which end every a_j that is still open).  Pass 2 replays max_j m_j - 1 iterations once and adds each replayed vector into the
 * outputs whose m_j it is still below; an output past its m_j is not touched.  On a device operator outputs[j] and itern_out[j] are
 * bit for bit what ll_expo_two_pass returns for a_j alone, for 2 max_j m_j - 1 operator applications instead of sum_j (2 m_j - 1).
 *   outputs   : host array of n_times pointers, each to n_local values in HOST or DEVICE memory, decided per pointer; pairwise
 *               non-overlapping (LL_ERR_INVALID otherwise); one of them may be the input's buffer; the input is otherwise never
 *               modified.  Device memory: 3 n-sized vectors plus one per output in host memory.
 *   itern_out : nullable; n_times values m_j.
 *   stats     : nullable; as ll_expo_two_pass, with total_iterations = max_j m_j and workspace_vectors = 3 + host outputs.
 * Parameters, refusals (full_orthogonalize, a communicator, an imaginary part on a real operator, a zero input) and everything
 * else as ll_expo_two_pass. */
int ll_expo_two_pass_multi(ll_context* ctx, ll_operator* op, const ll_expo_params* p, int64_t n_times,
                           const double* a_reim /* host, 2*n_times */, const void* input,
                           void* const* outputs /* host array of n_times pointers */,
                           int64_t* itern_out /* n_times values m_j, nullable */, ll_run_stats* stats);

/* ------------------------------------------------------------------ float storage types (_s float, _c complex float)
 * Same entry points as above; see the comments on the _d / _z versions. */
int ll_op_create_csr_c(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                       const int64_t* row_ptr_host, const int32_t* col_host, const void* val_host ,
                       ll_operator** out);
int ll_op_create_csr_s(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                       const int64_t* row_ptr_host, const int32_t* col_host, const float* val_host ,
                       ll_operator** out);
int ll_op_create_csr_dev_c(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                           const int64_t* row_ptr_dev, const int32_t* col_dev, const void* val_dev,
                           ll_operator** out);
int ll_op_create_csr_dev_s(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                           const int64_t* row_ptr_dev, const int32_t* col_dev, const float* val_dev,
                           ll_operator** out);
int ll_op_create_coo_c(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows_host, const int32_t* cols_host,
                       const void* vals_host, ll_operator** out);
int ll_op_create_coo_s(ll_context* ctx, int64_t n, int64_t nnz, const int32_t* rows_host, const int32_t* cols_host,
                       const float* vals_host, ll_operator** out);
int ll_op_create_host_c(ll_context* ctx, int64_t n, ll_host_mv_mul_z fn, void* user, ll_operator** out);
int ll_op_create_host_s(ll_context* ctx, int64_t n, ll_host_mv_mul_s fn, void* user, ll_operator** out);
int ll_op_create_device_c(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out);
int ll_op_create_device_s(ll_context* ctx, int64_t n, ll_dev_mv_mul fn, void* user, ll_operator** out);
int ll_op_create_dense_c(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                         const void* a_host, ll_operator** out);
int ll_op_create_dense_s(ll_context* ctx, int64_t n_rows_local, int64_t n_cols, int64_t row_begin,
                         const float* a_host, ll_operator** out);
int ll_op_create_stencil_c(ll_context* ctx, const ll_stencil_desc* desc, int64_t row_begin, int64_t n_local,
                           const double* onsite_host_local, ll_operator** out);
int ll_op_create_stencil_s(ll_context* ctx, const ll_stencil_desc* desc, int64_t row_begin, int64_t n_local,
                           const double* onsite_host_local, ll_operator** out);
int ll_spmv_c(ll_context* ctx, ll_operator* op, const void* x_dev, void* y_dev, double offset, double* dot_host);
int ll_spmv_s(ll_context* ctx, ll_operator* op, const float* x_dev, float* y_dev, double offset, double* dot_host);
int ll_dot_c(ll_context* ctx, int64_t n_local, const void* a_dev, const void* b_dev, double* out_host_reim);
int ll_dot_s(ll_context* ctx, int64_t n_local, const float* a_dev, const float* b_dev, double* out_host_reim);
int ll_nrm2_c(ll_context* ctx, int64_t n_local, const void* v_dev, double* out_host);
int ll_nrm2_s(ll_context* ctx, int64_t n_local, const float* v_dev, double* out_host);
int ll_scal_c(ll_context* ctx, int64_t n_local, double a, void* v_dev);
int ll_scal_s(ll_context* ctx, int64_t n_local, double a, float* v_dev);
int ll_normalize_c(ll_context* ctx, int64_t n_local, void* v_dev, double* norm_host );
int ll_normalize_s(ll_context* ctx, int64_t n_local, float* v_dev, double* norm_host );
int ll_three_term_c(ll_context* ctx, int64_t n_local, void* w_dev, const void* u_prev_dev, const void* u_cur_dev,
                    double beta, double alpha);
int ll_three_term_s(ll_context* ctx, int64_t n_local, float* w_dev, const float* u_prev_dev, const float* u_cur_dev,
                    double beta, double alpha);
int ll_recur_accum_c(ll_context* ctx, int64_t n_local, void* y_dev, const void* x_dev, const void* p_dev, double a, double b,
                     double g, void* psi_dev);
int ll_recur_accum_s(ll_context* ctx, int64_t n_local, float* y_dev, const float* x_dev, const float* p_dev, double a, double b,
                     double g, float* psi_dev);
int ll_orth_block_c(ll_context* ctx, int64_t n_local, int64_t nb, const void* basis_dev, int64_t ld, void* w_dev,
                    int mode, double* norm_host, double* h_host);
int ll_orth_block_s(ll_context* ctx, int64_t n_local, int64_t nb, const float* basis_dev, int64_t ld, float* w_dev,
                    int mode, double* norm_host, double* h_host);
int ll_gemv_basis_c(ll_context* ctx, int64_t n_local, int64_t m, const void* basis_dev, int64_t ld, int64_t nout,
                    const double* coeff_host_reim, void* out_dev, int64_t ld_out);
int ll_gemv_basis_s(ll_context* ctx, int64_t n_local, int64_t m, const float* basis_dev, int64_t ld, int64_t nout,
                    const double* coeff_host_reim, float* out_dev, int64_t ld_out);
int ll_lanczos_run_c(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals_host,
                     void* eigvecs_host, int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out,
                     double* beta_out, ll_run_stats* stats);
int ll_lanczos_run_s(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigvals_host,
                     float* eigvecs_host, int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out,
                     double* beta_out, ll_run_stats* stats);
int ll_lanczos_run_iteration_c(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const void* orth_host, double* eigvals_host, void* eigvecs_host,
                               int64_t* n_found, int64_t* itern_out, double* alpha_out, double* beta_out,
                               ll_run_stats* stats);
int ll_lanczos_run_iteration_s(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, int64_t nroot,
                               int64_t n_orth, const float* orth_host, double* eigvals_host, float* eigvecs_host,
                               int64_t* n_found, int64_t* itern_out, double* alpha_out, double* beta_out,
                               ll_run_stats* stats);
int ll_lanczos_two_pass_c(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval_out, void* eigvec,
                          int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats);
int ll_lanczos_two_pass_s(ll_context* ctx, ll_operator* op, const ll_lanczos_params* p, double* eigval_out, float* eigvec,
                          int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats);
int ll_expo_run_c(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                  const void* input_host, void* output_host, int64_t* itern_out, ll_run_stats* stats);
int ll_expo_run_s(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a, const float* input_host,
                  float* output_host, int64_t* itern_out, ll_run_stats* stats);
int ll_expo_taylor_run_c(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a_re, double a_im,
                         const void* input_host, void* output_host, int64_t* nterms_out);
int ll_expo_taylor_run_s(ll_context* ctx, ll_operator* op, const ll_expo_params* p, double a,
                         const float* input_host, float* output_host, int64_t* nterms_out);

#ifdef __cplusplus
}
#endif
#endif /* LANCZOS_HIP_H_ */
