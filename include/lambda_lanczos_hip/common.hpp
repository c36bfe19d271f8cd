// C++ facade over the C ABI (include/lanczos_hip.h): RAII handles, error translation and the tag dispatch from the
// template parameter T to the _d / _z entry points ("templates cannot cross a C ABI").
#ifndef LAMBDA_LANCZOS_HIP_COMMON_HPP_
#define LAMBDA_LANCZOS_HIP_COMMON_HPP_

#include <algorithm>
#include <complex>
#include <functional>
#include <cstdint>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../lanczos_hip.h"
#include "entropy.hpp"  // von_neumann_entropy of a reduced density matrix (host only)
#include "spectral.hpp"  // continued_fraction, spectral_function of the coefficients of a Lanczos run (host only)
#include "util.hpp"  // lambda_lanczos::util::{real_t, inner_prod, norm, normalize, schmidt_orth, m_norm, sort_eigenpairs, ...}

namespace lambda_lanczos_hip {

// The reference never throws (asserts only); device / RCCL failures need a channel, so the facade throws.
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error("lanczos_hip error " + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int status) {
  if (status != LL_OK) throw Error(status, ll_last_error());
}

template <typename T> struct is_supported : std::false_type {};
template <> struct is_supported<double> : std::true_type {};
template <> struct is_supported<std::complex<double>> : std::true_type {};
template <> struct is_supported<float> : std::true_type {};
template <> struct is_supported<std::complex<float>> : std::true_type {};

// Tag dispatch from T to the _d / _z / _s / _c entry points of the C ABI.
template <typename T> struct abi;
#define LL_FACADE_ABI(T, SFX, HOSTFN)                                                                                    \
  template <> struct abi<T> {                                                                                            \
    static int create_csr(ll_context* c, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,       \
                          const T* va, ll_operator** o) {                                                                \
      return ll_op_create_csr_##SFX(c, nr, nc, rb, rp, ci, va, o);                                                       \
    }                                                                                                                    \
    static int create_csr_opt(ll_context* c, int64_t nr, int64_t nc, int64_t rb, const int64_t* rp, const int32_t* ci,   \
                              const T* va, const ll_csr_options* opt, ll_operator** o) {                                 \
      return ll_op_create_csr_opt_##SFX(c, nr, nc, rb, rp, ci, va, opt, o);                                              \
    }                                                                                                                    \
    static int create_csr_sym(ll_context* c, int64_t n, int uplo, const int64_t* rp, const int32_t* ci, const T* va,     \
                              const ll_csr_options* opt, ll_operator** o) {                                              \
      return ll_op_create_csr_sym_##SFX(c, n, uplo, rp, ci, va, opt, o);                                                 \
    }                                                                                                                    \
    static int create_dense(ll_context* c, int64_t nr, int64_t nc, int64_t rb, const T* a, ll_operator** o) {            \
      return ll_op_create_dense_##SFX(c, nr, nc, rb, a, o);                                                              \
    }                                                                                                                    \
    static int create_stencil(ll_context* c, const ll_stencil_desc* d, int64_t rb, int64_t nl, const double* onsite,     \
                              ll_operator** o) {                                                                         \
      return ll_op_create_stencil_##SFX(c, d, rb, nl, onsite, o);                                                        \
    }                                                                                                                    \
    static int create_pauli(ll_context* c, int32_t ns, int64_t nt, const ll_pauli_term* t, ll_operator** o) {            \
      return ll_op_create_pauli_##SFX(c, ns, nt, t, o);                                                                  \
    }                                                                                                                    \
    static int create_pauli_sector(ll_context* c, int32_t ns, int32_t nd, int64_t nt, const ll_pauli_term* t,            \
                                   ll_operator** o) {                                                                    \
      return ll_op_create_pauli_sector_##SFX(c, ns, nd, nt, t, o);                                                       \
    }                                                                                                                    \
    static int create_pauli_momentum(ll_context* c, int32_t ns, int32_t nd, int32_t m, int64_t nt, const ll_pauli_term* t,\
                                     ll_operator** o) {                                                                  \
      return ll_op_create_pauli_momentum_##SFX(c, ns, nd, m, nt, t, o);                                                  \
    }                                                                                                                    \
    static int create_pauli_momentum_full(ll_context* c, int32_t ns, int32_t m, int64_t nt, const ll_pauli_term* t,      \
                                          ll_operator** o) {                                                             \
      return ll_op_create_pauli_momentum_full_##SFX(c, ns, m, nt, t, o);                                                 \
    }                                                                                                                    \
    static int create_pauli_symmetric(ll_context* c, int32_t ns, int32_t nd, int32_t m, int32_t p, int32_t z, int64_t nt, \
                                      const ll_pauli_term* t, ll_operator** o) {                                         \
      return ll_op_create_pauli_symmetric_##SFX(c, ns, nd, m, p, z, nt, t, o);                                           \
    }                                                                                                                    \
    static int create_host(ll_context* c, int64_t n, int (*fn)(const void*, void*, int64_t, void*), void* user,          \
                           ll_operator** o) {                                                                            \
      return ll_op_create_host_##SFX(c, n, reinterpret_cast<HOSTFN>(fn), user, o);                                       \
    }                                                                                                                    \
    static int run(ll_context* c, ll_operator* op, const ll_lanczos_params* p, double* vals, T* vecs, int64_t* found,    \
                   int64_t* counts, int64_t cap, ll_run_stats* st) {                                                     \
      return ll_lanczos_run_##SFX(c, op, p, vals, vecs, found, counts, cap, nullptr, nullptr, st);                       \
    }                                                                                                                    \
    static int run_iteration(ll_context* c, ll_operator* op, const ll_lanczos_params* p, int64_t nroot, int64_t n_orth,  \
                             const T* orth, double* vals, T* vecs, int64_t* found, int64_t* itern, ll_run_stats* st) {   \
      return ll_lanczos_run_iteration_##SFX(c, op, p, nroot, n_orth, orth, vals, vecs, found, itern, nullptr, nullptr,   \
                                            st);                                                                         \
    }                                                                                                                    \
    static int two_pass(ll_context* c, ll_operator* op, const ll_lanczos_params* p, double* val, T* vec, int64_t* itern, \
                        double* residual, ll_run_stats* st) {                                                            \
      return ll_lanczos_two_pass_##SFX(c, op, p, val, vec, itern, residual, nullptr, nullptr, st);                       \
    }                                                                                                                    \
  };
LL_FACADE_ABI(double, d, ll_host_mv_mul_d)
LL_FACADE_ABI(float, s, ll_host_mv_mul_s)
LL_FACADE_ABI(std::complex<double>, z, ll_host_mv_mul_z)
LL_FACADE_ABI(std::complex<float>, c, ll_host_mv_mul_z)
#undef LL_FACADE_ABI

// Device + stream + workspace.  Copyable handle (shared ownership).
class Context {
 public:
  explicit Context(int device = 0) {
    ll_context* c = nullptr;
    check(LL_ABI_CHECK());  // a binary built against an older lanczos_hip.h must not hand its structs to this library
    check(ll_ctx_create(device, &c));
    h_.reset(c, [](ll_context* p) { ll_ctx_destroy(p); });
  }
  Context(int device, void* hip_stream) {
    ll_context* c = nullptr;
    check(LL_ABI_CHECK());
    check(ll_ctx_create_on_stream(device, hip_stream, &c));
    h_.reset(c, [](ll_context* p) { ll_ctx_destroy(p); });
  }
  ll_context* get() const { return h_.get(); }
  // One process per GPU: attach an RCCL communicator (id from Context::unique_id() on rank 0, distributed by the host).
  static std::vector<char> unique_id() {
    std::vector<char> id(LL_UNIQUE_ID_BYTES);
    check(ll_comm_unique_id(id.data()));
    return id;
  }
  void init_comm(const std::vector<char>& id, int rank, int n_ranks) { check(ll_comm_init(get(), id.data(), rank, n_ranks)); }
  // Which transport answers the collectives: "rccl", "plugin:<path>", "attached" or "none" (ll_comm_transport).
  std::string transport() const {
    char buf[512];
    check(ll_comm_transport(get(), buf, sizeof(buf)));
    return std::string(buf);
  }
  // UNSTABLE: one tuning field of this context by key, on top of the environment switches (ll_ctx_set_tuning; value nullptr removes
  // the setting).  The environment carries only the user-facing switches of INTEGRATION.md section 8.
  void set_tuning(const char* key, const char* value) { check(ll_ctx_set_tuning(get(), key, value)); }
  static Context& default_context() {
    static Context ctx(0);
    return ctx;
  }

 private:
  std::shared_ptr<ll_context> h_;
};

// The device forms of the mv_mul plugin.  A DeviceOperator<T> is a shared handle to an operator resident in HBM; the
// engines accept it in place of the host std::function, and then only scalars cross PCIe per iteration.
template <typename T> class DeviceOperator {
  static_assert(is_supported<T>::value, "DeviceOperator<T>: T must be float, double or std::complex of those");

 public:
  ll_operator* get() const { return h_.get(); }
  const Context& context() const { return ctx_; }
  int64_t size() const { return n_; }
  int64_t local_rows() const { return n_local_; }
  // max_i sum_j |a_ij| over the local rows: a safe |eigenvalue_offset| (determine_eigenvalue_offset.cpp:12-29)
  double inf_norm() const {
    double v = 0;
    check(ll_op_inf_norm(get(), &v));
    return v;
  }

 protected:
  DeviceOperator(Context ctx) : ctx_(ctx) {}
  void adopt(ll_operator* op, int64_t n, int64_t n_local) {
    h_.reset(op, [](ll_operator* p) { ll_op_destroy(p); });
    n_ = n;
    n_local_ = n_local;
  }
  Context ctx_;
  std::shared_ptr<ll_operator> h_;
  int64_t n_ = 0, n_local_ = 0;
};

// CSR matrix: rows [row_begin, row_begin + n_rows) of an n_cols x n_cols symmetric/Hermitian operator (the whole
// matrix on a single GPU).
//
// Accuracy of y = A x — what stands in for the user's fp64 mv_mul loop (lambda_lanczos.hpp:120-126).  The default class
// (Accuracy::Default -> norm-wise where the propagation-blocked kernel is selected) bounds the error of every row by
// eps * sum_j |a_ij||x_j| + nnz_i 2^-60 ||A||_inf max|x|: right for Lanczos vectors of extended states and what the Krylov
// recurrence needs, but not component-wise for strongly LOCALISED vectors.  A caller who knows their vectors are localised
// passes Accuracy::Componentwise (floating-point sums in a fixed order: the accuracy of a plain fp64 row loop, 3-5 % slower
// on such matrices) — per operator, no environment variable; set_accuracy() moves an existing operator between the classes.
enum class Accuracy : int {
  Default = LL_ACCURACY_DEFAULT,
  Normwise = LL_ACCURACY_NORMWISE,
  Componentwise = LL_ACCURACY_COMPONENTWISE
};
template <typename T> class CsrMatrix : public DeviceOperator<T> {
 public:
  CsrMatrix(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& col, const std::vector<T>& val,
            Context ctx = Context::default_context(), int64_t n_cols = -1, int64_t row_begin = 0,
            Accuracy accuracy = Accuracy::Default)
      : DeviceOperator<T>(ctx) {
    const int64_t n_rows = (int64_t)row_ptr.size() - 1;
    if (n_cols < 0) n_cols = n_rows;
    ll_operator* op = nullptr;
    ll_csr_options opt;
    check(ll_csr_options_default(&opt));
    opt.accuracy = (int32_t)accuracy;
    check(abi<T>::create_csr_opt(ctx.get(), n_rows, n_cols, row_begin, row_ptr.data(), col.data(), val.data(), &opt, &op));
    this->adopt(op, n_cols, n_rows);
  }
  CsrMatrix(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& col, const std::vector<T>& val, Accuracy accuracy)
      : CsrMatrix(row_ptr, col, val, Context::default_context(), -1, 0, accuracy) {}
  void set_accuracy(Accuracy a) { check(ll_op_set_accuracy(this->get(), (int)a)); }
  Accuracy accuracy() const {
    int a = 0;
    check(ll_op_accuracy(this->get(), &a));
    return (Accuracy)a;
  }
};

// A symmetric (real T) / Hermitian (complex T) matrix given as ONE stored triangle (ll_op_create_csr_sym_*): a MatrixMarket
// symmetric / hermitian file, scipy.sparse.triu, an FEM assembly.  A = T + T^H - diag(T); the library keeps the one-triangle
// image (LL_SPMV_SYM) when the triangle is eligible, the expanded full matrix otherwise.  Single-rank contexts only.
enum class Triangle { Upper = LL_UPPER, Lower = LL_LOWER };
template <typename T> class SymmetricCsrMatrix : public DeviceOperator<T> {
 public:
  SymmetricCsrMatrix(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& col, const std::vector<T>& val,
                     Triangle uplo, Context ctx = Context::default_context(), Accuracy accuracy = Accuracy::Default)
      : DeviceOperator<T>(ctx) {
    const int64_t n = (int64_t)row_ptr.size() - 1;
    ll_operator* op = nullptr;
    ll_csr_options opt;
    check(ll_csr_options_default(&opt));
    opt.accuracy = (int32_t)accuracy;
    check(abi<T>::create_csr_sym(ctx.get(), n, (int)uplo, row_ptr.data(), col.data(), val.data(), &opt, &op));
    this->adopt(op, n, n);
  }
  int selected_spmv() const {
    int k = 0;
    check(ll_op_selected_spmv(this->get(), &k));
    return k;
  }
  int64_t device_bytes() const {
    int64_t b = 0;
    check(ll_op_device_bytes(this->get(), &b));
    return b;
  }
};

// Dense row-major matrix (the operator of src/samples/sample1_simple.cpp:22-28 without the host loop).
template <typename T> class DenseMatrix : public DeviceOperator<T> {
 public:
  explicit DenseMatrix(const std::vector<std::vector<T>>& rows, Context ctx = Context::default_context(),
                       int64_t row_begin = 0)
      : DeviceOperator<T>(ctx) {
    const int64_t nr = (int64_t)rows.size(), nc = nr ? (int64_t)rows[0].size() : 0;
    std::vector<T> flat;
    flat.reserve((size_t)(nr * nc));
    for (const auto& r : rows) {
      if ((int64_t)r.size() != nc) throw Error(LL_ERR_INVALID, "DenseMatrix: ragged rows");
      flat.insert(flat.end(), r.begin(), r.end());
    }
    ll_operator* op = nullptr;
    check(abi<T>::create_dense(ctx.get(), nr, nc, row_begin, flat.data(), &op));
    this->adopt(op, nc, nr);
  }
};

// Matrix-free lattice operator (the family of src/samples/sample3_dynamic.cpp:17-22):
//   (A x)(r) = (diag + onsite[r]) x(r) + sum_d ( hop[d] x(r + e_d) + conj(hop[d]) x(r - e_d) )
// on a row-major lattice dims[0] x dims[1] x .. (last index fastest), open or periodic per dimension.
template <typename T> class LatticeOperator : public DeviceOperator<T> {
 public:
  // phase_grad (optional, complex T): ndim x ndim row-major; the bond r -> r + e_d carries
  // hop[d] * exp(i * sum_e phase_grad[d*ndim + e] * c_e(r)) — Peierls phases of a magnetic field.
  LatticeOperator(const std::vector<int64_t>& dims, double diag, const std::vector<std::complex<double>>& hop,
                  const std::vector<bool>& periodic, const std::vector<double>& onsite = {},
                  Context ctx = Context::default_context(), int64_t row_begin = 0, int64_t n_local = -1,
                  const std::vector<double>& phase_grad = {})
      : DeviceOperator<T>(ctx) {
    if (dims.empty() || dims.size() > 3 || hop.size() != dims.size() || periodic.size() != dims.size())
      throw Error(LL_ERR_INVALID, "LatticeOperator: 1 to 3 dimensions, one hop and one periodic flag per dimension");
    ll_stencil_desc d = {};
    d.ndim = (int32_t)dims.size();
    int64_t n = 1;
    for (size_t k = 0; k < dims.size(); ++k) {
      d.dims[k] = dims[k];
      d.periodic[k] = periodic[k] ? 1 : 0;
      d.hop_re[k] = hop[k].real();
      d.hop_im[k] = hop[k].imag();
      n *= dims[k];
    }
    d.diag = diag;
    if (!phase_grad.empty()) {
      if (phase_grad.size() != dims.size() * dims.size()) throw Error(LL_ERR_INVALID, "LatticeOperator: phase_grad must be ndim x ndim");
      for (size_t k = 0; k < dims.size(); ++k)
        for (size_t e = 0; e < dims.size(); ++e) d.phase_grad[k][e] = phase_grad[k * dims.size() + e];
    }
    if (n_local < 0) n_local = n;
    if (!onsite.empty() && (int64_t)onsite.size() != n_local) throw Error(LL_ERR_INVALID, "LatticeOperator: onsite size");
    ll_operator* op = nullptr;
    check(abi<T>::create_stencil(ctx.get(), &d, row_begin, n_local, onsite.empty() ? nullptr : onsite.data(), &op));
    this->adopt(op, n, n_local);
  }
};

// What the six Pauli-sum operators below share: size() and local_rows() are read from the created operator (ll_op_info), and
// device_bytes().  PauliSpinBasisOperator and PauliRingBlockOperator add the measurements of the two kinds of basis.
template <typename T> class PauliFamilyOperator : public DeviceOperator<T> {
 public:
  int64_t device_bytes() const {
    int64_t b = 0;
    check(ll_op_device_bytes(this->get(), &b));
    return b;
  }

 protected:
  explicit PauliFamilyOperator(Context ctx) : DeviceOperator<T>(ctx) {}
  // ll_pauli_rdm on `op`, for both kinds of basis (a ring block measures on its target): rho[a][a'] row-major, 2^m x 2^m,
  // m = sites.size(); psi is host or device memory of op.local_rows() values (the library decides per pointer)
  static std::vector<std::complex<double>> rdm(const PauliFamilyOperator<T>& op, const std::vector<int>& sites, const T* psi,
                                               int64_t* sweeps) {
    const std::vector<int32_t> s32(sites.begin(), sites.end());
    const size_t dim = (size_t)1 << std::min<size_t>(s32.size(), 6);  // (a count the library refuses still gets a buffer)
    std::vector<std::complex<double>> out(dim * dim);
    check(ll_pauli_rdm(op.context().get(), op.get(), (int32_t)s32.size(), s32.data(), psi, reinterpret_cast<double*>(out.data()), sweeps));
    return out;
  }
  // ll_pauli_rdm_tiled on `op`: the same layout for 4 to 13 sites
  static std::vector<std::complex<double>> rdm_tiled(const PauliFamilyOperator<T>& op, const std::vector<int>& sites, const T* psi,
                                                     int64_t* sweeps) {
    const std::vector<int32_t> s32(sites.begin(), sites.end());
    const size_t dim = (size_t)1 << (s32.size() >= 4 && s32.size() <= 13 ? s32.size() : 4);  // (a refused count: a small buffer)
    std::vector<std::complex<double>> out(dim * dim);
    check(ll_pauli_rdm_tiled(op.context().get(), op.get(), (int32_t)s32.size(), s32.data(), psi, out.data(), sweeps));
    return out;
  }
  void adopt_created(ll_operator* op) {
    int64_t n = 0, n_local = 0, n_terms = 0;
    const int rc = ll_op_info(op, &n, &n_local, &n_terms);
    if (rc != LL_OK) (void)ll_op_destroy(op);
    check(rc);
    this->adopt(op, n, n_local);
  }
};

using PauliTerm = ll_pauli_term;

// The operators whose basis is a spin basis — PauliOperator (all 2^n_sites states) and PauliSectorOperator (one S_z sector): a
// site is a tensor factor, so Pauli strings and subsystems are measured on psi itself.
template <typename T> class PauliSpinBasisOperator : public PauliFamilyOperator<T> {
 public:
  // coef * Re <psi| P |psi> for every observable (x_mask, z_mask, coef), many per sweep over psi and with no n-sized workspace for
  // a device psi (ll_pauli_expect); nothing is divided by <psi|psi>.  psi: a device pointer (or any host pointer) to size()
  // values, or a std::vector<T>.  sweeps (nullable): the passes over psi that were launched.  On a sector a partner s ^ x outside
  // the sector contributes nothing.
  std::vector<double> expectation(const std::vector<PauliTerm>& observables, const T* psi, int64_t* sweeps = nullptr) const {
    std::vector<double> out(observables.size(), 0.0);
    check(ll_pauli_expect(this->context().get(), this->get(), (int64_t)observables.size(), observables.data(), psi, out.data(), sweeps));
    return out;
  }
  std::vector<double> expectation(const std::vector<PauliTerm>& observables, const std::vector<T>& psi, int64_t* sweeps = nullptr) const {
    if ((int64_t)psi.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "expectation: psi must hold local_rows() values");
    return expectation(observables, psi.data(), sweeps);
  }

  // rho_A = Tr_env |psi><psi| of up to six distinct sites in one sweep over psi (ll_pauli_rdm): row-major 2^m x 2^m with
  // rho[a][a'] = sum_e psi(a, e) conj(psi(a', e)), bit k of a = sites[k]; exactly Hermitian, not divided by <psi|psi> (the trace
  // is ||psi||^2).  psi as for expectation().  On a sector every entry with popcount(a) != popcount(a') is exactly +0.0.
  // von_neumann_entropy (entropy.hpp) takes the result.
  std::vector<std::complex<double>> reduced_density_matrix(const std::vector<int>& sites, const T* psi, int64_t* sweeps = nullptr) const {
    return this->rdm(*this, sites, psi, sweeps);
  }
  std::vector<std::complex<double>> reduced_density_matrix(const std::vector<int>& sites, const std::vector<T>& psi,
                                                           int64_t* sweeps = nullptr) const {
    if ((int64_t)psi.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "reduced_density_matrix: psi must hold local_rows() values");
    return reduced_density_matrix(sites, psi.data(), sweeps);
  }

  // The same rho_A for 4 to 13 distinct sites — the half chain of a ring of 20 to 26 sites — formed as a rank-K update on the f64
  // matrix cores (ll_pauli_rdm_tiled): the same layout and the same Hermitian contract, 4^m values (1 GiB at 13 sites).
  // von_neumann_entropy (entropy.hpp) keeps its limit of 64 x 64: a larger rho goes to an eigen-solver of the caller's.
  std::vector<std::complex<double>> reduced_density_matrix_tiled(const std::vector<int>& sites, const T* psi, int64_t* sweeps = nullptr) const {
    return this->rdm_tiled(*this, sites, psi, sweeps);
  }
  std::vector<std::complex<double>> reduced_density_matrix_tiled(const std::vector<int>& sites, const std::vector<T>& psi,
                                                                 int64_t* sweeps = nullptr) const {
    if ((int64_t)psi.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "reduced_density_matrix_tiled: psi must hold local_rows() values");
    return reduced_density_matrix_tiled(sites, psi.data(), sweeps);
  }

 protected:
  explicit PauliSpinBasisOperator(Context ctx) : PauliFamilyOperator<T>(ctx) {}
};

// The operators whose basis is a symmetry block of a ring — PauliMomentumOperator, PauliMomentumFullOperator and
// PauliSymmetricOperator — or of a torus, PauliTorusOperator (expectation() only: the library refuses the rest for that kind):
// vectors hold coefficients on the block's representatives, Psi = B c with B the block's isometry.
template <typename T> class PauliRingBlockOperator : public PauliFamilyOperator<T> {
 public:
  // coef * Re <Psi| P |Psi> for every observable, Psi = B psi the state that the size() coefficients psi on the block's basis stand
  // for — Psi is never formed: every observable is averaged over the block's group and measured with the gather of this
  // operator's apply, up to 32 per sweep over psi (ll_pauli_expect_block); nothing is divided by <psi|psi>.  psi: a device pointer
  // (or any host pointer) to size() values, or a std::vector<T>.  sweeps (nullable): the passes over psi that were launched.
  std::vector<double> expectation(const std::vector<PauliTerm>& observables, const T* psi, int64_t* sweeps = nullptr) const {
    std::vector<double> out(observables.size(), 0.0);
    check(ll_pauli_expect_block(this->context().get(), this->get(), (int64_t)observables.size(), observables.data(), psi, out.data(),
                                sweeps));
    return out;
  }
  std::vector<double> expectation(const std::vector<PauliTerm>& observables, const std::vector<T>& psi, int64_t* sweeps = nullptr) const {
    if ((int64_t)psi.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "expectation: psi must hold local_rows() values");
    return expectation(observables, psi.data(), sweeps);
  }

  // Psi = B c on the basis of `target` — the PauliOperator of the ring or the PauliSectorOperator of this block's n_down — and
  // c = B^H Psi, the part of ANY state of that basis in this block (ll_pauli_block_expand / ll_pauli_block_project): pointers to
  // host or device memory, or std::vector<T>; c holds local_rows() values, psi target.local_rows().
  void expand(const PauliFamilyOperator<T>& target, const T* c, T* psi_out) const {
    check(ll_pauli_block_expand(this->context().get(), this->get(), target.get(), c, psi_out));
  }
  std::vector<T> expand(const PauliFamilyOperator<T>& target, const std::vector<T>& c) const {
    if ((int64_t)c.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "expand: c must hold local_rows() values");
    std::vector<T> psi((size_t)target.local_rows());
    expand(target, c.data(), psi.data());
    return psi;
  }
  void project(const PauliFamilyOperator<T>& target, const T* psi, T* c_out) const {
    check(ll_pauli_block_project(this->context().get(), this->get(), target.get(), psi, c_out));
  }
  std::vector<T> project(const PauliFamilyOperator<T>& target, const std::vector<T>& psi) const {
    if ((int64_t)psi.size() != target.local_rows()) throw Error(LL_ERR_INVALID, "project: psi must hold target.local_rows() values");
    std::vector<T> c((size_t)this->local_rows());
    project(target, psi.data(), c.data());
    return c;
  }

  // out = B_t^H (sum of `terms`) B c: the strings applied to the state c of this block, taken on the momentum block `target` of the
  // same kind, n_sites and n_down, without a vector of the full space (ll_pauli_block_transfer) — the strings need not commute
  // with the translation, the target selects their component of momentum m_t - m.  c holds local_rows() values, out
  // target.local_rows(); norm2 (nullable): sum |out|^2 as the kernel sums it.  For PauliMomentumOperator and
  // PauliMomentumFullOperator; the library refuses a PauliSymmetricOperator (that needs semi-momentum states).
  void transfer(const PauliRingBlockOperator<T>& target, const std::vector<PauliTerm>& terms, const T* c, T* out,
                double* norm2 = nullptr) const {
    check(ll_pauli_block_transfer(this->context().get(), this->get(), target.get(), (int64_t)terms.size(), terms.data(), c, out, norm2));
  }
  std::vector<T> transfer(const PauliRingBlockOperator<T>& target, const std::vector<PauliTerm>& terms, const std::vector<T>& c,
                          double* norm2 = nullptr) const {
    if ((int64_t)c.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "transfer: c must hold local_rows() values");
    std::vector<T> out((size_t)target.local_rows());
    transfer(target, terms, c.data(), out.data(), norm2);
    return out;
  }

  // rho_A of Psi = B c: c is expanded into a device buffer of the context, measured by the target's reduced_density_matrix
  // (ll_pauli_rdm) and the buffer freed; von_neumann_entropy (entropy.hpp) takes the result.
  std::vector<std::complex<double>> reduced_density_matrix(const std::vector<int>& sites, const T* c, const PauliFamilyOperator<T>& target,
                                                           int64_t* sweeps = nullptr) const {
    void* buf = nullptr;
    check(ll_malloc(this->context().get(), (size_t)std::max<int64_t>(target.local_rows(), 1) * sizeof(T), &buf));
    std::vector<std::complex<double>> rho;
    try {
      expand(target, c, static_cast<T*>(buf));
      rho = this->rdm(target, sites, static_cast<const T*>(buf), sweeps);
    } catch (...) {
      (void)ll_free(this->context().get(), buf);
      throw;
    }
    check(ll_free(this->context().get(), buf));
    return rho;
  }
  std::vector<std::complex<double>> reduced_density_matrix(const std::vector<int>& sites, const std::vector<T>& c,
                                                           const PauliFamilyOperator<T>& target, int64_t* sweeps = nullptr) const {
    if ((int64_t)c.size() != this->local_rows()) throw Error(LL_ERR_INVALID, "reduced_density_matrix: c must hold local_rows() values");
    return reduced_density_matrix(sites, c.data(), target, sweeps);
  }

 protected:
  explicit PauliRingBlockOperator(Context ctx) : PauliFamilyOperator<T>(ctx) {}
};

// Matrix-free spin-1/2 Hamiltonian H = sum_t coef_t P_t on n_sites spins (n = 2^n_sites): what a many-body user writes as an
// mv_mul plugin, applied on the device from its list of Pauli strings.  Bit j of a basis state is site j; a term's site j
// carries X (x_mask bit only), Z (z_mask bit only), Y (both).  A Heisenberg bond J S_j.S_k is {m, 0, J/4}, {m, m, J/4},
// {0, m, J/4} with m = 2^j | 2^k.  Real T: an even number of Y per term.  Single-rank contexts only (ll_op_create_pauli_*).
// inf_norm() returns sum_t |coef_t|: an upper bound of every absolute row sum.
template <typename T> class PauliOperator : public PauliSpinBasisOperator<T> {
 public:
  PauliOperator(int n_sites, const std::vector<PauliTerm>& terms, Context ctx = Context::default_context())
      : PauliSpinBasisOperator<T>(ctx) {
    ll_operator* op = nullptr;
    check(abi<T>::create_pauli(ctx.get(), (int32_t)n_sites, (int64_t)terms.size(), terms.data(), &op));
    this->adopt_created(op);
  }
};

// The same Hamiltonian on one magnetisation sector: vectors hold the C(n_sites, n_down) amplitudes of the states with n_down set
// bits (a set bit is sigma_z = -1), in ascending integer order; size() returns that number.  H must conserve total S_z
// (Heisenberg, XXZ, J1-J2, Dzyaloshinskii-Moriya, z fields): one that does not is refused with an Error that names the x mask
// at fault (ll_op_create_pauli_sector_*).
template <typename T> class PauliSectorOperator : public PauliSpinBasisOperator<T> {
 public:
  PauliSectorOperator(int n_sites, int n_down, const std::vector<PauliTerm>& terms, Context ctx = Context::default_context())
      : PauliSpinBasisOperator<T>(ctx) {
    ll_operator* op = nullptr;
    check(abi<T>::create_pauli_sector(ctx.get(), (int32_t)n_sites, (int32_t)n_down, (int64_t)terms.size(), terms.data(), &op));
    this->adopt_created(op);
  }
};

// One momentum block of that sector on a ring: H must also commute with the one-site translation T (site j -> j + 1 mod n_sites).
// Vectors hold the D_m amplitudes of the basis |r; m> = N_r^(-1/2) sum_j e^(-2 pi i m j / n_sites) T^j |r>, r running over the
// orbit representatives (smallest member) whose orbit length R satisfies m R = 0 (mod n_sites), ascending; size() returns D_m.
// 0 <= momentum < n_sites; real T takes momentum 0 and n_sites / 2 only.  The image holds 4 C(n_sites, n_down) bytes of look-up
// table (device_bytes()); inf_norm() returns sum_t |coef_t|, a bound of every |eigenvalue| (ll_op_create_pauli_momentum_*).
template <typename T> class PauliMomentumOperator : public PauliRingBlockOperator<T> {
 public:
  PauliMomentumOperator(int n_sites, int n_down, int momentum, const std::vector<PauliTerm>& terms,
                        Context ctx = Context::default_context())
      : PauliRingBlockOperator<T>(ctx) {
    ll_operator* op = nullptr;
    check(abi<T>::create_pauli_momentum(ctx.get(), (int32_t)n_sites, (int32_t)n_down, (int32_t)momentum, (int64_t)terms.size(),
                                        terms.data(), &op));
    this->adopt_created(op);
  }
};

// One momentum block of the FULL 2^n_sites space of a ring: H must commute with the one-site translation and need not conserve
// S_z (transverse-field Ising, XYZ rings, transverse fields).  Vectors hold the D_m amplitudes of |r; m>, r running over the
// orbit representatives of ALL states whose orbit length R satisfies m R = 0 (mod n_sites), ascending; size() returns D_m (about
// 2^n_sites / n_sites).  0 <= momentum < n_sites; real T takes momentum 0 and n_sites / 2 only.  The image is O(D_m) — no table
// over the 2^n_sites states: device_bytes() <= 8 D_m + 64 KiB; inf_norm() returns sum_t |coef_t|, a bound of every |eigenvalue|
// (ll_op_create_pauli_momentum_full_*).
template <typename T> class PauliMomentumFullOperator : public PauliRingBlockOperator<T> {
 public:
  PauliMomentumFullOperator(int n_sites, int momentum, const std::vector<PauliTerm>& terms, Context ctx = Context::default_context())
      : PauliRingBlockOperator<T>(ctx) {
    ll_operator* op = nullptr;
    check(abi<T>::create_pauli_momentum_full(ctx.get(), (int32_t)n_sites, (int32_t)momentum, (int64_t)terms.size(), terms.data(),
                                             &op));
    this->adopt_created(op);
  }
};

// One block of a ring under momentum, reflection and spin inversion: parity / inversion are 0 (not used), +1 or -1; n_down = -1
// is the full space, else the S_z sector.  H must commute with the one-site translation and with every symmetry in use.  Vectors
// hold the D amplitudes of |r; chi>, r running over the admitted representatives of the group's orbits, ascending; size()
// returns D.  parity != 0 and real T take momentum 0 and n_sites / 2 only; an empty block is refused.  The image is O(D):
// device_bytes() <= 8 D + 192 KiB; inf_norm() returns sum_t |coef_t|, a bound of every |eigenvalue|
// (ll_op_create_pauli_symmetric_*).
template <typename T> class PauliSymmetricOperator : public PauliRingBlockOperator<T> {
 public:
  PauliSymmetricOperator(int n_sites, int momentum, const std::vector<PauliTerm>& terms, int parity = 0, int inversion = 0,
                         int n_down = -1, Context ctx = Context::default_context())
      : PauliRingBlockOperator<T>(ctx) {
    ll_operator* op = nullptr;
    check(abi<T>::create_pauli_symmetric(ctx.get(), (int32_t)n_sites, (int32_t)n_down, (int32_t)momentum, (int32_t)parity,
                                         (int32_t)inversion, (int64_t)terms.size(), terms.data(), &op));
    this->adopt_created(op);
  }
};

// One translation block (mx, my) of an lx x ly torus: site (x, y) is bit x + lx y, 0 <= mx < lx, 0 <= my < ly; n_down = -1 is the
// full space, else the S_z sector.  H must commute with both one-site translations (creation names the direction and the term at
// fault).  Vectors hold the D amplitudes of |r; mx my>, r running over the admitted representatives of the translation orbits,
// ascending; size() returns D.  Real T takes mx = 0 or lx / 2 and my = 0 or ly / 2 only; an empty block is refused.  The image
// is O(D): device_bytes() <= 8 D + 192 KiB; inf_norm() returns sum_t |coef_t|, a bound of every |eigenvalue|; expectation()
// measures on the block; the library refuses expand, project, transfer and the density matrices for this kind
// (ll_op_create_pauli_torus: one untyped entry point, the storage type goes as a character).
template <typename T> class PauliTorusOperator : public PauliRingBlockOperator<T> {
 public:
  PauliTorusOperator(int lx, int ly, int mx, int my, const std::vector<PauliTerm>& terms, int n_down = -1,
                     Context ctx = Context::default_context())
      : PauliRingBlockOperator<T>(ctx) {
    constexpr int32_t storage = std::is_same<T, double>::value                 ? 'd'
                                : std::is_same<T, std::complex<double>>::value ? 'z'
                                : std::is_same<T, float>::value                ? 's'
                                                                               : 'c';
    ll_operator* op = nullptr;
    check(ll_op_create_pauli_torus(ctx.get(), storage, (int32_t)lx, (int32_t)ly, (int32_t)n_down, (int32_t)mx, (int32_t)my,
                                   (int64_t)terms.size(), terms.data(), &op));
    this->adopt_created(op);
  }
};

// VectorRandomInitializer<T> (lambda_lanczos.hpp:70-104; the public init_vector member points at its init, :133): every
// element — real and imaginary part for complex T — uniform in [-1, 1] from a std::random_device-seeded mt19937.
// Callable like the reference's, so user code that invokes engine.init_vector(v) or names the class keeps working.
template <typename T> struct VectorRandomInitializer {
  static void init(std::vector<T>& v) {
    std::random_device dev;
    std::mt19937 mt(dev());
    std::uniform_real_distribution<T> rand((T)(-1.0), (T)(1.0));
    for (auto& e : v) e = rand(mt);
  }
};
template <typename R> struct VectorRandomInitializer<std::complex<R>> {
  static void init(std::vector<std::complex<R>>& v) {
    std::random_device dev;
    std::mt19937 mt(dev());
    std::uniform_real_distribution<R> rand((R)(-1.0), (R)(1.0));
    for (auto& e : v) {
      const R re = rand(mt);  // real part first, like the reference's constructor-argument order in practice
      const R im = rand(mt);
      e = std::complex<R>(re, im);
    }
  }
};

namespace detail {
// Host-callback trampoline: the reference's mv_mul signature works on std::vector, the C ABI on raw pointers.
template <typename T> struct HostOp {
  std::function<void(const std::vector<T>&, std::vector<T>&)> fn;
  std::vector<T> in, out;
  static int call(const void* in_p, void* out_p, int64_t n, void* user) {
    HostOp* self = static_cast<HostOp*>(user);
    try {
      const T* a = static_cast<const T*>(in_p);
      self->in.assign(a, a + n);
      self->out.assign((size_t)n, T());  // zero-filled on entry (lambda_lanczos.hpp:242)
      self->fn(self->in, self->out);
      std::copy(self->out.begin(), self->out.end(), static_cast<T*>(out_p));
      return 0;
    } catch (...) {
      return 1;
    }
  }
};

// The default of the public init_vector member: the reference's VectorRandomInitializer<T> under its own name (above,
// outside detail); RandomInit is the name earlier rounds of this facade used.
template <typename T> using RandomInit = VectorRandomInitializer<T>;

template <typename T> struct InitHook {
  std::function<void(std::vector<T>&)> fn;
  static void call(void* vec, int64_t n_local, int64_t /*row_begin*/, void* user) {
    InitHook* self = static_cast<InitHook*>(user);
    std::vector<T> v((size_t)n_local);
    self->fn(v);
    std::copy(v.begin(), v.end(), static_cast<T*>(vec));
  }
};

template <typename T> inline ll_operator* make_host_operator(ll_context* ctx, int64_t n, HostOp<T>* h) {
  ll_operator* op = nullptr;
  check(abi<T>::create_host(ctx, n, &HostOp<T>::call, h, &op));
  return op;
}
}  // namespace detail

}  // namespace lambda_lanczos_hip

#endif  // LAMBDA_LANCZOS_HIP_COMMON_HPP_
