// The extreme eigenpair WITHOUT a stored Krylov basis: pass 1 runs the plain three-term recurrence on three rotating
// vectors and records its coefficients; the host takes the eigenvector s of T_m; pass 2 replays the same recurrence from the record and
// accumulates psi = sum_k s_k u_k.  Memory is three or four vectors whatever the iteration count, against m + 1 for lanczos_run; the
// price is every operator application twice and no re-orthogonalisation (only the extreme pair is trustworthy: num_eigs = 1).
// Kernels: recur.hip.  The recurrence, the loop of pass 1 and the run's skeleton (TwoPass): recurrence.hpp, shared with
// expo_two_pass_multi_run.cpp.  Host side: the stop and breakdown tests of the eigen-solver loop (StepWorker<RitzTracker>, LL:264-309).
// Its own: where r_0 comes from, the Ritz vector of T_m, the final normalisation and the residual.
#include "recurrence.hpp"

namespace ll {

template <typename T>
void two_pass_run(ll_context* ctx, ll_operator* op, const ll_lanczos_params& P_in, double* eigval_out, T* eigvec,
                  int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  ll_lanczos_params P = P_in;
  check_run<T>(ctx, op, P, 1e3);
  LL_REQUIRE(P.num_eigs == 1, "the two-pass solver returns one eigenpair (num_eigs must be 1): without re-orthogonalisation only the extreme pair is trustworthy");
  LL_REQUIRE(ctx->comm == nullptr, "the two-pass solver does not run on sharded contexts yet");
  const bool want_vec = eigvec != nullptr;
  LL_REQUIRE(!want_vec || (const void*)eigvec != P.init_vector_dev, "the eigenvector buffer is the start vector's (init_vector_dev is never modified)");
  TwoPass<T> tp(ctx, op, P.eigenvalue_offset);
  Engine<T>& E = tp.E;
  Recurrence<T>& rc = tp.rc;
  hipStream_t s = tp.s;
  const int64_t nl = tp.nl;
  const size_t vbytes = tp.vbytes;
  const bool out_dev = is_device_ptr(eigvec);
  DevBuf<T> psi_own;
  if (want_vec && !out_dev) tp.own_vector(psi_own);
  T* const psi = want_vec ? (out_dev ? eigvec : psi_own.p) : nullptr;
  tp.prepare(P.max_iteration);

  // ---- start vector (LL:231-234): r_0, unnormalised, with c_0 = ||r_0||^2.  The hook (or the random default) runs ONCE; psi keeps
  // its result until pass 2 has taken r_0 from it again
  const double t_setup0 = now_s();
  if (P.init_vector_dev) {
    LL_HIP(hipMemcpyAsync(rc.vec(0), P.init_vector_dev, vbytes, hipMemcpyDeviceToDevice, s));
  } else {
    T* const stage = (T*)ctx->ensure_stage(std::max<size_t>(vbytes, sizeof(T)));
    if (P.init_vector) P.init_vector(stage, nl, op->row_begin, P.init_user);
    else random_start<T>(stage, nl);
    T* const first = psi ? psi : rc.vec(0);
    LL_HIP(hipMemcpyAsync(first, stage, vbytes, hipMemcpyHostToDevice, s));
    if (psi) LL_HIP(hipMemcpyAsync(rc.vec(0), psi, vbytes, hipMemcpyDeviceToDevice, s));
  }
  tp.start(t_setup0, "the start vector is zero or not finite");

  // ---- pass 1
  RitzTracker cfg;
  cfg.nroot = 1;
  cfg.find_maximum = P.find_maximum != 0;
  cfg.mode = P.tridiag_mode;
  cfg.eps = P.eps;
  cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon() * 1e1;  // H3 LL:279
  const RitzTracker::Out last = tp.pass1(cfg, P.max_iteration);
  const int64_t m = tp.m;
  std::vector<double>& alpha = tp.alpha;
  std::vector<double>& beta = tp.beta;
  alpha.resize((size_t)m);
  beta.resize((size_t)m);

  // ---- the Ritz pair of T_m (LL:312-319)
  double theta = last.evs[0];  // of the shifted operator
  if (P.tridiag_mode == LL_TRIDIAG_AUTO && !last.evs_from_qr) {  // as lanczos_run: the values of the reference's QR arithmetic
    std::vector<double> all((size_t)m);
    const double t0 = now_s();
    tridiag_qr(m, alpha.data(), beta.data(), all.data(), nullptr);
    tp.pt.tridiag += now_s() - t0;
    theta = P.find_maximum ? all[(size_t)m - 1] : all[0];
  }
  double residual = std::numeric_limits<double>::quiet_NaN();
  if (want_vec) {
    std::vector<double> sv((size_t)m, 1.0);
    const double t0 = now_s();
    if (m > 1 && P.tridiag_mode == LL_TRIDIAG_AUTO && m > 256) {
      tridiag_inverse_iteration(m, alpha.data(), beta.data(), 1, &theta, sv.data());
    } else if (m > 1) {
      std::vector<double> tev((size_t)m), tq((size_t)m * m);
      tridiag_qr(m, alpha.data(), beta.data(), tev.data(), tq.data());  // beta[m-1] is never read (LL:314)
      const int64_t row = P.find_maximum ? m - 1 : 0;
      std::copy(tq.begin() + row * m, tq.begin() + (row + 1) * m, sv.begin());
    }
    tp.pt.tridiag += now_s() - t0;
    std::vector<double> g((size_t)m + 1, 0.0);  // psi = sum_k g_k r_k, g_k = s_k / ||r_k||
    for (int64_t k = 0; k < m; ++k) g[(size_t)k] = sv[(size_t)k] / std::sqrt(tp.csq[(size_t)k]);
    DevBuf<double> gdev;
    // ---- pass 2: r_0 again, psi = g_0 r_0, then the replay
    tp.replay(
        g, gdev,
        [&] {
          if (P.init_vector_dev) {
            LL_HIP(hipMemcpyAsync(rc.vec(0), P.init_vector_dev, vbytes, hipMemcpyDeviceToDevice, s));
            LL_HIP(hipMemcpyAsync(psi, P.init_vector_dev, vbytes, hipMemcpyDeviceToDevice, s));
          } else {
            LL_HIP(hipMemcpyAsync(rc.vec(0), psi, vbytes, hipMemcpyDeviceToDevice, s));
          }
          launch_scale<T>(nl, psi, g[0], nullptr, s);
        },
        [&](int64_t k, T* y, const T* x, const T* p, const typename Engine<T>::DeferredAlpha& da, long long* mism) {
          launch_recur_accum<T>(nl, y, x, p, psi, rc.rec.p, gdev.p, k, 0.0, 0.0, 0.0, da.partials, da.nparts, mism, s);
        });
    E.norm2_dev(psi, E.S(kScalScratch) + 1);
    const NormRefs nr = E.plain_norm(E.S(kScalScratch) + 1);
    launch_scale<T>(nl, psi, 0.0, &nr, s);  // LL:58
    // ---- residual ||(A + offset) psi - theta psi||: one more application
    E.apply(psi, rc.vec(0), P.eigenvalue_offset, nullptr);
    launch_three_term<T>(nl, rc.vec(0), nullptr, psi, 0.0, theta, s);
    E.norm2_dev(rc.vec(0), E.S(kScalSpare));
    double r2 = 0.0;
    E.fetch(E.S(kScalSpare), &r2, 1);
    residual = std::sqrt(std::max(r2, 0.0));
    tp.read_mismatches();
    if (!out_dev) tp.to_host(eigvec, psi);
    LL_HIP(hipStreamSynchronize(s));
  }

  *eigval_out = theta - P.eigenvalue_offset;  // LL:317-319
  if (itern_out) *itern_out = m;
  if (residual_out) *residual_out = residual;
  if (alpha_out) std::copy(alpha.begin(), alpha.end(), alpha_out);
  if (beta_out) std::copy(beta.begin(), beta.end(), beta_out);
  tp.finish(stats);
}

#define LL_INST_TWO_PASS_RUN(T)                                                                                              \
  template void two_pass_run<T>(ll_context*, ll_operator*, const ll_lanczos_params&, double*, T*, int64_t*, double*, double*, \
                                double*, ll_run_stats*);
LL_FOR_EACH_SCALAR(LL_INST_TWO_PASS_RUN)

}  // namespace ll
