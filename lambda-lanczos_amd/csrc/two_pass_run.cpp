// The extreme eigenpair WITHOUT a stored Krylov basis: pass 1 runs the plain three-term recurrence on three rotating
// vectors and records its coefficients; the host takes the eigenvector s of T_m; pass 2 replays the same recurrence from the record and
// accumulates psi = sum_k s_k u_k.  Memory is three or four vectors whatever the iteration count, against m + 1 for lanczos_run; the
// price is every operator application twice and no re-orthogonalisation (only the extreme pair is trustworthy: num_eigs = 1).
// Kernels: recur.hip.  The recurrence and the loop of pass 1: recurrence.hpp, shared with expo_two_pass_run.cpp.  Host side: the stop
// and breakdown tests of the eigen-solver loop (StepWorker<RitzTracker>, LL:264-309).
#include "recurrence.hpp"

#include <random>

namespace ll {
namespace {

// LL:70-104: std::random_device-seeded mt19937, uniform [-1,1]; complex: both parts
template <typename T> void random_start(T* v, int64_t n) {
  typedef typename scalar_traits<T>::real Real;
  std::random_device dev;
  std::mt19937 mt(dev());
  std::uniform_real_distribution<Real> r((Real)-1, (Real)1);
  Real* f = reinterpret_cast<Real*>(v);
  for (int64_t i = 0; i < n * scalar_traits<T>::reals; ++i) f[i] = r(mt);
}

}  // namespace

template <typename T>
void two_pass_run(ll_context* ctx, ll_operator* op, const ll_lanczos_params& P_in, double* eigval_out, T* eigvec,
                  int64_t* itern_out, double* residual_out, double* alpha_out, double* beta_out, ll_run_stats* stats) {
  ll_lanczos_params P = P_in;
  check_run<T>(ctx, op, P, 1e3);
  LL_REQUIRE(P.num_eigs == 1, "the two-pass solver returns one eigenpair (num_eigs must be 1): without re-orthogonalisation only the extreme pair is trustworthy");
  LL_REQUIRE(ctx->comm == nullptr, "the two-pass solver does not run on sharded contexts yet");
  LL_HIP(hipSetDevice(ctx->device));
  const double t_start = now_s();
  hipStream_t s = ctx->stream;
  const int64_t nl = op->n_local;
  const int64_t ld = round_up(std::max<int64_t>(std::max(nl, op->n_shard), 1), 256);
  const size_t vbytes = (size_t)nl * sizeof(T);
  const bool want_vec = eigvec != nullptr;
  const bool out_dev = is_device_ptr(eigvec);
  LL_REQUIRE(!want_vec || (const void*)eigvec != P.init_vector_dev, "the eigenvector buffer is the start vector's (init_vector_dev is never modified)");

  Engine<T> E(ctx, op, nl);
  Recurrence<T> rc{E, s, nl, P.eigenvalue_offset, E.can_scale_input(), {}, {}, 0};
  for (auto& b : rc.buf) b.alloc(ctx, (size_t)ld);
  DevBuf<T> psi_own;
  int64_t workspace_vectors = 3;
  if (want_vec && !out_dev) {
    psi_own.alloc(ctx, (size_t)ld);
    ++workspace_vectors;
  }
  T* const psi = want_vec ? (out_dev ? eigvec : psi_own.p) : nullptr;
  ctx->ensure_pinned(kPinnedScalars);
  ctx->ensure_partials((size_t)kMaxGrid * Engine<T>::R);
  ctx->ensure_h(4);
  EventRing ring;
  rc.ensure_rec(std::min<int64_t>(P.max_iteration, 4095));

  // ---- start vector (LL:231-234): r_0, unnormalised, with c_0 = ||r_0||^2.  The hook (or the random default) runs ONCE; psi keeps
  // its result until pass 2 has taken r_0 from it again
  double t_setup = now_s();
  T* stage = nullptr;
  if (P.init_vector_dev) {
    LL_HIP(hipMemcpyAsync(rc.vec(0), P.init_vector_dev, vbytes, hipMemcpyDeviceToDevice, s));
  } else {
    stage = (T*)ctx->ensure_stage(std::max<size_t>(vbytes, sizeof(T)));
    if (P.init_vector) P.init_vector(stage, nl, op->row_begin, P.init_user);
    else random_start<T>(stage, nl);
    T* const first = psi ? psi : rc.vec(0);
    LL_HIP(hipMemcpyAsync(first, stage, vbytes, hipMemcpyHostToDevice, s));
    if (psi) LL_HIP(hipMemcpyAsync(rc.vec(0), psi, vbytes, hipMemcpyDeviceToDevice, s));
  }
  E.norm2_dev(rc.vec(0), rc.c(0));
  std::vector<double> csq(1);  // c_k on the host
  E.fetch(rc.c(0), csq.data(), 1);
  LL_REQUIRE(csq[0] > 0.0 && std::isfinite(csq[0]), "the start vector is zero or not finite");
  t_setup = now_s() - t_setup;

  // ---- pass 1
  RitzTracker cfg;
  cfg.nroot = 1;
  cfg.find_maximum = P.find_maximum != 0;
  cfg.mode = P.tridiag_mode;
  cfg.eps = P.eps;
  cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon() * 1e1;  // H3 LL:279
  std::vector<double> alpha, beta;
  RitzTracker::Out last;
  double t_tridiag = 0.0, t_enqueue = 0.0, t_wait = 0.0;
  {
    TridiagWorker worker(cfg, threaded_verdicts(ctx, op), ctx->tune.tridiag_test_jitter_us);
    RecurPassTimes pt;
    recur_pass1(rc, worker, ring, P.max_iteration, alpha, beta, csq, last, pt);
    t_tridiag += pt.tridiag;
    t_enqueue = pt.enqueue;
    t_wait = pt.wait;
  }
  const int64_t m = last.m;  // iterations the device ran ahead of the verdict are dropped
  alpha.resize((size_t)m);
  beta.resize((size_t)m);
  LL_HIP(hipStreamSynchronize(s));

  // ---- the Ritz pair of T_m (LL:312-319)
  const double t_fin0 = now_s();
  double theta = last.evs[0];  // of the shifted operator
  if (P.tridiag_mode == LL_TRIDIAG_AUTO && !last.evs_from_qr) {  // as lanczos_run: the values of the reference's QR arithmetic
    std::vector<double> all((size_t)m);
    const double t0 = now_s();
    tridiag_qr(m, alpha.data(), beta.data(), all.data(), nullptr);
    t_tridiag += now_s() - t0;
    theta = P.find_maximum ? all[(size_t)m - 1] : all[0];
  }
  double residual = std::numeric_limits<double>::quiet_NaN();
  long long mismatches = 0;
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
    t_tridiag += now_s() - t0;
    std::vector<double> g((size_t)m + 1, 0.0);  // psi = sum_k g_k r_k, g_k = s_k / ||r_k||
    for (int64_t k = 0; k < m; ++k) g[(size_t)k] = sv[(size_t)k] / std::sqrt(csq[(size_t)k]);
    DevBuf<double> gdev;
    DevBuf<long long> mism;
    gdev.alloc(ctx, g.size());
    mism.alloc(ctx, 2);
    LL_HIP(hipMemcpyAsync(gdev.p, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice, s));
    LL_HIP(hipMemsetAsync(mism.p, 0, 2 * sizeof(long long), s));

    // ---- pass 2: r_0 again, psi = g_0 r_0, then the replay
    if (P.init_vector_dev) {
      LL_HIP(hipMemcpyAsync(rc.vec(0), P.init_vector_dev, vbytes, hipMemcpyDeviceToDevice, s));
      LL_HIP(hipMemcpyAsync(psi, P.init_vector_dev, vbytes, hipMemcpyDeviceToDevice, s));
    } else {
      LL_HIP(hipMemcpyAsync(rc.vec(0), psi, vbytes, hipMemcpyDeviceToDevice, s));
    }
    launch_scale<T>(nl, psi, g[0], nullptr, s);
    for (int64_t k = 0; k + 1 < m; ++k) {
      const typename Engine<T>::DeferredAlpha da = rc.operate(k);
      launch_recur_accum<T>(nl, rc.vec(k + 1), rc.vec(k), k > 0 ? rc.vec(k + 2) : nullptr, psi, rc.rec.p, gdev.p, k, 0.0, 0.0, 0.0,
                            da.partials, da.nparts, mism.p, s);
    }
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
    LL_HIP(hipMemcpyAsync(&mismatches, mism.p, sizeof(long long), hipMemcpyDeviceToHost, s));
    if (!out_dev) {
      if (!stage) stage = (T*)ctx->ensure_stage(std::max<size_t>(vbytes, sizeof(T)));
      LL_HIP(hipMemcpyAsync(stage, psi, vbytes, hipMemcpyDeviceToHost, s));
      LL_HIP(hipStreamSynchronize(s));
      host_copy(eigvec, stage, vbytes);
    }
    LL_HIP(hipStreamSynchronize(s));
  }
  const double t_finish = now_s() - t_fin0;

  *eigval_out = theta - P.eigenvalue_offset;  // LL:317-319
  if (itern_out) *itern_out = m;
  if (residual_out) *residual_out = residual;
  if (alpha_out) std::copy(alpha.begin(), alpha.end(), alpha_out);
  if (beta_out) std::copy(beta.begin(), beta.end(), beta_out);
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->n_passes = 1;
    stats->total_iterations = m;
    stats->last_alpha_len = m;
    stats->seconds_host_tridiag = t_tridiag;
    stats->seconds_host_enqueue = t_enqueue;
    stats->seconds_host_wait = t_wait;
    stats->seconds_setup = t_setup;
    stats->seconds_finish = t_finish;
    stats->workspace_vectors = workspace_vectors;
    stats->replay_mismatches = (int64_t)mismatches;
    stats->seconds_total = now_s() - t_start;
  }
  ctx->drain_comm_events(nullptr, nullptr);
}

#define LL_INST_TWO_PASS_RUN(T)                                                                                              \
  template void two_pass_run<T>(ll_context*, ll_operator*, const ll_lanczos_params&, double*, T*, int64_t*, double*, double*, \
                                double*, ll_run_stats*);
LL_FOR_EACH_SCALAR(LL_INST_TWO_PASS_RUN)

}  // namespace ll
