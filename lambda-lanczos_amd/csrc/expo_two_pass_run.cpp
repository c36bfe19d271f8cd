// Exponentiator<T>::run (EX:87-173) WITHOUT a stored Krylov basis: with the reference's default, full_orthogonalize =
// false, its loop IS the plain three-term recurrence, so the two-pass machinery of the eigen-solver (recurrence.hpp, recur.hip) runs
// it unchanged.  Pass 1: r_0 = input, unnormalised, on three rotating vectors, with the Exponentiator's stop rule (ExpoTracker,
// EX:124-158) on the recorded tridiagonal.  Between the passes the host turns the tracker's coeff = exp(a T_m) e_1 into
//   g_k = ||input|| coeff[k] / ||r_k||     (g_0 = coeff[0]),      output = sum_k g_k r_k = ||input|| sum_k coeff[k] u_k  (EX:163-170).
// Pass 2 replays the recurrence from the record, bit for bit, and accumulates that sum in the caller's buffer.  Memory: three
// vectors (four with a host output) against one per iteration plus one for expo_run; the price is every operator application twice.
#include "recurrence.hpp"

namespace ll {
namespace {

// the device image of the coefficients g_k: doubles on real vectors, (re, im) pairs on complex ones
template <typename T> struct ReplayCoeff {
  typedef double type;
  static double of(double g) { return g; }
};
template <> struct ReplayCoeff<zc> {
  typedef zc type;
  static zc of(std::complex<double> g) { return zc{g.real(), g.imag()}; }
};
template <> struct ReplayCoeff<cf> : ReplayCoeff<zc> {};

}  // namespace

template <typename T>
void expo_two_pass_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P_in, typename host_scalar<T>::type a,
                       const T* input, T* output, int64_t* itern_out, ll_run_stats* stats) {
  typedef typename host_scalar<T>::type H;
  typedef typename ReplayCoeff<T>::type G;
  ll_expo_params P = P_in;
  check_run<T>(ctx, op, P, 1e2);  // EX:58
  LL_REQUIRE(P.full_orthogonalize == 0,
             "full_orthogonalize must be 0 for the two-pass Exponentiator: there is no stored basis to orthogonalise against");
  LL_REQUIRE(ctx->comm == nullptr, "the two-pass Exponentiator does not run on sharded contexts yet");
  LL_HIP(hipSetDevice(ctx->device));
  const double t_start = now_s();
  hipStream_t s = ctx->stream;
  const int64_t nl = op->n_local;
  const int64_t ld = round_up(std::max<int64_t>(std::max(nl, op->n_shard), 1), 256);
  const size_t vbytes = (size_t)nl * sizeof(T);
  const bool out_dev = is_device_ptr(output);

  Engine<T> E(ctx, op, nl);
  Recurrence<T> rc{E, s, nl, 0.0, E.can_scale_input(), {}, {}, 0};
  for (auto& b : rc.buf) b.alloc(ctx, (size_t)ld);
  DevBuf<T> out_own;
  int64_t workspace_vectors = 3;
  if (!out_dev) {
    out_own.alloc(ctx, (size_t)ld);
    ++workspace_vectors;
  }
  T* const out = out_dev ? output : out_own.p;  // (may be the input's buffer: it is read for the last time before out is written)
  ctx->ensure_pinned(kPinnedScalars);
  ctx->ensure_partials((size_t)kMaxGrid * Engine<T>::R);
  ctx->ensure_h(4);
  EventRing ring;
  rc.ensure_rec(std::min<int64_t>(P.max_iteration, 4095));

  // ---- r_0 = input (EX:100 without the normalisation), c_0 = ||input||^2 (kept for the output scaling, EX:165)
  double t_setup = now_s();
  LL_HIP(hipMemcpyAsync(rc.vec(0), input, vbytes, hipMemcpyDefault, s));
  E.norm2_dev(rc.vec(0), rc.c(0));
  std::vector<double> csq(1);  // c_k on the host
  E.fetch(rc.c(0), csq.data(), 1);
  LL_REQUIRE(csq[0] > 0.0 && std::isfinite(csq[0]), "the input vector is zero or not finite");
  const double in_norm = std::sqrt(csq[0]);
  t_setup = now_s() - t_setup;

  // ---- pass 1 (EX:107-118, 145, 160) with the stop rule of EX:124-158
  ExpoTracker<H> cfg;
  cfg.a = a;
  cfg.eps = P.eps;
  cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon();  // EX:154
  std::vector<double> alpha, beta;
  typename ExpoTracker<H>::Out last;
  RecurPassTimes pt;
  {
    StepWorker<ExpoTracker<H>> worker(cfg, threaded_verdicts(ctx, op), ctx->tune.tridiag_test_jitter_us);
    recur_pass1(rc, worker, ring, P.max_iteration, alpha, beta, csq, last, pt);
  }
  const int64_t m = last.m;  // iterations the device ran ahead of the verdict are dropped
  LL_HIP(hipStreamSynchronize(s));

  // ---- g_k = ||input|| coeff[k] / ||r_k||: the ratio is exactly 1 at k = 0
  const double t_fin0 = now_s();
  std::vector<G> g((size_t)m + 1, G());
  for (int64_t k = 0; k < m; ++k) g[(size_t)k] = ReplayCoeff<T>::of(last.coeff[(size_t)k] * (in_norm / std::sqrt(csq[(size_t)k])));
  DevBuf<G> gdev;
  DevBuf<long long> mism;
  gdev.alloc(ctx, g.size());
  mism.alloc(ctx, 2);
  LL_HIP(hipMemcpyAsync(gdev.p, g.data(), g.size() * sizeof(G), hipMemcpyHostToDevice, s));
  LL_HIP(hipMemsetAsync(mism.p, 0, 2 * sizeof(long long), s));

  // ---- pass 2: r_0 again, out = g_0 r_0, then m - 1 replayed iterations, each with out += g_{k+1} r_{k+1} in the update's sweep
  LL_HIP(hipMemcpyAsync(rc.vec(0), input, vbytes, hipMemcpyDefault, s));
  if constexpr (scalar_traits<T>::is_complex) launch_recur_seed_cplx<T>(nl, out, rc.vec(0), g[0], s);
  else launch_recur_seed<T>(nl, out, rc.vec(0), g[0], s);
  for (int64_t k = 0; k + 1 < m; ++k) {
    const typename Engine<T>::DeferredAlpha da = rc.operate(k);
    T* const p = k > 0 ? rc.vec(k + 2) : nullptr;
    if constexpr (scalar_traits<T>::is_complex)
      launch_recur_accum_cplx<T>(nl, rc.vec(k + 1), rc.vec(k), p, out, rc.rec.p, gdev.p, k, 0.0, 0.0, G(), da.partials, da.nparts, mism.p, s);
    else
      launch_recur_accum<T>(nl, rc.vec(k + 1), rc.vec(k), p, out, rc.rec.p, gdev.p, k, 0.0, 0.0, 0.0, da.partials, da.nparts, mism.p, s);
  }
  long long mismatches = 0;
  LL_HIP(hipMemcpyAsync(&mismatches, mism.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  if (!out_dev) {
    T* const stage = (T*)ctx->ensure_stage(std::max<size_t>(vbytes, sizeof(T)));
    LL_HIP(hipMemcpyAsync(stage, out, vbytes, hipMemcpyDeviceToHost, s));
    LL_HIP(hipStreamSynchronize(s));
    host_copy(output, stage, vbytes);
  }
  LL_HIP(hipStreamSynchronize(s));
  const double t_finish = now_s() - t_fin0;

  *itern_out = m;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->n_passes = 1;
    stats->total_iterations = m;
    stats->last_alpha_len = m;
    stats->seconds_host_tridiag = pt.tridiag;
    stats->seconds_host_enqueue = pt.enqueue;
    stats->seconds_host_wait = pt.wait;
    stats->seconds_setup = t_setup;
    stats->seconds_finish = t_finish;
    stats->workspace_vectors = workspace_vectors;
    stats->replay_mismatches = (int64_t)mismatches;
    stats->seconds_total = now_s() - t_start;
  }
  ctx->drain_comm_events(nullptr, nullptr);
}

#define LL_INST_EXPO_TWO_PASS_RUN(T)                                                                                         \
  template void expo_two_pass_run<T>(ll_context*, ll_operator*, const ll_expo_params&, typename host_scalar<T>::type, const T*, \
                                     T*, int64_t*, ll_run_stats*);
LL_FOR_EACH_SCALAR(LL_INST_EXPO_TWO_PASS_RUN)

}  // namespace ll
