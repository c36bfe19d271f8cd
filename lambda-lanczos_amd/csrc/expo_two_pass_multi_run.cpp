// expo_two_pass_run for SEVERAL a on one Krylov space (ll_expo_two_pass_multi): output_j = exp(a_j A) input for
// j < n_times.  The Krylov space of (A, input) does not depend on a, so pass 1 runs once, with the stop rule of EX:124-158 applied
// to every a_j on its own (ExpoMultiTracker: m_j and coeff_j = exp(a_j T_{m_j}) e_1 are frozen where a_j's test fires), until the
// last a_j has fired: m = max_j m_j iterations.  Pass 2 replays m - 1 iterations once; the sweep that forms r_{k+1} adds
// g_{j,k+1} r_{k+1} into output j for every j with k + 1 < m_j and touches no other output (recur_accum_multi_kernel).  Record,
// coefficients, element update and accumulate are those of expo_two_pass_run, so on a device operator (m_j, output_j) are bit for
// bit what that run returns for a_j alone; the operator runs 2 m - 1 times instead of sum_j (2 m_j - 1).  Memory: three vectors,
// plus one per output in host memory.
#include "recurrence.hpp"

namespace ll {
namespace {

template <typename G> G replay_coeff(double g, const G*) { return g; }
inline zc replay_coeff(std::complex<double> g, const zc*) { return zc{g.real(), g.imag()}; }

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace

template <typename T>
void expo_two_pass_multi_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P_in, int64_t n_times,
                             const typename host_scalar<T>::type* a, const T* input, T* const* outputs, int64_t* itern_out,
                             ll_run_stats* stats) {
  typedef typename host_scalar<T>::type H;
  typedef typename RecurCoeff<T>::type G;
  ll_expo_params P = P_in;
  check_run<T>(ctx, op, P, 1e2);  // EX:58
  LL_REQUIRE(n_times >= 1 && n_times <= kRecurMultiMax, "n_times must be between 1 and 16");
  LL_REQUIRE(P.full_orthogonalize == 0,
             "full_orthogonalize must be 0 for the two-pass Exponentiator: there is no stored basis to orthogonalise against");
  LL_REQUIRE(ctx->comm == nullptr, "the two-pass Exponentiator does not run on sharded contexts yet");
  const int ns = (int)n_times;
  const int64_t nl = op->n_local;
  const size_t vbytes = (size_t)nl * sizeof(T);
  for (int j = 0; j < ns; ++j) {
    LL_REQUIRE(outputs[j] != nullptr, "null output");
    LL_REQUIRE((const T*)outputs[j] == input || !ranges_overlap(outputs[j], input, vbytes),
               "an output overlaps the input without being the input's buffer");
    for (int i = 0; i < j; ++i) LL_REQUIRE(!ranges_overlap(outputs[i], outputs[j], vbytes), "two outputs overlap");
  }
  LL_HIP(hipSetDevice(ctx->device));
  const double t_start = now_s();
  hipStream_t s = ctx->stream;
  const int64_t ld = round_up(std::max<int64_t>(std::max(nl, op->n_shard), 1), 256);

  Engine<T> E(ctx, op, nl);
  Recurrence<T> rc{E, s, nl, 0.0, E.can_scale_input(), {}, {}, 0};
  for (auto& b : rc.buf) b.alloc(ctx, (size_t)ld);
  std::vector<DevBuf<T>> out_own((size_t)ns);  // one device vector per output in host memory
  std::vector<T*> out((size_t)ns);
  int64_t workspace_vectors = 3;
  for (int j = 0; j < ns; ++j) {
    if (is_device_ptr(outputs[j])) {
      out[(size_t)j] = outputs[j];  // (may be the input's buffer: it is read for the last time before any output is written)
    } else {
      out_own[(size_t)j].alloc(ctx, (size_t)ld);
      out[(size_t)j] = out_own[(size_t)j].p;
      ++workspace_vectors;
    }
  }
  ctx->ensure_pinned(kPinnedScalars);
  ctx->ensure_partials((size_t)kMaxGrid * Engine<T>::R);
  ctx->ensure_h(4);
  EventRing ring;
  rc.ensure_rec(std::min<int64_t>(P.max_iteration, 4095));

  // ---- r_0 = input, c_0 = ||input||^2
  double t_setup = now_s();
  LL_HIP(hipMemcpyAsync(rc.vec(0), input, vbytes, hipMemcpyDefault, s));
  E.norm2_dev(rc.vec(0), rc.c(0));
  std::vector<double> csq(1);
  E.fetch(rc.c(0), csq.data(), 1);
  LL_REQUIRE(csq[0] > 0.0 && std::isfinite(csq[0]), "the input vector is zero or not finite");
  const double in_norm = std::sqrt(csq[0]);
  t_setup = now_s() - t_setup;

  // ---- pass 1, once, with one stop test per a_j
  ExpoMultiTracker<H> cfg;
  cfg.a.assign(a, a + ns);
  cfg.eps = P.eps;
  cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon();  // EX:154
  std::vector<double> alpha, beta;
  typename ExpoMultiTracker<H>::Out last;
  RecurPassTimes pt;
  {
    StepWorker<ExpoMultiTracker<H>> worker(cfg, threaded_verdicts(ctx, op), ctx->tune.tridiag_test_jitter_us);
    recur_pass1(rc, worker, ring, P.max_iteration, alpha, beta, csq, last, pt);
  }
  const int64_t m = last.m;  // = max_j m_j; iterations the device ran ahead of the verdict are dropped
  LL_HIP(hipStreamSynchronize(s));

  // ---- g_{j,k} = ||input|| coeff_j[k] / ||r_k|| for k < m_j: row j of the device table (the rest of the row is never read)
  const double t_fin0 = now_s();
  const int64_t ldg = m + 1;
  std::vector<G> g((size_t)(ns * ldg), G());
  for (int j = 0; j < ns; ++j)
    for (int64_t k = 0; k < last.mj[(size_t)j]; ++k)
      g[(size_t)(j * ldg + k)] = replay_coeff(last.coeff[(size_t)j][(size_t)k] * (in_norm / std::sqrt(csq[(size_t)k])), (const G*)nullptr);
  DevBuf<G> gdev;
  DevBuf<long long> mism;
  gdev.alloc(ctx, g.size());
  mism.alloc(ctx, 2);
  LL_HIP(hipMemcpyAsync(gdev.p, g.data(), g.size() * sizeof(G), hipMemcpyHostToDevice, s));
  LL_HIP(hipMemsetAsync(mism.p, 0, 2 * sizeof(long long), s));

  // ---- pass 2: r_0 again (before any output is written: one of them may be the input's buffer), out_j = g_{j,0} r_0, then m - 1
  // replayed iterations with the accumulators that are still active
  LL_HIP(hipMemcpyAsync(rc.vec(0), input, vbytes, hipMemcpyDefault, s));
  for (int j = 0; j < ns; ++j) {
    if constexpr (scalar_traits<T>::is_complex) launch_recur_seed_cplx<T>(nl, out[(size_t)j], rc.vec(0), g[(size_t)(j * ldg)], s);
    else launch_recur_seed<T>(nl, out[(size_t)j], rc.vec(0), g[(size_t)(j * ldg)], s);
  }
  for (int64_t k = 0; k + 1 < m; ++k) {
    const typename Engine<T>::DeferredAlpha da = rc.operate(k);
    RecurMultiArgs<T, G> acc = {};
    for (int j = 0; j < ns; ++j)
      if (k + 1 < last.mj[(size_t)j]) {
        acc.psi[acc.count] = out[(size_t)j];
        acc.row[acc.count] = j;
        ++acc.count;
      }
    T* const p = k > 0 ? rc.vec(k + 2) : nullptr;
    if (acc.count > 1) {
      launch_recur_accum_multi<T>(nl, rc.vec(k + 1), rc.vec(k), p, acc, rc.rec.p, gdev.p, ldg, k, 0.0, 0.0, da.partials, da.nparts,
                                  mism.p, s);
    } else {  // one accumulator left: recur_accum_kernel, which is 3 % faster per launch than the multi kernel with a list of one
      const G* const grow = gdev.p + acc.row[0] * ldg;
      if constexpr (scalar_traits<T>::is_complex)
        launch_recur_accum_cplx<T>(nl, rc.vec(k + 1), rc.vec(k), p, acc.psi[0], rc.rec.p, grow, k, 0.0, 0.0, G(), da.partials, da.nparts, mism.p, s);
      else
        launch_recur_accum<T>(nl, rc.vec(k + 1), rc.vec(k), p, acc.psi[0], rc.rec.p, grow, k, 0.0, 0.0, 0.0, da.partials, da.nparts, mism.p, s);
    }
  }
  long long mismatches = 0;
  LL_HIP(hipMemcpyAsync(&mismatches, mism.p, sizeof(long long), hipMemcpyDeviceToHost, s));
  for (int j = 0; j < ns; ++j)
    if (out_own[(size_t)j].p) {
      T* const stage = (T*)ctx->ensure_stage(std::max<size_t>(vbytes, sizeof(T)));
      LL_HIP(hipMemcpyAsync(stage, out[(size_t)j], vbytes, hipMemcpyDeviceToHost, s));
      LL_HIP(hipStreamSynchronize(s));
      host_copy(outputs[j], stage, vbytes);
    }
  LL_HIP(hipStreamSynchronize(s));
  const double t_finish = now_s() - t_fin0;

  if (itern_out)
    for (int j = 0; j < ns; ++j) itern_out[j] = last.mj[(size_t)j];
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

#define LL_INST_EXPO_TWO_PASS_MULTI_RUN(T)                                                                              \
  template void expo_two_pass_multi_run<T>(ll_context*, ll_operator*, const ll_expo_params&, int64_t,                   \
                                           const typename host_scalar<T>::type*, const T*, T* const*, int64_t*, ll_run_stats*);
LL_FOR_EACH_SCALAR(LL_INST_EXPO_TWO_PASS_MULTI_RUN)

}  // namespace ll
