// Exponentiator<T>::run (EX:87-173) on the loop machinery of lanczos_loop.hpp, and Exponentiator<T>::taylor_run (EX:175-210).
#include "lanczos_loop.hpp"

namespace ll {
namespace {

// LL_STALL_TRACE=ms: a whole-loop call that takes longer than that prints where its time went (host timestamps at
// the phase boundaries) — for hunting one-off runtime stalls in launch-bound runs.
struct StallTrace {
  double limit_s = -1.0;
  const char* what;
  std::vector<std::pair<const char*, double>> pts;
  StallTrace(const char* w, double limit_ms) : what(w) {
    if (limit_ms >= 0) limit_s = limit_ms * 1e-3;
    if (limit_s >= 0) pts.emplace_back("start", now_s());
  }
  void at(const char* label) {
    if (limit_s >= 0) pts.emplace_back(label, now_s());
  }
  ~StallTrace() {
    if (limit_s < 0 || pts.size() < 2 || pts.back().second - pts.front().second < limit_s) return;
    std::fprintf(stderr, "[ll stall] %s took %.2f ms:", what, (pts.back().second - pts.front().second) * 1e3);
    for (size_t i = 1; i < pts.size(); ++i) std::fprintf(stderr, " %s +%.2f", pts[i].first, (pts[i].second - pts[i - 1].second) * 1e3);
    std::fprintf(stderr, "\n");
  }
};

}  // namespace

// ================================================================= Exponentiator<T>::run
template <typename T>
void expo_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P_in, typename host_scalar<T>::type a,
              const T* input, T* output, int64_t* itern_out, ll_run_stats* stats) {
  typedef typename host_scalar<T>::type H;
  ll_expo_params P = P_in;
  check_run<T>(ctx, op, P, 1e2);  // EX:58
  LL_HIP(hipSetDevice(ctx->device));
  const double t_start = now_s();
  hipStream_t s = ctx->stream;
  StallTrace st("expo_run", ctx->tune.stall_trace_ms);
  const int64_t nl = op->n_local;
  const int64_t ld = round_up(std::max(nl, op->n_shard), 256);
  Engine<T> E(ctx, op, nl);
  st.at("engine");
  Basis<T> U;
  U.init(ctx, nl, ld, pick_chunk_vecs(P.initial_vector_size, P.max_iteration, ld * (int64_t)sizeof(T), ctx->tune.slab_bytes));
  st.at("basis");
  ctx->ensure_pinned(kPinnedScalars);
  EventRing ring;
  PhaseTimer timer(ctx, s);
  double t_tridiag = 0.0;
  st.at("events");

  // u[0] = input / ||input||  (EX:100-101); ||input|| is kept for the output scaling (EX:165)
  LL_HIP(hipMemcpyAsync(U.vec(0), input, (size_t)nl * sizeof(T), hipMemcpyDefault, s));
  st.at("input-copy-enqueued");
  E.norm2_dev(U.vec(0), E.S(kScalScratch) + 1);
  double in_norm2 = 0.0;
  E.fetch(E.S(kScalScratch) + 1, &in_norm2, 1);
  st.at("input-norm-fetched");
  const double in_norm = std::sqrt(in_norm2);
  const NormRefs refs0 = E.plain_norm(E.S(kScalScratch) + 1);
  launch_scale<T>(nl, U.vec(0), 0.0, &refs0, s);

  std::vector<double> alpha, beta;
  std::vector<H> coeff_prev;
  int64_t itern = P.max_iteration;

  // Gram-Schmidt against the basis with full_orthogonalize (EX:120-122), and with it the one-sweep forms, exactly as in the
  // eigen-solver loop
  const bool full = P.full_orthogonalize != 0;
  LoopState<T> LS(E, U, ring, timer, nl, s);
  LS.configure(ld, P.max_iteration, full && P.orth_mode == LL_ORTH_CGS_DGKS, !full);
  LS.begin_pass(refs0, nullptr, 0);
  // Host half of iteration j (EX:124-158: exp(a T_j) e_1 and the overlap test, O(j^3)) on the Exponentiator's tracker
  ExpoTracker<H> tracker_cfg;
  tracker_cfg.a = a;
  tracker_cfg.eps = P.eps;
  tracker_cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon();  // EX:154
  StepWorker<ExpoTracker<H>> worker(tracker_cfg, threaded_verdicts(ctx, op), ctx->tune.tridiag_test_jitter_us);
  typename ExpoTracker<H>::Out last;
  // EX:107-118 (+ EX:120-122 with full_orthogonalize), EX:145, EX:160
  run_pass(LS, worker, P.max_iteration, 0.0, P.orth_mode, full, alpha, beta, last, t_tridiag,
           [](int64_t, const typename LoopState<T>::Scalars&) {});
  itern = last.m;
  coeff_prev = last.coeff;
  // (the output below needs u_0 .. u_{m-1}: a pending pair is completed in the basis, a raw basis of the block form enters the GEMV
  // through transformed coefficients)
  const typename LoopState<T>::Tail tail = LS.end_pass((int64_t)coeff_prev.size(), false);
  alpha.resize((size_t)itern);
  beta.resize((size_t)itern);
  st.at("loop");
  LL_HIP(hipStreamSynchronize(s));
  st.at("drained");

  // output = ||input|| * sum_l coeff_prev[l] u[l]  (EX:163-170)
  const int64_t m = (int64_t)coeff_prev.size();
  std::vector<T> c((size_t)m);
  for (int64_t l = 0; l < m; ++l) from_z(H(in_norm) * coeff_prev[l], &c[l]);
  DevBuf<T> d_out;
  d_out.alloc(ctx, (size_t)ld);
  const RunList<T> basis = LS.ritz_basis(tail, m, 1, c);
  st.at("out-alloc");
  E.gemv(basis, m, 1, c.data(), d_out.p, ld);
  LL_HIP(hipMemcpyAsync(output, d_out.p, (size_t)nl * sizeof(T), hipMemcpyDefault, s));
  st.at("gemv+copy-enqueued");
  LL_HIP(hipStreamSynchronize(s));
  st.at("output-done");
  *itern_out = itern;
  fill_stats(stats, LS, itern, alpha.size(), t_tridiag, t_start);
  if (stats) stats->n_passes = 1;
}
#define LL_INST_EXPO_RUN(T)                                                                                            \
  template void expo_run<T>(ll_context*, ll_operator*, const ll_expo_params&, typename host_scalar<T>::type, const T*, T*, \
                            int64_t*, ll_run_stats*);
LL_FOR_EACH_SCALAR(LL_INST_EXPO_RUN)

// ================================================================= Exponentiator<T>::taylor_run (EX:175-210)
template <typename T>
void taylor_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P, typename host_scalar<T>::type a,
                const T* input, T* output, int64_t* nterms_out) {
  typedef typename host_scalar<T>::type H;
  LL_REQUIRE(op && op->ctx == ctx, "operator belongs to another context");
  LL_REQUIRE(op->is_complex == scalar_traits<T>::is_complex && op->elem_bytes == (int)sizeof(T),
             "operator scalar type mismatch");
  LL_REQUIRE(P.matrix_size == op->n, "matrix_size differs from the operator dimension");
  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t nl = op->n_local;
  if (a == H(0)) {  // EX:179-182; input / output may be host or device memory, and may be the same buffer
    if (output != input) {
      LL_HIP(hipMemcpyAsync(output, input, (size_t)nl * sizeof(T), hipMemcpyDefault, s));
      LL_HIP(hipStreamSynchronize(s));
    }
    *nterms_out = 1;
    return;
  }
  const int64_t ld = round_up(std::max(nl, op->n_shard), 256);
  Engine<T> E(ctx, op, nl);
  Basis<T> V;
  V.init(ctx, nl, ld, 32);
  LL_HIP(hipMemcpyAsync(V.vec(0), input, (size_t)nl * sizeof(T), hipMemcpyDefault, s));
  H factor = 1.0;
  int64_t terms = 1;
  for (int64_t k = 1;; ++k) {  // EX:187-195
    factor *= a / H((double)k);
    E.apply(V.vec(k - 1), V.vec(k), 0.0, nullptr, true);
    ++terms;
    E.norm2_dev(V.vec(k), E.S(kScalScratch) + 1);
    double nn = 0.0;
    E.fetch(E.S(kScalScratch) + 1, &nn, 1);
    if (!(std::sqrt(nn) * std::abs(factor) >= P.eps)) break;  // (a term that is not a number ends the series too: the output then says so)
  }
  std::vector<T> c((size_t)terms);
  for (int64_t k = terms; k-- > 0;) {  // backward sum with the reference's factor recurrence (EX:198-206)
    from_z(factor, &c[k]);
    factor *= H((double)k) / a;
  }
  DevBuf<T> d_out;
  d_out.alloc(ctx, (size_t)ld);
  RunList<T> basis;
  basis.ld = ld;
  basis.add_basis(V, terms);
  E.gemv(basis, terms, 1, c.data(), d_out.p, ld);
  LL_HIP(hipMemcpyAsync(output, d_out.p, (size_t)nl * sizeof(T), hipMemcpyDefault, s));
  LL_HIP(hipStreamSynchronize(s));
  *nterms_out = terms;
}
#define LL_INST_TAYLOR_RUN(T)                                                                                          \
  template void taylor_run<T>(ll_context*, ll_operator*, const ll_expo_params&, typename host_scalar<T>::type, const T*, T*, \
                              int64_t*);
LL_FOR_EACH_SCALAR(LL_INST_TAYLOR_RUN)

}  // namespace ll
