// LambdaLanczos<T>::run (LL:216-366) and run_iteration: the restart loop over Lanczos passes, the Ritz pairs of every pass and the
// EigenPairManager bookkeeping, on the loop machinery of lanczos_loop.hpp.
#include "lanczos_loop.hpp"

namespace ll {

// ================================================================= LambdaLanczos<T>::run
template <typename T>
void lanczos_run(ll_context* ctx, ll_operator* op, const ll_lanczos_params& P_in, double* eigvals, T* eigvecs,
                 int64_t* n_found, int64_t* iter_counts, int64_t iter_cap, double* alpha_out, double* beta_out,
                 ll_run_stats* stats, const IterationSpec<T>* spec) {
  ll_lanczos_params P = P_in;
  check_run<T>(ctx, op, P, 1e3);
  LL_REQUIRE(P.num_eigs >= 1 && P.num_eigs <= P.matrix_size, "num_eigs out of range");
  if (spec) {
    LL_REQUIRE(spec->nroot >= 1 && spec->nroot <= P.matrix_size, "nroot out of range");
    LL_REQUIRE(spec->n_orth >= 0 && (spec->n_orth == 0 || spec->orth_host != nullptr), "bad orthogonalizeTo list");
  }
  LL_REQUIRE(P.num_eigs_per_iteration >= 1, "num_eigs_per_iteration must be >= 1");
  LL_HIP(hipSetDevice(ctx->device));
  const double t_start = now_s();
  hipStream_t s = ctx->stream;
  const int64_t n = op->n, nl = op->n_local;
  const int64_t ld = round_up(std::max(nl, op->n_shard), 256);
  const int mode = P.orth_mode;
  Engine<T> E(ctx, op, nl);

  Basis<T> U;
  U.init(ctx, nl, ld, pick_chunk_vecs(P.initial_vector_size, P.max_iteration, ld * (int64_t)sizeof(T), ctx->tune.slab_bytes));
  DevBuf<T> d_locked, d_ritz;
  int64_t d_ritz_cap = 0;
  if (spec) {
    if (spec->n_orth > 0) d_locked.alloc(ctx, (size_t)spec->n_orth * ld);
  } else if (P.num_eigs > 1) {
    d_locked.alloc(ctx, (size_t)P.num_eigs * ld);
  }
  const int64_t nroot_max = std::min<int64_t>(P.num_eigs_per_iteration, n);
  ctx->ensure_pinned(kPinnedScalars);
  EventRing ring;
  PhaseTimer timer(ctx, s);

  // EigenPairManager (EPM:21-80): best num_eigs pairs, ordered by the comparator
  std::function<bool(double, double)> cmp;
  if (P.find_maximum) cmp = std::greater<double>(); else cmp = std::less<double>();
  std::multimap<double, std::vector<T>, std::function<bool(double, double)>> kept(cmp);

  int64_t passes = 0, total_iters = 0;
  double t_inf_prev = 0.0;  // max over the passes so far of ||T_m||_inf (same numbers on every rank; between 1 and 3 x ||A + offset||_2)
  double t_tridiag = 0.0, t_setup = 0.0, t_finish = 0.0;
  LoopState<T> LS(E, U, ring, timer, nl, s);
  LS.configure(ld, P.max_iteration, mode == LL_ORTH_CGS_DGKS, false);
  std::vector<double> alpha, beta;
  // Pinned staging buffer owned by the context (reused across runs): the init_vector hook fills it directly and the
  // Ritz vectors land in it, so n-sized host<->device copies run at full PCIe rate and nothing n-sized is zero-filled
  // or page-faulted per call.
  T* stage = (T*)ctx->ensure_stage((size_t)std::max<int64_t>(nl, 1) * sizeof(T));
  const bool single_pair = P.num_eigs == 1 && !spec;  // one pass, one survivor: its vector goes stage -> caller directly
  bool result_in_stage = false, result_in_caller = false;
  const bool out_dev = is_device_ptr(eigvecs);
  auto to_caller = [&](T* dst, const T* src_host) {  // host -> the caller's buffer, wherever it lives
    if (out_dev) LL_HIP(hipMemcpy(dst, src_host, (size_t)nl * sizeof(T), hipMemcpyHostToDevice));
    else host_copy(dst, src_host, (size_t)nl * sizeof(T));
  };

  struct TraceFile {  // LL_ITER_TRACE
    FILE* f = nullptr;
    ~TraceFile() {
      if (f) std::fclose(f);
    }
  } trace_holder;
  if (!ctx->tune.iter_trace.empty()) trace_holder.f = std::fopen(ctx->tune.iter_trace.c_str(), "a");
  if (trace_holder.f) std::setvbuf(trace_holder.f, nullptr, _IOLBF, 0);  // line by line: the callback lines (Engine::apply) interleave in order
  FILE* const trace_file = trace_holder.f;

  while (true) {  // restart loop LL:334-354
    const int64_t nroot = spec ? spec->nroot : std::min<int64_t>(P.num_eigs_per_iteration, n - (int64_t)kept.size());  // LL:338
    const double t_pass0 = now_s();
    // ---- start vector (LL:231-234)
    if (P.init_vector_dev) {  // start vector already in HBM (copied: the caller's buffer is left untouched)
      LL_HIP(hipMemcpyAsync(U.vec(0), P.init_vector_dev, (size_t)nl * sizeof(T), hipMemcpyDeviceToDevice, s));
    } else {
      if (P.init_vector) P.init_vector(stage, nl, op->row_begin, P.init_user);
      else random_start<T>(stage, nl);
      LL_HIP(hipMemcpyAsync(U.vec(0), stage, (size_t)nl * sizeof(T), hipMemcpyHostToDevice, s));
    }
    const int64_t L = spec ? spec->n_orth : (int64_t)kept.size();
    if (spec) {
      for (int64_t j = 0; j < L; ++j)  // the caller's orthogonalizeTo, in the caller's order
        LL_HIP(hipMemcpyAsync(d_locked.p + j * ld, spec->orth_host + j * nl, (size_t)nl * sizeof(T), hipMemcpyDefault, s));  // host or device
    } else {
      int64_t j = 0;
      for (auto& kv : kept) {  // comparator order, like MapValueIterable (CM:58-74)
        LL_HIP(hipMemcpyAsync(d_locked.p + j * ld, kv.second.data(), (size_t)nl * sizeof(T), hipMemcpyHostToDevice, s));
        ++j;
      }
    }
    NormRefs refs0;
    if (L > 0) {
      RunList<T> lk;
      lk.ld = ld;
      lk.add(d_locked.p, L);
      refs0 = E.orth(U.vec(0), lk, mode, ThreeTerm<T>::none(), E.S(kScalScratch), nullptr);  // LL:233
    } else {
      E.norm2_dev(U.vec(0), E.S(kScalScratch) + 1);
      refs0 = E.plain_norm(E.S(kScalScratch) + 1);
    }
    launch_scale<T>(nl, U.vec(0), 0.0, &refs0, s);  // LL:234
    t_setup += now_s() - t_pass0;

    // ---- the Lanczos loop (LL:240-310)
    alpha.clear();
    beta.clear();
    std::vector<double> evs, all;
    bool evs_from_qr = true;  // whether `evs` hold the values of the reference's QR arithmetic (else: bisection values)
    int64_t itern = P.max_iteration;
    // One-sweep form against locked vectors: they must be eigenvectors (LoopState::begin_pass measures their residuals);
    // a caller's orthogonalizeTo list (run_iteration) is not, and keeps the two-sweep form.
    std::vector<double> locked_lambda;  // of the operator the loop applies (A + eigenvalue_offset)
    if (!spec)
      for (auto& kv : kept) locked_lambda.push_back(kv.first + P.eigenvalue_offset);
    LS.begin_pass(refs0, d_locked.p, L, locked_lambda.empty() ? nullptr : locked_lambda.data(), P.eigenvalue_offset, t_inf_prev);
    // Host half of iteration j (H1-H4: Ritz values, breakdown, convergence) on the Ritz tracker
    RitzTracker tracker_cfg;
    tracker_cfg.nroot = nroot;
    tracker_cfg.find_maximum = P.find_maximum != 0;
    tracker_cfg.mode = P.tridiag_mode;
    tracker_cfg.eps = P.eps;
    tracker_cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon() * 1e1;  // H3 LL:279
    TridiagWorker worker(tracker_cfg, threaded_verdicts(ctx, op), ctx->tune.tridiag_test_jitter_us);
    RitzTracker::Out last;
    const bool stopped = run_pass(LS, worker, P.max_iteration, P.eigenvalue_offset, mode, true, alpha, beta, last, t_tridiag,
                                  [&](int64_t j, const typename LoopState<T>::Scalars& sc) {
                                    if (trace_file)  // (verdict 2: redone)
                                      std::fprintf(trace_file, "iter %lld %lld %.17g %.17g %.17g %.17g %d\n", (long long)passes,
                                                   (long long)j, sc.alpha, sc.beta2, sc.c0, sc.c1, sc.redone ? 2 : 0);
                                  });
    itern = last.m;  // == max_iteration without a stop (LL:239,312)
    // (the Ritz vectors below need u_0 .. u_{itern-1}; the ones still raw enter the GEMV through their raw vectors)
    const typename LoopState<T>::Tail tail = LS.end_pass(itern, true);
    if (trace_file) {
      std::fprintf(trace_file, "stop %lld %lld %d collected %zu\n", (long long)passes, (long long)itern, (int)stopped, alpha.size());
      std::fflush(trace_file);
    }
    evs = last.evs;
    evs_from_qr = last.evs_from_qr;
    alpha.resize((size_t)itern);  // iterations the device ran ahead of the verdict are dropped
    beta.resize((size_t)itern);
    for (size_t i = 0; i < alpha.size(); ++i)  // ||T||_inf of this pass: the operator-size scale of the next pass's gate
      t_inf_prev = std::max(t_inf_prev, std::fabs(alpha[i]) + (i > 0 ? beta[i - 1] : 0.0) + (i + 1 < alpha.size() ? beta[i] : 0.0));
    LL_HIP(hipStreamSynchronize(s));

    // ---- Ritz pairs (LL:312-319, LL:33-62)
    TraceRange trace_ritz("ll::ritz (tridiagonal eigenvectors + GEMV + copy back)");
    const double t_fin0 = now_s();
    const int64_t m = (int64_t)alpha.size();  // == itern
    (void)itern;
    if (P.tridiag_mode == LL_TRIDIAG_AUTO && !evs_from_qr && m > 0) {
      // the loop ended without a convergence stop (max_iteration or breakdown) while bisection was tracking the
      // roots: return the values of the reference's QR arithmetic, like every other exit of this mode
      all.resize((size_t)m);
      const double t0 = now_s();
      tridiag_qr(m, alpha.data(), beta.data(), all.data(), nullptr);
      t_tridiag += now_s() - t0;
      for (size_t i = 0; i < evs.size(); ++i) evs[i] = P.find_maximum ? all[(size_t)m - i - 1] : all[i];
    }
    const int64_t nev = (int64_t)evs.size();
    // Eigenvectors of T_m: the reference accumulates all m of them by QR (LL:44, O(m^3)); LL_TRIDIAG_AUTO switches to
    // inverse iteration for the few wanted ones once m is large.
    const bool few_vectors = P.tridiag_mode == LL_TRIDIAG_AUTO && m > 256;
    std::vector<double> tev, tq;
    if (!few_vectors) {
      tev.resize((size_t)m);
      tq.resize((size_t)m * m);
      const double t0 = now_s();
      tridiag_qr(m, alpha.data(), beta.data(), tev.data(), tq.data());  // beta[m-1] is never read (LL:314)
      t_tridiag += now_s() - t0;
    }
    const std::vector<double> evs_raw = evs;  // Ritz values of the shifted operator, comparator order
    for (auto& e : evs) e -= P.eigenvalue_offset;  // LL:317-319
    // EigenPairManager::insertEigenpairs (EPM:52-71) decides from the VALUES alone which of the nev new pairs
    // survive; replay it on (value, index) first so that only surviving Ritz vectors are formed and copied to the
    // host (the reference forms all nroot = 5 and throws 4 away when one pair is requested, LL:338, EPM:60-64).
    std::vector<char> survives((size_t)nev, 0);
    bool nothing_added = true;
    {
      std::multimap<double, int64_t, std::function<bool(double, double)>> sim(cmp);
      for (auto& kv : kept) sim.emplace(kv.first, (int64_t)-1);
      for (int64_t i = 0; i < nev; ++i) {
        auto ins = sim.emplace(evs[i], i);
        auto last = sim.end();
        --last;
        if ((int64_t)sim.size() > P.num_eigs) {
          if (ins != last) nothing_added = false;
          sim.erase(last);
        } else {
          nothing_added = false;
        }
      }
      for (auto& kv : sim)
        if (kv.second >= 0) survives[(size_t)kv.second] = 1;
    }
    if (spec) std::fill(survives.begin(), survives.end(), (char)1);  // run_iteration returns every computed pair
    std::vector<int64_t> want;
    for (int64_t i = 0; i < nev; ++i)
      if (survives[(size_t)i]) want.push_back(i);
    const int64_t nw = (int64_t)want.size();
    std::vector<std::vector<T>> xs((size_t)nev);
    if (nw > 0) {
      std::vector<T> coeff((size_t)nw * m);
      if (few_vectors) {
        std::vector<double> lam((size_t)nw), sv((size_t)nw * m);
        for (int64_t w = 0; w < nw; ++w) lam[(size_t)w] = evs_raw[(size_t)want[w]];
        const double t0 = now_s();
        tridiag_inverse_iteration(m, alpha.data(), beta.data(), nw, lam.data(), sv.data());
        t_tridiag += now_s() - t0;
        for (size_t i = 0; i < sv.size(); ++i) from_z(sv[i], &coeff[i]);
      } else {
        for (int64_t w = 0; w < nw; ++w) {
          const int64_t it = P.find_maximum ? m - want[w] - 1 : want[w];
          for (int64_t k = 0; k < m; ++k) from_z(tq[(size_t)it * m + k], &coeff[(size_t)w * m + k]);
        }
      }
      const RunList<T> basis = LS.ritz_basis(tail, m, nw, coeff);
      if (!d_ritz.p || d_ritz_cap < nw) {  // only the surviving vectors are formed; sized by what a pass can return at
        d_ritz_cap = std::max<int64_t>(nw, std::min<int64_t>(nroot_max, spec ? spec->nroot : P.num_eigs));  // most, so that
        d_ritz.alloc(ctx, (size_t)d_ritz_cap * ld);  // repeated runs of one problem reuse ONE cached buffer size
      }
      E.gemv(basis, basis.total(), (int)nw, coeff.data(), d_ritz.p, ld);
      for (int64_t w = 0; w < nw; ++w) {
        E.norm2_dev(d_ritz.p + w * ld, E.S(kScalScratch) + 1);
        const NormRefs nr = E.plain_norm(E.S(kScalScratch) + 1);
        launch_scale<T>(nl, d_ritz.p + w * ld, 0.0, &nr, s);  // LL:58
        if (single_pair && out_dev) {  // the one survivor goes straight to the caller's device buffer
          LL_HIP(hipMemcpyAsync(eigvecs, d_ritz.p + w * ld, (size_t)nl * sizeof(T), hipMemcpyDeviceToDevice, s));
          LL_HIP(hipStreamSynchronize(s));
          result_in_caller = true;
          continue;
        }
        LL_HIP(hipMemcpyAsync(stage, d_ritz.p + w * ld, (size_t)nl * sizeof(T), hipMemcpyDeviceToHost, s));
        LL_HIP(hipStreamSynchronize(s));
        if (single_pair) {
          result_in_stage = true;  // copied to the caller once, at the end
        } else {
          xs[(size_t)want[w]].assign(stage, stage + nl);
        }
      }
    }

    t_finish += now_s() - t_fin0;
    if (passes < iter_cap && iter_counts) iter_counts[passes] = m;
    ++passes;
    total_iters += m;

    if (spec) {  // LL:312-321: hand the pairs back as they are
      for (int64_t i = 0; i < nev; ++i) {
        eigvals[i] = evs[(size_t)i];
        if (eigvecs) to_caller(eigvecs + (size_t)i * nl, xs[(size_t)i].data());
      }
      *n_found = nev;
      break;
    }
    // ---- EigenPairManager::insertEigenpairs (EPM:52-71), now with the vectors of the survivors
    {
      bool check_nothing = true;
      for (int64_t i = 0; i < nev; ++i) {
        auto ins = kept.emplace(evs[i], std::move(xs[(size_t)i]));
        auto last = kept.end();
        --last;
        if ((int64_t)kept.size() > P.num_eigs) {
          if (ins != last) check_nothing = false;
          kept.erase(last);
        } else {
          check_nothing = false;
        }
      }
      (void)check_nothing;
    }
    if (nothing_added) break;    // LL:346-348
    if (P.num_eigs == 1) break;  // LL:350-353
  }

  int64_t cnt = spec ? *n_found : 0;
  for (auto kv = kept.begin(); !spec && kv != kept.end(); ++kv) {  // comparator order (LL:356-365)
    eigvals[cnt] = kv->first;
    if (eigvecs && !(single_pair && result_in_caller)) {
      const T* src = (single_pair && result_in_stage) ? stage : kv->second.data();
      to_caller(eigvecs + (size_t)cnt * nl, src);
    }
    ++cnt;
  }
  *n_found = cnt;
  if (alpha_out) std::copy(alpha.begin(), alpha.end(), alpha_out);
  if (beta_out) std::copy(beta.begin(), beta.end(), beta_out);
  fill_stats(stats, LS, total_iters, alpha.size(), t_tridiag, t_start);
  if (stats) {
    stats->n_passes = passes;
    stats->seconds_setup = t_setup;
    stats->seconds_finish = t_finish;
  }
}

#define LL_INST_LANCZOS_RUN(T)                                                                                         \
  template void lanczos_run<T>(ll_context*, ll_operator*, const ll_lanczos_params&, double*, T*, int64_t*, int64_t*, int64_t, \
                               double*, double*, ll_run_stats*, const IterationSpec<T>*);
LL_FOR_EACH_SCALAR(LL_INST_LANCZOS_RUN)

}  // namespace ll
