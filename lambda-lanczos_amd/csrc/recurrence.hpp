// The plain three-term recurrence on three rotating, UNNORMALISED vectors that both basis-free drivers run:
// two_pass_run.cpp (the extreme eigenpair) and expo_two_pass_multi_run.cpp (exp(a_j A) v).  Here: the buffers and the operator call
// of one iteration (Recurrence), the host side of pass 1 (recur_pass1: enqueue, collect the scalars, hand T_k to the tracker's
// worker), and the run both drivers are written on (TwoPass: set-up, c_0, pass 1, the replay loop, host outputs, statistics).
// What differs between the two drivers is the tracker (RitzTracker / ExpoMultiTracker), where r_0 comes from and what pass 2
// accumulates.  Kernels: recur.hip.
#pragma once

#include "lanczos_loop.hpp"

#include <optional>

namespace ll {

// The recurrence both passes run: r_k lives in buf[k % 3] (pass 1 and pass 2 use the same buffers in the same rotation), its
// scalars in rec[k] (recur.hip).
template <typename T> struct Recurrence {
  Engine<T>& E;
  hipStream_t s;
  int64_t nl;
  double offset;
  bool op_scales;  // the operator takes r_k with ||r_k||^2; else (callbacks) r_k is normalised in place in front of it
  DevBuf<T> buf[3];
  DevBuf<double> rec;
  int64_t rec_cap = 0;  // records

  T* vec(int64_t k) { return buf[k % 3].p; }
  double* c(int64_t k) { return rec.p + kRecurRec * k + 3; }
  // records 0 .. upto exist.  Growth (doubling, from 4096 iterations) drains the stream: rare, and never inside pass 2
  void ensure_rec(int64_t upto) {
    if (upto < rec_cap) return;
    int64_t cap = std::max<int64_t>(rec_cap, 4096);
    while (cap <= upto) cap *= 2;
    DevBuf<double> grown;
    grown.alloc(E.ctx, (size_t)cap * kRecurRec);
    if (rec.p) {
      LL_HIP(hipStreamSynchronize(s));
      LL_HIP(hipMemcpy(grown.p, rec.p, (size_t)rec_cap * kRecurRec * sizeof(double), hipMemcpyDeviceToDevice));
    }
    std::swap(rec.p, grown.p);
    std::swap(rec.owner, grown.owner);
    std::swap(rec.bytes, grown.bytes);
    rec_cap = cap;
  }
  // buf[(k + 1) % 3] = (A + offset)(r_k / ||r_k||); returns where the partial sums of alpha_k are
  typename Engine<T>::DeferredAlpha operate(int64_t k) {
    typename Engine<T>::DeferredAlpha da;
    double* const alpha = E.S(kScalAlpha + (int)(k % kRingSlots));
    if (op_scales) {
      E.apply(vec(k), vec(k + 1), offset, alpha, true, &da, nullptr, c(k));
    } else {
      const NormRefs nr = E.plain_norm(c(k));
      launch_scale<T>(nl, vec(k), 0.0, &nr, s);
      E.apply(vec(k), vec(k + 1), offset, alpha, true, &da);
    }
    if (da.nparts == 0) {  // apply folded alpha itself: a list of one
      da.partials = alpha;
      da.nparts = 1;
    }
    return da;
  }
};

// Host time of pass 1, by where it went (ll_run_stats)
struct RecurPassTimes {
  double tridiag = 0.0, enqueue = 0.0, wait = 0.0;
};

// Pass 1: iterations 0 .. max_iteration - 1 of the recurrence, from r_0 in rc.vec(0) with c_0 in rc.c(0) and csq = {c_0}.  Per
// iteration: the operator, recur_step_kernel, recur_fold_kernel, an event; alpha_k, beta_k = ||r_{k+1}|| and c_{k+1} are appended to
// alpha / beta / csq as they arrive and T_k goes to the worker's tracker, whose verdicts are absorbed into `last` (the first stop
// verdict wins; else the last iteration's values).  Device operators run one iteration ahead of the scalars that are read
// (speculates): the caller drops what the device ran beyond last.m.
template <typename T, typename Tracker>
void recur_pass1(Recurrence<T>& rc, StepWorker<Tracker>& worker, EventRing& ring, int64_t max_iteration, std::vector<double>& alpha,
                 std::vector<double>& beta, std::vector<double>& csq, typename Tracker::Out& last, RecurPassTimes& t) {
  ll_context* const ctx = rc.E.ctx;
  const bool ahead = speculates(rc.E.op);  // device operators: iteration k + 1 is enqueued before k's scalars are read
  const size_t max_lag = worker.threaded() ? 24 : 0;
  bool stopped = false;
  auto absorb = [&](typename Tracker::Out& o) {
    t.tridiag += o.seconds;
    last = std::move(o);
    return last.stop;
  };
  int64_t enq = 0, col = 0;  // iterations enqueued / collected
  while (!stopped && col < max_iteration) {
    const int64_t target = ahead ? std::min(col + 2, max_iteration) : col + 1;
    const double te0 = now_s();
    for (; enq < target; ++enq) {
      const int64_t k = enq;
      const int slot = (int)(k % kRingSlots);
      rc.ensure_rec(k + 1);
      const typename Engine<T>::DeferredAlpha da = rc.operate(k);
      const int grid = launch_recur_step<T>(rc.nl, rc.vec(k + 1), rc.vec(k), k > 0 ? rc.vec(k + 2) : nullptr, da.partials, da.nparts,
                                            rc.rec.p, k, !rc.op_scales, ctx->partials.get(), rc.s);
      launch_recur_fold(ctx->partials.get(), grid, rc.rec.p, k, ctx->pinned.get() + kSlotScalars * slot, rc.s);
      LL_HIP(hipEventRecord(ring.ev[slot], rc.s));
    }
    t.enqueue += now_s() - te0;
    const int slot = (int)(col % kRingSlots);
    const double tw0 = now_s();
    LL_HIP(hipEventSynchronize(ring.ev[slot]));
    t.wait += now_s() - tw0;
    const volatile double* hp = ctx->pinned.get() + kSlotScalars * slot;
    const double a_k = hp[0], c_next = hp[1];
    alpha.push_back(a_k);
    beta.push_back(std::sqrt(c_next));  // beta_k = ||r_{k+1}||
    csq.push_back(c_next);
    ++col;
    worker.submit(col, alpha.data(), beta.data());
    stopped = worker.consume(col, -1, max_lag, absorb);
  }
  typename Tracker::Out r;
  while (!stopped && worker.wait_pop(r)) stopped = absorb(r);  // the first stop verdict wins; else the last iteration's values
}

// One run of the two passes: what every basis-free driver owns, and the steps they share, in the order they take them.
//   TwoPass tp(ctx, op, offset);  tp.own_vector(b) per output kept in a workspace vector;  tp.prepare(max_iteration);
//   r_0 -> tp.rc.vec(0);  tp.start(t0, noun);  last = tp.pass1(tracker, max_iteration);
//   tp.replay(g, gdev, seed, step);  tp.read_mismatches();  tp.to_host(dst, src) per host output;  sync;  tp.finish(stats)
template <typename T> struct TwoPass {
  ll_context* const ctx;
  ll_operator* const op;
  const double t_start;
  const hipStream_t s;
  const int64_t nl, ld;
  const size_t vbytes;
  Engine<T> E;
  Recurrence<T> rc;
  std::optional<EventRing> ring;
  std::vector<double> alpha, beta, csq;  // of pass 1; csq[k] = c_k = ||r_k||^2
  RecurPassTimes pt;                     // (a driver adds its own host steps to pt.tridiag)
  double t_setup = 0.0, t_fin0 = 0.0;
  int64_t m = 0;  // iterations kept
  int64_t workspace_vectors = 3;
  DevBuf<long long> mism;
  long long mismatches = 0;

  static double begin(ll_context* ctx) {
    LL_HIP(hipSetDevice(ctx->device));
    return now_s();
  }
  TwoPass(ll_context* ctx_, ll_operator* op_, double offset)
      : ctx(ctx_), op(op_), t_start(begin(ctx_)), s(ctx_->stream), nl(op_->n_local),
        ld(round_up(std::max<int64_t>(std::max(nl, op_->n_shard), 1), 256)), vbytes((size_t)nl * sizeof(T)), E(ctx_, op_, nl),
        rc{E, s, nl, offset, E.can_scale_input(), {}, {}, 0} {
    for (auto& b : rc.buf) b.alloc(ctx, (size_t)ld);
  }
  void own_vector(DevBuf<T>& b) {
    b.alloc(ctx, (size_t)ld);
    ++workspace_vectors;
  }
  void prepare(int64_t max_iteration) {
    ctx->ensure_pinned(kPinnedScalars);
    ctx->ensure_partials((size_t)kMaxGrid * Engine<T>::R);
    ctx->ensure_h(4);
    ring.emplace();
    rc.ensure_rec(std::min<int64_t>(max_iteration, 4095));
  }
  // r_0 is in rc.vec(0): c_0 = ||r_0||^2 to the record and the host; t0: when the driver began to bring r_0 there
  void start(double t0, const char* refusal) {
    E.norm2_dev(rc.vec(0), rc.c(0));
    csq.resize(1);
    E.fetch(rc.c(0), csq.data(), 1);
    LL_REQUIRE(csq[0] > 0.0 && std::isfinite(csq[0]), refusal);
    t_setup = now_s() - t0;
  }
  template <typename Tracker> typename Tracker::Out pass1(const Tracker& cfg, int64_t max_iteration) {
    typename Tracker::Out last;
    {
      StepWorker<Tracker> worker(cfg, threaded_verdicts(ctx, op), ctx->tune.tridiag_test_jitter_us);
      recur_pass1(rc, worker, *ring, max_iteration, alpha, beta, csq, last, pt);
    }
    m = last.m;  // iterations the device ran ahead of the verdict are dropped
    LL_HIP(hipStreamSynchronize(s));
    t_fin0 = now_s();
    return last;
  }
  // Pass 2: the coefficient table to the device; seed() brings r_0 back to rc.vec(0) and enqueues the first term of the sum; then
  // m - 1 replayed iterations, each the operator and step(k, y = r_{k+1}, x = r_k, p = r_{k-1} or nullptr, da, mism), which
  // launches the update with its accumulate
  template <typename G, typename Seed, typename Step> void replay(const std::vector<G>& g, DevBuf<G>& gdev, Seed&& seed, Step&& step) {
    gdev.alloc(ctx, g.size());
    mism.alloc(ctx, 2);
    LL_HIP(hipMemcpyAsync(gdev.p, g.data(), g.size() * sizeof(G), hipMemcpyHostToDevice, s));
    LL_HIP(hipMemsetAsync(mism.p, 0, 2 * sizeof(long long), s));
    seed();
    for (int64_t k = 0; k + 1 < m; ++k) {
      const typename Engine<T>::DeferredAlpha da = rc.operate(k);
      step(k, rc.vec(k + 1), rc.vec(k), k > 0 ? rc.vec(k + 2) : nullptr, da, mism.p);
    }
  }
  void read_mismatches() { LL_HIP(hipMemcpyAsync(&mismatches, mism.p, sizeof(long long), hipMemcpyDeviceToHost, s)); }
  void to_host(T* dst, const T* src) {
    T* const stage = (T*)ctx->ensure_stage(std::max<size_t>(vbytes, sizeof(T)));
    LL_HIP(hipMemcpyAsync(stage, src, vbytes, hipMemcpyDeviceToHost, s));
    LL_HIP(hipStreamSynchronize(s));
    host_copy(dst, stage, vbytes);
  }
  void finish(ll_run_stats* stats) {
    if (stats) {
      std::memset(stats, 0, sizeof(*stats));
      stats->n_passes = 1;
      stats->total_iterations = m;
      stats->last_alpha_len = m;
      stats->seconds_host_tridiag = pt.tridiag;
      stats->seconds_host_enqueue = pt.enqueue;
      stats->seconds_host_wait = pt.wait;
      stats->seconds_setup = t_setup;
      stats->seconds_finish = now_s() - t_fin0;
      stats->workspace_vectors = workspace_vectors;
      stats->replay_mismatches = (int64_t)mismatches;
      stats->seconds_total = now_s() - t_start;
    }
    ctx->drain_comm_events(nullptr, nullptr);
  }
};

}  // namespace ll
