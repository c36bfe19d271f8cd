// Exponentiator<T>::run (EX:87-173) WITHOUT a stored Krylov basis, for one a (ll_expo_two_pass) or SEVERAL a on one
// Krylov space (ll_expo_two_pass_multi): output_j = exp(a_j A) input for j < n_times.  With the reference's default,
// full_orthogonalize = false, its loop IS the plain three-term recurrence, so the two-pass machinery of the eigen-solver
// (recurrence.hpp, recur.hip) runs it unchanged.  The Krylov space of (A, input) does not depend on a, so pass 1 runs once: r_0 =
// input, unnormalised, on three rotating vectors, with the stop rule of EX:124-158 applied to every a_j on its own
// (ExpoMultiTracker: m_j and coeff_j = exp(a_j T_{m_j}) e_1 are frozen where a_j's test fires), until the last a_j has fired:
// m = max_j m_j iterations.  Between the passes the host turns the coefficients into
//   g_{j,k} = ||input|| coeff_j[k] / ||r_k||   (g_{j,0} = coeff_j[0]),   output_j = sum_k g_{j,k} r_k = ||input|| sum_k coeff_j[k] u_k
// (EX:163-170).  Pass 2 replays m - 1 iterations from the record, bit for bit; the sweep that forms r_{k+1} adds g_{j,k+1} r_{k+1}
// into output j for every j with k + 1 < m_j and touches no other output (recur_accum_multi_kernel; recur_accum_kernel where one
// accumulator is active, as in every launch of a single-time run).  On a device operator (m_j, output_j) are bit for bit what a run
// for a_j alone returns; the operator runs 2 m - 1 times instead of sum_j (2 m_j - 1).  Memory: three vectors, plus one per output
// in host memory, against one per iteration plus one for expo_run.
#include "recurrence.hpp"

namespace ll {
namespace {

bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// the refusals both entry points share, behind check_run
void require_two_pass_expo(const ll_context* ctx, const ll_expo_params& P) {
  LL_REQUIRE(P.full_orthogonalize == 0,
             "full_orthogonalize must be 0 for the two-pass Exponentiator: there is no stored basis to orthogonalise against");
  LL_REQUIRE(ctx->comm == nullptr, "the two-pass Exponentiator does not run on sharded contexts yet");
}

// The run behind both entry points; P is checked, ns >= 1 outputs are not null.  An output may be the input's buffer, or overlap it
// in host memory: the input is read for the last time before any output is written.
template <typename T>
void expo_two_pass(ll_context* ctx, ll_operator* op, const ll_expo_params& P, int ns, const typename host_scalar<T>::type* a,
                   const T* input, T* const* outputs, int64_t* itern_out, ll_run_stats* stats) {
  typedef typename host_scalar<T>::type H;
  typedef typename RecurCoeff<T>::type G;
  TwoPass<T> tp(ctx, op, 0.0);
  Recurrence<T>& rc = tp.rc;
  hipStream_t s = tp.s;
  const int64_t nl = tp.nl;
  std::vector<DevBuf<T>> out_own((size_t)ns);  // one device vector per output in host memory
  std::vector<T*> out((size_t)ns);
  for (int j = 0; j < ns; ++j) {
    if (is_device_ptr(outputs[j])) {
      out[(size_t)j] = outputs[j];
    } else {
      tp.own_vector(out_own[(size_t)j]);
      out[(size_t)j] = out_own[(size_t)j].p;
    }
  }
  tp.prepare(P.max_iteration);

  // ---- r_0 = input (EX:100 without the normalisation), c_0 = ||input||^2 (kept for the output scaling, EX:165)
  const double t_setup0 = now_s();
  LL_HIP(hipMemcpyAsync(rc.vec(0), input, tp.vbytes, hipMemcpyDefault, s));
  tp.start(t_setup0, "the input vector is zero or not finite");
  const double in_norm = std::sqrt(tp.csq[0]);

  // ---- pass 1 (EX:107-118, 145, 160), once, with one stop test per a_j
  ExpoMultiTracker<H> cfg;
  cfg.a.assign(a, a + ns);
  cfg.eps = P.eps;
  cfg.breakdown_tol = (double)std::numeric_limits<typename scalar_traits<T>::real>::epsilon();  // EX:154
  const typename ExpoMultiTracker<H>::Out last = tp.pass1(cfg, P.max_iteration);
  const int64_t m = tp.m;  // = max_j m_j

  // ---- g_{j,k} for k < m_j: row j of the device table (the rest of the row is never read); the ratio is exactly 1 at k = 0
  const int64_t ldg = m + 1;
  std::vector<G> g((size_t)(ns * ldg), G());
  for (int j = 0; j < ns; ++j)
    for (int64_t k = 0; k < last.mj[(size_t)j]; ++k)
      g[(size_t)(j * ldg + k)] = RecurCoeff<T>::of(last.coeff[(size_t)j][(size_t)k] * (in_norm / std::sqrt(tp.csq[(size_t)k])));
  DevBuf<G> gdev;
  // ---- pass 2: r_0 again (before any output is written), out_j = g_{j,0} r_0, then m - 1 replayed iterations with the accumulators
  // that are still active
  tp.replay(
      g, gdev,
      [&] {
        LL_HIP(hipMemcpyAsync(rc.vec(0), input, tp.vbytes, hipMemcpyDefault, s));
        for (int j = 0; j < ns; ++j) launch_recur_seed<T>(nl, out[(size_t)j], rc.vec(0), g[(size_t)(j * ldg)], s);
      },
      [&](int64_t k, T* y, const T* x, const T* p, const typename Engine<T>::DeferredAlpha& da, long long* mism) {
        int count = 0, only = 0;
        for (int j = 0; j < ns; ++j)
          if (k + 1 < last.mj[(size_t)j]) {
            only = j;
            ++count;
          }
        if (count > 1) {
          RecurMultiArgs<T, G> acc = {};
          for (int j = 0; j < ns; ++j)
            if (k + 1 < last.mj[(size_t)j]) {
              acc.psi[acc.count] = out[(size_t)j];
              acc.row[acc.count] = j;
              ++acc.count;
            }
          launch_recur_accum_multi<T>(nl, y, x, p, acc, rc.rec.p, gdev.p, ldg, k, 0.0, 0.0, da.partials, da.nparts, mism, s);
        } else {  // one accumulator left: recur_accum_kernel, which is 3 % faster per launch than the multi kernel with a list of one
          launch_recur_accum<T>(nl, y, x, p, out[(size_t)only], rc.rec.p, gdev.p + only * ldg, k, 0.0, 0.0, G(), da.partials, da.nparts,
                                mism, s);
        }
      });
  tp.read_mismatches();
  for (int j = 0; j < ns; ++j)
    if (out_own[(size_t)j].p) tp.to_host(outputs[j], out[(size_t)j]);
  LL_HIP(hipStreamSynchronize(s));

  if (itern_out)
    for (int j = 0; j < ns; ++j) itern_out[j] = last.mj[(size_t)j];
  tp.finish(stats);
}

}  // namespace

template <typename T>
void expo_two_pass_multi_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P_in, int64_t n_times,
                             const typename host_scalar<T>::type* a, const T* input, T* const* outputs, int64_t* itern_out,
                             ll_run_stats* stats) {
  ll_expo_params P = P_in;
  check_run<T>(ctx, op, P, 1e2);  // EX:58
  LL_REQUIRE(n_times >= 1 && n_times <= kRecurMultiMax, "n_times must be between 1 and 16");
  require_two_pass_expo(ctx, P);
  const size_t vbytes = (size_t)op->n_local * sizeof(T);
  for (int j = 0; j < (int)n_times; ++j) {
    LL_REQUIRE(outputs[j] != nullptr, "null output");
    LL_REQUIRE((const T*)outputs[j] == input || !ranges_overlap(outputs[j], input, vbytes),
               "an output overlaps the input without being the input's buffer");
    for (int i = 0; i < j; ++i) LL_REQUIRE(!ranges_overlap(outputs[i], outputs[j], vbytes), "two outputs overlap");
  }
  expo_two_pass<T>(ctx, op, P, (int)n_times, a, input, outputs, itern_out, stats);
}

// One time: the same run with a list of one.  This entry point makes no demand on how the output lies to the input, and always
// reports the iteration count.
template <typename T>
void expo_two_pass_run(ll_context* ctx, ll_operator* op, const ll_expo_params& P_in, typename host_scalar<T>::type a,
                       const T* input, T* output, int64_t* itern_out, ll_run_stats* stats) {
  ll_expo_params P = P_in;
  check_run<T>(ctx, op, P, 1e2);  // EX:58
  require_two_pass_expo(ctx, P);
  int64_t m = 0;
  expo_two_pass<T>(ctx, op, P, 1, &a, input, &output, &m, stats);
  *itern_out = m;
}

#define LL_INST_EXPO_TWO_PASS_RUN(T)                                                                                            \
  template void expo_two_pass_multi_run<T>(ll_context*, ll_operator*, const ll_expo_params&, int64_t,                           \
                                           const typename host_scalar<T>::type*, const T*, T* const*, int64_t*, ll_run_stats*); \
  template void expo_two_pass_run<T>(ll_context*, ll_operator*, const ll_expo_params&, typename host_scalar<T>::type, const T*, \
                                     T*, int64_t*, ll_run_stats*);
LL_FOR_EACH_SCALAR(LL_INST_EXPO_TWO_PASS_RUN)

}  // namespace ll
