// ExpoMultiTracker (csrc/ritz_tracker.hpp) against independent ExpoTrackers, one per time, on the same (alpha, beta) prefixes: the
// tridiagonal of a plain Lanczos run on the 1-D Laplacian with a fixed start vector, generated here.  For H = double and
// H = std::complex<double>:
//   every m_j and every frozen coeff_j equals, by memcmp, what the single tracker for a_j holds at its stop (or at the last prefix
//   where it never stops); `stop` is false before max_j m_j and true at it;
//   breakdown (beta = 0 at m = 3) ends every time there: all m_j = 3;
//   a max_iteration cut (prefixes end before the last time has fired) gives the unfrozen times that m and that coefficient vector;
//   through StepWorker, threaded and unthreaded, consumed the way recur_pass1 does, the last verdict is the inline one;
//   with ONE time the multi tracker IS the single one (ll_expo_two_pass runs on it): at every prefix up to and including the stop,
//   m, stop and the coefficient bytes are the ExpoTracker's, inline and through StepWorker, for a run that stops by overlap, one
//   that breaks down at m = 1 and one cut by the prefixes ending.
// A clean run prints "<checks> checks, 0 failures".
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ritz_tracker.hpp"

namespace {
int checks = 0, failures = 0;
#define CHECK(cond)                                                               \
  do {                                                                            \
    ++checks;                                                                     \
    if (!(cond)) {                                                                \
      ++failures;                                                                 \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);                       \
    }                                                                             \
  } while (0)

// alpha_k, beta_k = ||w_k|| of the plain three-term recurrence on tridiag(-1, 2, -1), n points
void laplace_lanczos(int n, int iters, std::vector<double>& alpha, std::vector<double>& beta) {
  std::vector<double> u((size_t)n), prev((size_t)n, 0.0), w((size_t)n);
  double nrm = 0;
  for (int i = 0; i < n; ++i) u[(size_t)i] = 1.0 + 0.5 * std::sin(0.7 * (i + 1)) + (i % 7 == 0 ? 0.8 : 0.0), nrm += u[(size_t)i] * u[(size_t)i];
  for (double& x : u) x /= std::sqrt(nrm);
  double b_prev = 0.0;
  for (int k = 0; k < iters; ++k) {
    for (int i = 0; i < n; ++i)
      w[(size_t)i] = 2.0 * u[(size_t)i] - (i > 0 ? u[(size_t)(i - 1)] : 0.0) - (i + 1 < n ? u[(size_t)(i + 1)] : 0.0);
    double a = 0;
    for (int i = 0; i < n; ++i) a += u[(size_t)i] * w[(size_t)i];
    double b = 0;
    for (int i = 0; i < n; ++i) {
      w[(size_t)i] -= a * u[(size_t)i] + b_prev * prev[(size_t)i];
      b += w[(size_t)i] * w[(size_t)i];
    }
    b = std::sqrt(b);
    alpha.push_back(a);
    beta.push_back(b);
    prev = u;
    for (int i = 0; i < n; ++i) u[(size_t)i] = w[(size_t)i] / b;
    b_prev = b;
  }
}

template <typename H> struct Single {
  int64_t m = 0;
  bool stopped = false;
  std::vector<H> coeff;
};
// what a single-time run keeps of an ExpoTracker fed the prefixes 1 .. K: the first stop verdict, else the last one
template <typename H>
Single<H> run_single(H a, double eps, double tol, const std::vector<double>& A, const std::vector<double>& B, int64_t K) {
  ll::ExpoTracker<H> t;
  t.a = a;
  t.eps = eps;
  t.breakdown_tol = tol;
  Single<H> r;
  for (int64_t m = 1; m <= K && !r.stopped; ++m) {
    typename ll::ExpoTracker<H>::Out o = t.step(m, A.data(), B.data());
    r.m = o.m;
    r.stopped = o.stop;
    r.coeff = o.coeff;
  }
  return r;
}

template <typename H> bool same_bytes(const std::vector<H>& x, const std::vector<H>& y) {
  return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(H)) == 0);
}

template <typename H> ll::ExpoMultiTracker<H> config(const std::vector<H>& a, double eps, double tol) {
  ll::ExpoMultiTracker<H> cfg;
  cfg.a = a;
  cfg.eps = eps;
  cfg.breakdown_tol = tol;
  return cfg;
}

// the multi tracker inline over the prefixes 1 .. K, against the singles; returns its last verdict
template <typename H>
typename ll::ExpoMultiTracker<H>::Out compare(const char* what, const std::vector<H>& a, double eps, double tol, const std::vector<double>& A,
                                              const std::vector<double>& B, int64_t K) {
  std::vector<Single<H>> single;
  int64_t m_max = 0;
  bool all_stopped = true;
  for (const H& v : a) {
    single.push_back(run_single<H>(v, eps, tol, A, B, K));
    m_max = std::max(m_max, single.back().m);
    all_stopped = all_stopped && single.back().stopped;
  }
  ll::ExpoMultiTracker<H> t = config(a, eps, tol);
  typename ll::ExpoMultiTracker<H>::Out last;
  for (int64_t m = 1; m <= K; ++m) {
    last = t.step(m, A.data(), B.data());
    CHECK(last.m == m);
    CHECK(last.stop == (all_stopped && m == m_max));  // true exactly at max_j m_j
    if (last.stop) break;
  }
  CHECK(last.m == m_max);
  CHECK(last.mj.size() == a.size() && last.coeff.size() == a.size());
  for (size_t j = 0; j < a.size() && j < last.mj.size(); ++j) {
    CHECK(last.mj[j] == single[j].m);
    CHECK(same_bytes(last.coeff[j], single[j].coeff));
    std::printf("%s: time %zu: m = %lld (single %lld%s)\n", what, j, (long long)last.mj[j], (long long)single[j].m,
                single[j].stopped ? "" : ", never stopped");
  }
  return last;
}

// the consumption of recur_pass1 (recurrence.hpp): submit prefix `col`, absorb whatever is there, the first stop verdict wins.
// Returns every verdict absorbed, in order: the prefixes 1 .. stop (or 1 .. K)
template <typename Tracker>
std::vector<typename Tracker::Out> worker_verdicts(const Tracker& cfg, bool threaded, const std::vector<double>& A,
                                                   const std::vector<double>& B, int64_t K) {
  ll::StepWorker<Tracker> worker(cfg, threaded);
  std::vector<typename Tracker::Out> seen;
  std::vector<double> alpha, beta;
  bool stopped = false;
  auto absorb = [&](typename Tracker::Out& o) {
    seen.push_back(std::move(o));
    return seen.back().stop;
  };
  for (int64_t col = 0; !stopped && col < K;) {
    alpha.push_back(A[(size_t)col]);
    beta.push_back(B[(size_t)col]);
    ++col;
    worker.submit(col, alpha.data(), beta.data());
    stopped = worker.consume(col, -1, worker.threaded() ? 24 : 0, absorb);
  }
  typename Tracker::Out r;
  while (!stopped && worker.wait_pop(r)) stopped = absorb(r);
  return seen;
}
template <typename H>
typename ll::ExpoMultiTracker<H>::Out through_worker(const ll::ExpoMultiTracker<H>& cfg, bool threaded, const std::vector<double>& A,
                                                     const std::vector<double>& B, int64_t K) {
  return worker_verdicts(cfg, threaded, A, B, K).back();
}

template <typename H>
void same_verdict(const typename ll::ExpoMultiTracker<H>::Out& x, const typename ll::ExpoMultiTracker<H>::Out& y) {
  CHECK(x.m == y.m && x.stop == y.stop && x.mj == y.mj && x.coeff.size() == y.coeff.size());
  for (size_t j = 0; j < x.coeff.size() && j < y.coeff.size(); ++j) CHECK(same_bytes(x.coeff[j], y.coeff[j]));
}

// ---- one time: the multi tracker's verdict against the single tracker's for the same prefix
template <typename H> void same_as_single(const typename ll::ExpoTracker<H>::Out& s, const typename ll::ExpoMultiTracker<H>::Out& t) {
  CHECK(t.m == s.m);
  CHECK(t.stop == s.stop);
  CHECK(t.mj.size() == 1 && t.mj[0] == s.m);
  CHECK(t.coeff.size() == 1 && same_bytes(t.coeff[0], s.coeff));
}
// both trackers over the prefixes 1 .. K; the run must end at want_m, by a stop verdict or (want_stop == false) by the prefixes ending
template <typename H>
void one_time(const char* what, H a, double eps, double tol, const std::vector<double>& A, const std::vector<double>& B, int64_t K,
              int64_t want_m, bool want_stop) {
  ll::ExpoTracker<H> single;
  single.a = a;
  single.eps = eps;
  single.breakdown_tol = tol;
  const ll::ExpoMultiTracker<H> multi = config<H>({a}, eps, tol);
  {
    ll::ExpoTracker<H> s = single;
    ll::ExpoMultiTracker<H> t = multi;
    int64_t last_m = 0;
    bool stopped = false;
    for (int64_t m = 1; m <= K && !stopped; ++m) {
      const typename ll::ExpoTracker<H>::Out os = s.step(m, A.data(), B.data());
      same_as_single<H>(os, t.step(m, A.data(), B.data()));
      CHECK(os.m == m);
      last_m = m;
      stopped = os.stop;
    }
    CHECK(last_m == want_m);
    CHECK(stopped == want_stop);
    std::printf("%s, one time: m = %lld%s\n", what, (long long)last_m, stopped ? "" : ", never stopped");
  }
  for (bool threaded : {false, true}) {
    const std::vector<typename ll::ExpoTracker<H>::Out> vs = worker_verdicts(single, threaded, A, B, K);
    const std::vector<typename ll::ExpoMultiTracker<H>::Out> vt = worker_verdicts(multi, threaded, A, B, K);
    CHECK((int64_t)vs.size() == want_m);
    CHECK(vt.size() == vs.size());
    for (size_t i = 0; i < vs.size() && i < vt.size(); ++i) {
      CHECK(vs[i].m == (int64_t)i + 1);
      CHECK(vs[i].stop == (want_stop && (int64_t)i + 1 == want_m));
      same_as_single<H>(vs[i], vt[i]);
    }
  }
}
}  // namespace

int main() {
  typedef std::complex<double> Z;
  const double eps = 2.2e-14, tol = 2.2e-16;
  std::vector<double> A, B;
  laplace_lanczos(300, 120, A, B);
  const int64_t K = (int64_t)A.size();

  // ---- complex times, unsorted, one of them zero: every time fires, at different iterations
  const std::vector<Z> tz = {Z(0, -2.0), Z(0, 0), Z(0, -6.0), Z(0, -0.4), Z(0, -2.0)};
  const ll::ExpoMultiTracker<Z>::Out full = compare<Z>("complex", tz, eps, tol, A, B, K);
  CHECK(full.stop);
  CHECK(full.mj.size() == 5 && full.mj[1] == 2 && full.mj[3] < full.mj[0] && full.mj[0] < full.mj[2] && full.mj[4] == full.mj[0]);
  CHECK(full.m < K);
  // ---- a max_iteration cut between the second and the third stop: the times still open carry the cut's m and coefficients
  const int64_t cut = full.mj.size() == 5 ? (full.mj[0] + full.mj[2]) / 2 : 1;
  const ll::ExpoMultiTracker<Z>::Out at_cut = compare<Z>("complex, cut", tz, eps, tol, A, B, cut);
  CHECK(!at_cut.stop && at_cut.m == cut);
  CHECK(at_cut.mj.size() == 5 && at_cut.mj[2] == cut && at_cut.mj[0] == full.mj[0] && at_cut.mj[3] == full.mj[3]);
  // ---- real times: exp(a T) e_1 is no unit vector, the overlap test never fires, every time ends at the cut
  const std::vector<double> td = {-0.5, -0.1, 0.3};
  const ll::ExpoMultiTracker<double>::Out real_cut = compare<double>("real", td, eps, tol, A, B, 40);
  CHECK(!real_cut.stop && real_cut.mj == std::vector<int64_t>(3, 40));
  // ---- breakdown: beta = 0 at m = 3 ends every time there
  {
    const std::vector<double> a4 = {1.0, 2.0, 3.0, 4.0, 5.0}, b4 = {0.5, 0.7, 0.0, 0.9, 0.3};
    const ll::ExpoMultiTracker<Z>::Out bz = compare<Z>("complex, breakdown", {Z(0, -0.5), Z(0, -1.5), Z(0, -1.0)}, eps, tol, a4, b4, 5);
    CHECK(bz.stop && bz.mj == std::vector<int64_t>(3, 3));
    const ll::ExpoMultiTracker<double>::Out bd = compare<double>("real, breakdown", td, eps, tol, a4, b4, 5);
    CHECK(bd.stop && bd.mj == std::vector<int64_t>(3, 3));
  }
  // ---- through StepWorker, unthreaded and threaded (verdicts asked for after the stop are dropped or repeat it)
  for (bool threaded : {false, true}) {
    same_verdict<Z>(through_worker<Z>(config(tz, eps, tol), threaded, A, B, K), full);
    same_verdict<Z>(through_worker<Z>(config(tz, eps, tol), threaded, A, B, cut), at_cut);
    same_verdict<double>(through_worker<double>(config(td, eps, tol), threaded, A, B, 40), real_cut);
  }
  // ---- a tracker that is asked again after its stop repeats the verdict
  {
    ll::ExpoMultiTracker<Z> t = config(tz, eps, tol);
    ll::ExpoMultiTracker<Z>::Out o;
    for (int64_t m = 1; m <= full.m; ++m) o = t.step(m, A.data(), B.data());
    const ll::ExpoMultiTracker<Z>::Out again = t.step(full.m + 1, A.data(), B.data());
    CHECK(again.stop && again.mj == full.mj);
    for (size_t j = 0; j < again.coeff.size(); ++j) CHECK(same_bytes(again.coeff[j], full.coeff[j]));
  }
  // ---- one time: ExpoMultiTracker against ExpoTracker at every prefix, with the three ways a run ends
  {
    const std::vector<double> a1 = {1.0, 2.0, 3.0}, b1 = {0.0, 0.7, 0.9};  // r_1 = 0: breakdown at m = 1
    one_time<Z>("complex, overlap", Z(0, -2.0), eps, tol, A, B, K, full.mj[0], true);
    one_time<Z>("complex, breakdown", Z(0, -2.0), eps, tol, a1, b1, 3, 1, true);
    one_time<Z>("complex, cut", Z(0, -6.0), eps, tol, A, B, cut, cut, false);
    one_time<double>("real, overlap", 0.0, eps, tol, A, B, K, 2, true);  // exp(0 T) e_1 = e_1 at every m: the test fires at m = 2
    one_time<double>("real, breakdown", -0.5, eps, tol, a1, b1, 3, 1, true);
    one_time<double>("real, cut", -0.5, eps, tol, A, B, 40, 40, false);
  }
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
