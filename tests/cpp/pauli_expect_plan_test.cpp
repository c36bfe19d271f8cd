// The host-side planning of ll_pauli_expect (lambda-lanczos_amd/csrc/pauli_expect_plan.hpp) against properties that follow from
// what the kernels READ — the slot tables of one batch — and from the definition of an observable, by brute force over small
// cases: every non-zero observable lands in exactly one slot, the groups ascend and keep the caller's order, no batch exceeds B, a
// batch's first slot and every change of x mask load the partner, the back-map is a bijection, the zero rules hold, and the
// folded sign and part equal i^nY — checked by evaluating the definition with complex arithmetic on a random state and comparing
// it with what a kernel would sum from the plan.  Built (plain, and with the address and undefined-behaviour sanitizers) and run by
// tests/test_pauli_expect_plan_host.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "pauli_expect_plan.hpp"

using namespace ll;

struct Term {
  uint64_t x_mask, z_mask;
  double coef;
};

static std::mt19937_64 rng(20261019);
static long long checks = 0, fails = 0;
#define REQUIRE(cond, ...)                          \
  do {                                              \
    ++checks;                                       \
    if (!(cond) && fails++ < 20) {                  \
      std::printf("FAIL line %d: ", __LINE__);      \
      std::printf(__VA_ARGS__);                     \
      std::printf("\n");                            \
    }                                               \
  } while (0)

static int popc(uint64_t v) { return __builtin_popcountll(v); }

// the definition, in complex arithmetic: coef * sum_s Re[conj(psi(s ^ x)) i^nY (-1)^popcount(s & z) psi(s)] over the states of
// `basis` whose partner is in it (in[s]: the state's position, -1 outside)
static double by_definition(const Term& t, const std::vector<uint32_t>& basis, const std::vector<int>& in,
                            const std::vector<std::complex<double>>& psi) {
  static const std::complex<double> iy[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
  const std::complex<double> ph = iy[popc(t.x_mask & t.z_mask) & 3];
  double sum = 0.0;
  for (size_t i = 0; i < basis.size(); ++i) {
    const uint32_t s = basis[i];
    const int j = in[s ^ (uint32_t)t.x_mask];
    if (j < 0) continue;
    const double sign = (popc(s & t.z_mask) & 1) ? -1.0 : 1.0;
    sum += (std::conj(psi[(size_t)j]) * ph * sign * psi[i]).real();
  }
  return t.coef * sum;
}
// what the kernels sum for slot k: per state v = conj(partner) psi(s), the slot's part of it with the parity's sign; then the host's
// folded coefficient
static double by_plan(const PauliExpectPlan& p, size_t k, const std::vector<uint32_t>& basis, const std::vector<int>& in,
                      const std::vector<std::complex<double>>& psi) {
  double sum = 0.0;
  for (size_t i = 0; i < basis.size(); ++i) {
    const uint32_t s = basis[i];
    const int j = in[s ^ p.x[k]];
    if (j < 0) continue;
    const std::complex<double> v = std::conj(psi[(size_t)j]) * psi[i];
    const double part = (p.flags[k] & kExpectSlotImag) ? v.imag() : v.real();
    sum += (popc(s & p.z[k]) & 1) ? -part : part;
  }
  return p.coef[k] * sum;
}

static void test_case(int n_sites, int n_down /* -1: the full space */, bool cplx, int64_t n_obs, int B, int mask_pool) {
  const bool sector = n_down >= 0;
  const uint32_t site_mask = (uint32_t)((1ull << n_sites) - 1);
  std::vector<Term> obs((size_t)n_obs);
  std::vector<uint32_t> pool((size_t)mask_pool);
  for (auto& m : pool) m = (uint32_t)rng() & site_mask;
  for (auto& t : obs) {
    t.x_mask = (rng() % 4 == 0) ? 0 : pool[rng() % pool.size()];  // few distinct x masks: long groups that straddle batches
    t.z_mask = (uint32_t)rng() & site_mask;
    t.coef = (rng() % 7 == 0) ? 0.0 : std::ldexp((double)(int64_t)(rng() % 2001) - 1000.0, -7);
  }
  const PauliExpectPlan p = pauli_expect_plan(cplx, sector, n_obs, obs.data(), B);
#define CASE "n_sites=%d n_down=%d cplx=%d n_obs=%lld B=%d"
#define CASE_ARGS n_sites, n_down, (int)cplx, (long long)n_obs, B
  const int64_t ns = p.nslots();
  REQUIRE(p.batch == B && p.n_obs == n_obs && (int64_t)p.slot.size() == n_obs, CASE ": header", CASE_ARGS);
  REQUIRE((int64_t)p.z.size() == ns && (int64_t)p.flags.size() == ns && (int64_t)p.coef.size() == ns && (int64_t)p.obs.size() == ns,
          CASE ": table lengths", CASE_ARGS);
  // the zero rules, and only they, drop an observable; every other one has exactly one slot and the maps invert each other
  std::vector<int> hits((size_t)n_obs, 0);
  for (int64_t k = 0; k < ns; ++k) {
    const int64_t j = p.obs[(size_t)k];
    REQUIRE(j >= 0 && j < n_obs, CASE ": slot %lld names observable %lld", CASE_ARGS, (long long)k, (long long)j);
    if (j < 0 || j >= n_obs) return;
    ++hits[(size_t)j];
    REQUIRE(p.slot[(size_t)j] == k, CASE ": slot[obs[%lld]] != %lld", CASE_ARGS, (long long)k, (long long)k);
    REQUIRE(p.x[(size_t)k] == obs[(size_t)j].x_mask && p.z[(size_t)k] == obs[(size_t)j].z_mask, CASE ": slot %lld masks", CASE_ARGS,
            (long long)k);
  }
  int64_t nonzero = 0;
  for (int64_t j = 0; j < n_obs; ++j) {
    const Term& t = obs[(size_t)j];
    const bool zero = (!cplx && (popc(t.x_mask & t.z_mask) & 1)) || (sector && (popc(t.x_mask) & 1));
    REQUIRE(zero == pauli_expect_is_zero(t.x_mask, t.z_mask, cplx, sector), CASE ": zero rule of observable %lld", CASE_ARGS, (long long)j);
    REQUIRE(hits[(size_t)j] == (zero ? 0 : 1), CASE ": observable %lld has %d slots", CASE_ARGS, (long long)j, hits[(size_t)j]);
    REQUIRE((p.slot[(size_t)j] < 0) == zero, CASE ": observable %lld slot %lld", CASE_ARGS, (long long)j, (long long)p.slot[(size_t)j]);
    nonzero += zero ? 0 : 1;
  }
  REQUIRE(ns == nonzero, CASE ": %lld slots for %lld observables that need one", CASE_ARGS, (long long)ns, (long long)nonzero);
  // order: x masks ascend, equal masks keep the caller's order
  for (int64_t k = 1; k < ns; ++k) {
    REQUIRE(p.x[(size_t)k - 1] <= p.x[(size_t)k], CASE ": x masks descend at slot %lld", CASE_ARGS, (long long)k);
    if (p.x[(size_t)k - 1] == p.x[(size_t)k])
      REQUIRE(p.obs[(size_t)k - 1] < p.obs[(size_t)k], CASE ": caller's order lost at slot %lld", CASE_ARGS, (long long)k);
  }
  // batches: they tile the slots, none exceeds B, and a kernel that walks one batch alone loads a partner before it uses one
  REQUIRE(p.nbatches() == (ns + B - 1) / B, CASE ": %lld batches", CASE_ARGS, (long long)p.nbatches());
  int64_t covered = 0;
  for (int64_t b = 0; b < p.nbatches(); ++b) {
    const int64_t i0 = p.batch_begin(b), cnt = p.batch_count(b);
    REQUIRE(i0 == covered && cnt >= 1 && cnt <= B, CASE ": batch %lld = [%lld, +%lld)", CASE_ARGS, (long long)b, (long long)i0, (long long)cnt);
    covered += cnt;
    int remote = 0;
    for (int64_t i = i0; i < i0 + cnt && i < ns; ++i) {
      const bool must = i == i0 || p.x[(size_t)i] != p.x[(size_t)i - 1];
      REQUIRE(((p.flags[(size_t)i] & kExpectSlotNewGroup) != 0) == must, CASE ": new-group flag of slot %lld", CASE_ARGS, (long long)i);
      if (must && (p.x[(size_t)i] >> 2) != 0) ++remote;
    }
    REQUIRE(pauli_expect_remote_groups(p, b, 2) == remote, CASE ": remote groups of batch %lld", CASE_ARGS, (long long)b);
  }
  REQUIRE(covered == ns, CASE ": the batches cover %lld of %lld slots", CASE_ARGS, (long long)covered, (long long)ns);
  // the folded sign and part are i^nY: the definition against what a kernel sums from the tables, on a random state
  std::vector<uint32_t> basis;
  std::vector<int> in((size_t)1 << n_sites, -1);
  for (uint32_t s = 0; s <= site_mask; ++s)
    if (!sector || popc(s) == n_down) {
      in[s] = (int)basis.size();
      basis.push_back(s);
    }
  std::vector<std::complex<double>> psi(basis.size());
  for (auto& v : psi) {
    const double re = std::ldexp((double)(int64_t)(rng() % 129) - 64.0, -6), im = std::ldexp((double)(int64_t)(rng() % 129) - 64.0, -6);
    v = cplx ? std::complex<double>(re, im) : std::complex<double>(re, 0.0);  // dyadic: every sum below is exact
  }
  for (int64_t j = 0; j < n_obs; ++j) {
    const double want = by_definition(obs[(size_t)j], basis, in, psi);
    const double got = p.slot[(size_t)j] >= 0 ? by_plan(p, (size_t)p.slot[(size_t)j], basis, in, psi) : 0.0;
    REQUIRE(got == want, CASE ": observable %lld (x %llx z %llx): plan %.17g, definition %.17g", CASE_ARGS, (long long)j,
            (unsigned long long)obs[(size_t)j].x_mask, (unsigned long long)obs[(size_t)j].z_mask, got, want);
    bool imag = false;
    double sign = 0.0;
    pauli_expect_phase(obs[(size_t)j].x_mask, obs[(size_t)j].z_mask, &imag, &sign);
    const int ny = popc(obs[(size_t)j].x_mask & obs[(size_t)j].z_mask) & 3;
    REQUIRE(imag == ((ny & 1) != 0) && sign == ((ny == 1 || ny == 2) ? -1.0 : 1.0), CASE ": phase of observable %lld", CASE_ARGS, (long long)j);
  }
#undef CASE
#undef CASE_ARGS
}

int main() {
  for (int n_sites = 1; n_sites <= 6; ++n_sites)
    for (int n_down = -1; n_down <= n_sites; ++n_down)
      for (int cplx = 0; cplx < 2; ++cplx)
        for (int B : {1, 2, 3, 8, 32})
          for (int64_t n_obs : {0, 1, 2, 7, 33, 100})
            for (int pool : {1, 3, 64}) test_case(n_sites, n_down, cplx != 0, n_obs, B, pool);
  // an empty plan has no batches
  {
    const PauliExpectPlan p = pauli_expect_plan<Term>(true, false, 0, nullptr, 32);
    REQUIRE(p.nslots() == 0 && p.nbatches() == 0, "empty plan");
  }
  // PauliBatches, which both plans and the measuring driver count with: the batches tile [0, nslots) exactly, in order, none empty
  // and none above the batch size; no slots: no batches; a non-positive batch size: no batches
  for (int64_t ns = 0; ns <= 70; ++ns) {
    for (int B : {1, 2, 31, 32, 33}) {
      const PauliBatches bt{ns, B};
      REQUIRE(bt.nslots() == ns && bt.nbatches() == (ns + B - 1) / B, "batches: %lld slots by %d: %lld batches", (long long)ns, B,
              (long long)bt.nbatches());
      REQUIRE(ns != 0 || bt.nbatches() == 0, "batches: no slots, %lld batches", (long long)bt.nbatches());
      int64_t at = 0;
      for (int64_t k = 0; k < bt.nbatches(); ++k) {
        REQUIRE(bt.batch_begin(k) == at && bt.batch_count(k) >= 1 && bt.batch_count(k) <= B,
                "batches: %lld slots by %d: batch %lld begins at %lld with %lld, after %lld", (long long)ns, B, (long long)k,
                (long long)bt.batch_begin(k), (long long)bt.batch_count(k), (long long)at);
        at += bt.batch_count(k);
      }
      REQUIRE(at == ns, "batches: %lld slots by %d: the batches hold %lld", (long long)ns, B, (long long)at);
    }
    for (int B : {0, -1, -32}) REQUIRE((PauliBatches{ns, B}).nbatches() == 0, "batches: %lld slots by %d", (long long)ns, B);
  }
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
