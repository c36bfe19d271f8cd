// The host side of the matrix-free spin-1/2 family H = sum_t c_t P_t: the term tables, the checks that H commutes with what a
// block assumes, the bases, the six create_pauli* that capi.cpp calls, and launch_pauli_op, the dispatch to the six launchers.
#include <cmath>
#include <thread>
#include <utility>

#include "ll_internal.hpp"
#include "pauli_torus_plan.hpp"

namespace ll {
void check_pauli_string(const char* what, int64_t j, const ll_pauli_term& q, int n_sites) {
  const uint64_t site_mask = ((uint64_t)1 << n_sites) - 1;
  LL_REQUIRE(((q.x_mask | q.z_mask) & ~site_mask) == 0, what + (" " + std::to_string(j)) + ": a mask bit at or above n_sites");
  LL_REQUIRE(std::isfinite(q.coef), what + (" " + std::to_string(j)) + ": the coefficient is not finite");
}

namespace {
// Validate, fold i^nY into the coefficient (a sign for the real types, one of {1, i, -1, -i} for the complex ones), group the
// terms by x mask — groups by ascending mask, the terms of a group in the caller's order.
struct PauliTables {
  std::vector<uint32_t> gx, tz;   // x mask per group, z mask per term
  std::vector<int32_t> gptr;      // [groups + 1] first term of each group
  std::vector<double> tc;         // per term: c i^nY (real types), (re, im) of it (complex types)
  double norm = 0.0;              // sum_t |c_t|
};
template <typename T>
PauliTables pauli_tables(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  use(ctx);
  LL_REQUIRE(out != nullptr, "null argument (out)");
  LL_REQUIRE(n_terms >= 0, "n_terms is negative");
  LL_REQUIRE(terms != nullptr || n_terms == 0, "null argument (terms)");
  LL_REQUIRE(n_sites >= 1 && n_sites <= kPauliMaxSites,
             "n_sites must lie in [1, " + std::to_string(kPauliMaxSites) + "] (2^n_sites states, 32-bit local indices)");
  LL_REQUIRE(ctx->nranks == 1,
             "a sum of Pauli strings cannot be created on a sharded context (flips of the sites that would number the ranks are "
             "exchanges between them, which are not built): use a single-GPU context");
  LL_REQUIRE(n_terms < (int64_t)0x7fffffff, "too many terms");
  constexpr bool cplx = scalar_traits<T>::is_complex;
  std::vector<int64_t> order((size_t)n_terms);
  PauliTables pt;
  for (int64_t t = 0; t < n_terms; ++t) {
    const ll_pauli_term& q = terms[t];
    check_pauli_string("term", t, q, n_sites);
    LL_REQUIRE(cplx || (__builtin_popcountll(q.x_mask & q.z_mask) & 1) == 0,
               "term " + std::to_string(t) + ": an odd number of Y factors makes the matrix complex; use a complex storage type");
    order[(size_t)t] = t;
    pt.norm += std::fabs(q.coef);
  }
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return terms[a].x_mask < terms[b].x_mask; });
  pt.tz.resize((size_t)n_terms);
  pt.tc.resize((size_t)n_terms * (cplx ? 2 : 1));
  for (int64_t k = 0; k < n_terms; ++k) {
    const ll_pauli_term& q = terms[order[(size_t)k]];
    if (pt.gx.empty() || pt.gx.back() != (uint32_t)q.x_mask) {
      pt.gx.push_back((uint32_t)q.x_mask);
      pt.gptr.push_back((int32_t)k);
    }
    pt.tz[(size_t)k] = (uint32_t)q.z_mask;
    const int ny = __builtin_popcountll(q.x_mask & q.z_mask) & 3;  // i^nY: 1, i, -1, -i
    const double c = ny >= 2 ? -q.coef : q.coef;
    if (cplx) {
      pt.tc[2 * (size_t)k] = (ny & 1) ? 0.0 : c;
      pt.tc[2 * (size_t)k + 1] = (ny & 1) ? c : 0.0;
    } else {
      pt.tc[(size_t)k] = c;
    }
  }
  pt.gptr.push_back((int32_t)n_terms);
  return pt;
}
// a host table on the device
template <typename V> void pauli_upload(ll_context* ctx, DevArray<V>& dst, const std::vector<V>& src, const char* what) {
  dst = ctx->dev_alloc<V>(std::max<size_t>(src.size(), 1), what);
  if (!src.empty()) LL_HIP(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice));
}
// What every create_pauli* ends on: the header (n = n_local = dim), nnz = the terms, inf_norm = sum_t |c_t| (a bound of every
// absolute row sum; of every |eigenvalue| of a block: >= ||H||_2 >= ||B^H H B||_2) and the term tables of its image on the device.
template <typename T, typename Image>
std::unique_ptr<ll_operator> pauli_operator(ll_context* ctx, ll_operator::Kind kind, int64_t dim, const PauliTables& pt,
                                            Image ll_operator::*image) {
  std::unique_ptr<ll_operator> op = new_operator<T>(ctx, kind, dim, 0, dim);
  op->nnz = (int64_t)pt.tz.size();
  op->inf_norm = pt.norm;
  PauliTermImage& im = (op.get()->*image).terms;
  im.ngroups = (int)pt.gx.size();
  im.nterms = (int64_t)pt.tz.size();
  pauli_upload(ctx, im.gx, pt.gx, "Pauli x masks");
  pauli_upload(ctx, im.gptr, pt.gptr, "Pauli group offsets");
  pauli_upload(ctx, im.tz, pt.tz, "Pauli z masks");
  pauli_upload(ctx, im.tc, pt.tc, "Pauli coefficients");
  return op;
}

// S_z conservation, group by group: over every assignment of the bits the group touches (its x mask and its z masks) for which
// flipping the x mask changes the number of set bits, the group's weight — summed as the kernel sums it, in double, terms in
// order — must be exactly 0.  R = doubles per coefficient (2: re, im, summed separately as the kernel does).
void pauli_require_sz_conserving(const PauliTables& pt, int R) {
  for (size_t g = 0; g < pt.gx.size(); ++g) {
    const uint32_t X = pt.gx[g];
    if (X == 0) continue;
    char hex[16];
    std::snprintf(hex, sizeof hex, "0x%x", (unsigned)X);
    const std::string who = "the terms with x mask " + std::string(hex);
    uint32_t U = X;
    for (int32_t k = pt.gptr[g]; k < pt.gptr[g + 1]; ++k) U |= pt.tz[(size_t)k];
    LL_REQUIRE(__builtin_popcount(U) <= kPauliSectorMaxSupport,
               who + " act on " + std::to_string(__builtin_popcount(U)) + " sites: the S_z conservation check cannot be made for more than " +
                   std::to_string(kPauliSectorMaxSupport) + " (it visits every assignment of them)");
    const int px = __builtin_popcount(X);
    uint32_t s = 0;
    do {  // every subset s of U
      if (2 * __builtin_popcount(s & X) != px) {
        for (int r = 0; r < R; ++r) {
          double w = 0.0;
          for (int32_t k = pt.gptr[g]; k < pt.gptr[g + 1]; ++k) {
            const double c = pt.tc[(size_t)k * R + r];
            w += (__builtin_popcount((s ^ X) & pt.tz[(size_t)k]) & 1) ? -c : c;
          }
          LL_REQUIRE(w == 0.0, who + " do not conserve S_z (they change the number of flipped spins with a weight that is not "
                                     "zero): a magnetisation sector needs an H that commutes with total S_z");
        }
      }
      s = (s - U) & U;
    } while (s != 0);
  }
}

// The one-site shift and the reflection of a ring of L sites, on a state or on a mask
inline uint64_t ring_rot(uint64_t v, int L) { return ((v << 1) | (v >> (L - 1))) & (((uint64_t)1 << L) - 1); }
inline uint64_t ring_rev(uint64_t v, int L) {
  uint64_t r = 0;
  for (int j = 0; j < L; ++j) r |= ((v >> j) & 1u) << (L - 1 - j);
  return r;
}
// Invariance under the symmetries of the ring, on the caller's terms with the coefficients of equal (x_mask, z_mask) merged (summed
// in the caller's order; i^nY does not change under a site permutation).  A refusal names the first term at fault, then `why`.
struct PauliInvariance {
  int64_t n_terms;
  const ll_pauli_term* terms;
  std::map<std::pair<uint64_t, uint64_t>, double> merged;
  PauliInvariance(int64_t n, const ll_pauli_term* q) : n_terms(n), terms(q) {
    for (int64_t t = 0; t < n; ++t) merged[{q[t].x_mask, q[t].z_mask}] += q[t].coef;
  }
  double coef(int64_t t) const { return merged.at({terms[t].x_mask, terms[t].z_mask}); }
  void refuse(int64_t t, const char* why) const {
    char hex[64];
    std::snprintf(hex, sizeof hex, "(x_mask 0x%llx, z_mask 0x%llx)", (unsigned long long)terms[t].x_mask,
                  (unsigned long long)terms[t].z_mask);
    LL_REQUIRE(false, "term " + std::to_string(t) + " " + hex + why);
  }
  // a site permutation, given on a mask, must map every term onto an exactly equal coefficient (a missing term counts as 0)
  template <typename Move> void require(Move move, const char* why) const {
    for (int64_t t = 0; t < n_terms; ++t) {
      const auto it = merged.find({move(terms[t].x_mask), move(terms[t].z_mask)});
      if ((it == merged.end() ? 0.0 : it->second) != coef(t)) refuse(t, why);
    }
  }
  void require_translation(int L) const {
    require([&](uint64_t v) { return ring_rot(v, L); },
            " does not commute with the one-site translation of the ring: shifted by one site it meets a different coefficient (an "
            "open chain, or bonds that differ); a momentum sector needs a translation-invariant H");
  }
  // the one-site translation of an Lx x Ly torus along x (dir 0) or y (dir 1)
  void require_torus_translation(const PauliTorus& g, int dir) const {
    require([&](uint64_t v) { return (uint64_t)(dir == 0 ? g.tx((uint32_t)v) : g.ty((uint32_t)v)); },
            dir == 0 ? " does not commute with T_x, the one-site translation of the torus along x (site (x, y) -> (x + 1 mod Lx, y)): "
                       "shifted by one site along x it meets a different coefficient (open boundaries along x, bonds that differ, "
                       "or a ring's Hamiltonian given as a torus); a translation block needs an H invariant under T_x and T_y"
                     : " does not commute with T_y, the one-site translation of the torus along y (site (x, y) -> (x, y + 1 mod Ly)): "
                       "shifted by one site along y it meets a different coefficient (an open cylinder, or bonds that differ); a "
                       "translation block needs an H invariant under T_x and T_y");
  }
  void require_reflection(int L) const {
    require([&](uint64_t v) { return ring_rev(v, L); },
            " does not commute with the reflection of the ring (site j -> n_sites - 1 - j): reflected it meets a different "
            "coefficient (a Dzyaloshinskii-Moriya bond, or bonds that differ); a parity block needs a reflection-invariant H");
  }
  void require_inversion() const {  // prod_j X_j anticommutes with Y and Z: odd popcount(z_mask) needs the merged coefficient 0
    for (int64_t t = 0; t < n_terms; ++t)
      if ((__builtin_popcountll(terms[t].z_mask) & 1) != 0 && coef(t) != 0.0)
        refuse(t, " does not commute with the global spin flip (the product of all X_j): it holds an odd number of Y and Z "
                  "factors (a longitudinal field, for example); a spin-inversion block needs an H that is even under the flip");
  }
};

// The states of the sector of n_down set bits in ascending order and the two tables that give a state's index back
// (ll_internal.hpp PauliSectorImage): one pass over the C(n_sites, n_down) states, on the host.
struct SectorTables {
  int h = 0;
  int64_t dim = 0;
  std::vector<uint32_t> states, lo_rank, hi_rank;
  uint32_t rank(uint32_t s) const { return lo_rank[s & (((uint32_t)1 << h) - 1)] + hi_rank[s >> h]; }
};
SectorTables sector_tables(int32_t n_sites, int32_t n_down) {
  // binom[p][k] = C(p, k), p <= n_sites <= 30: below 2^32
  std::vector<std::vector<uint64_t>> binom((size_t)n_sites + 1, std::vector<uint64_t>((size_t)n_sites + 2, 0));
  for (int p = 0; p <= n_sites; ++p) {
    binom[(size_t)p][0] = 1;
    for (int k = 1; k <= p; ++k) binom[(size_t)p][(size_t)k] = binom[(size_t)p - 1][(size_t)k - 1] + binom[(size_t)p - 1][(size_t)k];
  }
  SectorTables st;
  st.dim = (int64_t)binom[(size_t)n_sites][(size_t)n_down];
  const int h = st.h = (n_sites + 1) / 2, hb = n_sites - h;  // low / other bits: both tables at most 2^15 entries
  // rank(s) = sum_k C(p_k, k) over the set bits p_1 < p_2 < ...: the low bits count k from 1, the others from
  // n_down - popcount(others) + 1 (entries no state of the sector reaches stay 0)
  std::vector<uint32_t>& lo_rank = st.lo_rank;
  std::vector<uint32_t>& hi_rank = st.hi_rank;
  lo_rank.assign((size_t)1 << h, 0);
  hi_rank.assign((size_t)1 << hb, 0);
  for (uint32_t lo = 0; lo < ((uint32_t)1 << h); ++lo) {
    if (__builtin_popcount(lo) > n_down) continue;
    uint64_t r = 0;
    int k = 0;
    for (int p = 0; p < h; ++p)
      if (lo >> p & 1u) r += binom[(size_t)p][(size_t)++k];
    lo_rank[lo] = (uint32_t)r;
  }
  for (uint32_t hi = 0; hi < ((uint32_t)1 << hb); ++hi) {
    int k = n_down - __builtin_popcount(hi);
    if (k < 0 || k > h) continue;
    uint64_t r = 0;
    for (int p = 0; p < hb; ++p)
      if (hi >> p & 1u) r += binom[(size_t)(p + h)][(size_t)++k];
    hi_rank[hi] = (uint32_t)r;
  }
  const int64_t dim = st.dim;
  std::vector<uint32_t>& states = st.states;
  states.resize((size_t)dim);
  {
    uint64_t s = ((uint64_t)1 << n_down) - 1;  // the smallest state; the next one with as many set bits follows (Gosper)
    for (int64_t i = 0; i < dim; ++i) {
      states[(size_t)i] = (uint32_t)s;
      if (s == 0) break;
      const uint64_t c = s & (0 - s), r = s + c;
      s = (((r ^ s) >> 2) >> __builtin_ctzll(s)) | r;
    }
  }
  return st;
}
// the momentum argument of the three momentum-block operators
template <typename T> void pauli_require_momentum(int32_t n_sites, int32_t momentum) {
  LL_REQUIRE(momentum >= 0 && momentum < n_sites, "momentum must lie in [0, n_sites) (the block of k = 2 pi momentum / n_sites)");
  LL_REQUIRE(scalar_traits<T>::is_complex || (2 * momentum) % n_sites == 0,
             "a real storage type takes momentum 0 and n_sites / 2 only (the other blocks are complex Hermitian); use a complex "
             "storage type");
}
// ratio[Ra * 32 + Rb] = sqrt(Ra / Rb) for the orbit lengths of a ring of at most 30 sites: the table of both momentum-block operators
std::vector<double> momentum_ratio_table() {
  std::vector<double> ratio(32 * 32, 0.0);
  for (int a = 1; a < 32; ++a)
    for (int b = 1; b < 32; ++b) ratio[(size_t)a * 32 + (size_t)b] = std::sqrt((double)a / (double)b);
  return ratio;
}
// phase[l] = e^(-2 pi i m l / n_sites) as (re, im), l < n_sites, exact on the axes: the table of the three momentum-block operators
// entry l of a table of n_sites phases: e^(-2 pi i k / n_sites), 0 <= k < n_sites
void unit_phase_entry(int32_t n_sites, int k, int l, std::vector<double>& phase) {
  const double th = 2.0 * M_PI * (double)k / (double)n_sites;
  double c = std::cos(th), sn = -std::sin(th);
  if (4 * k % n_sites == 0) {
    const int quarter = 4 * k / n_sites;  // 0 .. 3
    c = quarter == 0 ? 1.0 : quarter == 2 ? -1.0 : 0.0;
    sn = quarter == 1 ? -1.0 : quarter == 3 ? 1.0 : 0.0;
  }
  phase[2 * (size_t)l] = c;
  phase[2 * (size_t)l + 1] = sn;
}
void momentum_phase_table(int32_t n_sites, int32_t momentum, std::vector<double>& phase) {
  for (int l = 0; l < n_sites; ++l) unit_phase_entry(n_sites, (int)(((int64_t)momentum * l) % n_sites), l, phase);
}
// phase[code] = chi(T_x^a T_y^b) = e^(-2 pi i (m_x a Ly + m_y b Lx) / (Lx Ly)), code = a + Lx b: the table of the torus operator, by
// the arithmetic of the ring's (with Ly = 1 or Lx = 1 the ring's bits)
void torus_phase_table(const PauliTorus& g, int32_t mx, int32_t my, std::vector<double>& phase) {
  for (int c = 0; c < g.sites(); ++c) unit_phase_entry(g.sites(), g.phase_num(mx, my, c), c, phase);
}
// The binary necklaces of n_sites bits in ascending order with their periods, by the Fredricksen-Kessler-Maiorana enumeration: a
// string read from site n_sites - 1 down to site 0 that is the lexicographically smallest of its rotations is the smallest
// integer of its orbit, and the enumeration yields these strings in ascending order with their period (the length of the Lyndon
// word they repeat) — one step per pre-necklace, about two steps per necklace, no pass over the 2^n_sites states.  A step: raise
// the lowest 0 bit (position i from the top), drop what lies below it and repeat the top i bits downwards; the result is a
// necklace iff i divides n_sites, and then its period is i.  visit(a, period) is called for every necklace, the string of zeros
// (period 1) first.
template <typename Visit> void for_each_necklace(int L, Visit visit) {
  const uint32_t site_mask = (uint32_t)(((uint64_t)1 << L) - 1);
  visit((uint32_t)0, 1);
  uint32_t a = 0;
  while (a != site_mask) {
    const int low0 = __builtin_ctz(~a);  // the lowest 0 bit of a (a != all ones): string position i = L - low0 from the top
    const int i = L - low0;
    a = ((a >> low0) | 1u) << low0;      // raise it, clear what lies below
    for (int sft = i; sft < L; sft *= 2) a |= a >> sft;  // repeat the top i bits downwards (bits shifted out fall off the end)
    if (L % i != 0) continue;            // a pre-necklace only
    visit(a, i);
  }
}
// The representatives of one block of a ring — momentum, reflection (parity != 0), spin inversion (inversion != 0), the full
// space (n_down = -1) or the sector n_down — ascending, with their orbit lengths R = |G| / |stabiliser|.  A necklace a is the
// representative of its G-orbit iff no rotation of rev(a), ~a, ~rev(a) (those in use) lies below it, and in the block iff the
// character is 1 on its stabiliser.  Its own rotations fix it L / period times, with character 1 iff momentum * period = 0 (mod L):
// no walk, and with no flag in use nothing else per necklace (two divisions there cost a third of the enumeration).  The other
// streams are walked: O(L) per necklace, no table over the states.  `too_many` refuses the (2^27 - 1)th representative.
struct BlockReps {
  int group_size = 0;  // |G|
  std::vector<uint32_t> reps;
  std::vector<uint8_t> orbit_len;
};
BlockReps block_reps(int L, int n_down, int momentum, int parity, int inversion, const char* too_many) {
  const uint32_t site_mask = (uint32_t)(((uint64_t)1 << L) - 1);
  const bool flags = parity != 0 || inversion != 0;
  BlockReps br;
  br.group_size = L * (parity != 0 ? 2 : 1) * (inversion != 0 ? 2 : 1);
  if (n_down < 0 && !flags) {  // a lower bound of D_m that saves most of the re-allocations: the orbits of full length alone
    br.reps.reserve((size_t)(((uint64_t)1 << L) / (uint64_t)L) + 64);
    br.orbit_len.reserve(br.reps.capacity());
  }
  for_each_necklace(L, [&](uint32_t a, int period) {
    if (n_down >= 0 && __builtin_popcount(a) != n_down) return;  // G keeps the popcount (inversion: 2 n_down = L)
    if (((int64_t)momentum * period) % L != 0) return;           // the string of zeros (period 1) lies in momentum 0 only
    int orbit = period;  // under the shift alone
    if (flags) {
      int stab = L / period;
      bool least = true, admitted = true;
      for (int rho = 0; rho <= (parity != 0 ? 1 : 0); ++rho)
        for (int zeta = rho ? 0 : 1; zeta <= (inversion != 0 ? 1 : 0); ++zeta) {
          uint32_t cur = rho ? (uint32_t)ring_rev(a, L) : a;
          if (zeta) cur ^= site_mask;
          const bool neg = (rho && parity < 0) != (zeta && inversion < 0);
          for (int j = 0; j < L; ++j) {  // cur = T^j P^rho Z^zeta a; its character in units of pi / L: 2 m j, + L for a factor -1
            if (cur < a) least = false;
            if (cur == a) {
              ++stab;
              if ((2 * (int64_t)momentum * j + (neg ? L : 0)) % (2 * L) != 0) admitted = false;
            }
            cur = (uint32_t)ring_rot(cur, L);
          }
        }
      if (!least || !admitted) return;
      orbit = br.group_size / stab;
    }
    LL_REQUIRE(br.reps.size() < (((size_t)1 << 27) - 1), too_many);
    br.reps.push_back(a);
    br.orbit_len.push_back((uint8_t)orbit);
  });
  return br;
}
// The bucket table over the top bits of ascending representatives (PauliRepImage): the largest power of two not above
// dim / 8 buckets (the table stays below dim / 2 bytes), and the halvings that bring the largest bucket down to one candidate.
struct RepBuckets {
  std::vector<uint32_t> start;
  int shift = 0, trips = 0;
  int64_t max_bucket = 0;
};
RepBuckets rep_buckets(int L, const std::vector<uint32_t>& reps) {
  const int64_t dim = (int64_t)reps.size();
  RepBuckets rb;
  int pb = 0;
  while (pb < L && ((int64_t)2 << pb) <= dim / 8) ++pb;
  rb.shift = L - pb;
  rb.start.assign(((size_t)1 << pb) + 1, 0);
  for (int64_t k = 0; k < dim; ++k) ++rb.start[(size_t)(reps[(size_t)k] >> rb.shift) + 1];
  for (size_t q = 1; q < rb.start.size(); ++q) {
    rb.max_bucket = std::max<int64_t>(rb.max_bucket, rb.start[q]);
    rb.start[q] += rb.start[q - 1];
  }
  for (int64_t n = rb.max_bucket; n > 1; n -= n / 2) ++rb.trips;  // n -> n - n / 2
  return rb;
}
// The operator of a searched-basis kind from its representatives: bucket table, the image and its tables on the device, the
// allocations named "<who> ...".  phase: the n_sites phases of the kind's group elements.
template <typename T>
std::unique_ptr<ll_operator> pauli_block_operator(ll_context* ctx, ll_operator::Kind kind, const PauliTables& pt, int n_sites, int n_down,
                                                  int momentum, int parity, int inversion, const BlockReps& br,
                                                  const std::vector<double>& ratio, const std::vector<double>& phase,
                                                  const std::string& who) {
  const RepBuckets rb = rep_buckets(n_sites, br.reps);
  std::unique_ptr<ll_operator> op = pauli_operator<T>(ctx, kind, (int64_t)br.reps.size(), pt, &ll_operator::pauli_block);
  PauliBlockImage& im = op->pauli_block;
  im.n_sites = n_sites;
  im.n_down = n_down;
  im.momentum = momentum;
  im.parity = parity;
  im.inversion = inversion;
  im.group_size = br.group_size;
  im.dim = (int64_t)br.reps.size();
  im.basis.prefix_shift = rb.shift;
  im.basis.search_trips = rb.trips;
  im.basis.max_bucket = rb.max_bucket;
  pauli_upload(ctx, im.basis.reps, br.reps, (who + " representatives").c_str());
  pauli_upload(ctx, im.basis.orbit_len, br.orbit_len, (who + " orbit lengths").c_str());
  pauli_upload(ctx, im.basis.start, rb.start, (who + " bucket table").c_str());
  pauli_upload(ctx, im.ratio, ratio, (who + " norm ratios").c_str());
  pauli_upload(ctx, im.phase, phase, (who + " phases").c_str());
  return op;
}
// the phases of a ring's shifts
std::vector<double> ring_phases(int n_sites, int momentum) {
  std::vector<double> phase(2 * (size_t)n_sites);
  momentum_phase_table(n_sites, momentum, phase);
  return phase;
}
}  // namespace

// n = 2^n_sites: the whole space (pauli.hip)
template <typename T>
void create_pauli(ll_context* ctx, int32_t n_sites, int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  std::unique_ptr<ll_operator> op = pauli_operator<T>(ctx, ll_operator::PAULI, (int64_t)1 << n_sites, pt, &ll_operator::pauli);
  op->pauli.n_sites = n_sites;
  *out = op.release();
}

// The same terms on the sector of n_down set bits (pauli_sector.hip).  The states and the two rank tables are built here, on the
// host: one pass over the C(n_sites, n_down) states in ascending order.
template <typename T>
void create_pauli_sector(ll_context* ctx, int32_t n_sites, int32_t n_down, int64_t n_terms, const ll_pauli_term* terms,
                         ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(n_down >= 0 && n_down <= n_sites, "n_down must lie in [0, n_sites] (the number of flipped spins of the sector)");
  pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
  const SectorTables st = sector_tables(n_sites, n_down);
  std::unique_ptr<ll_operator> op = pauli_operator<T>(ctx, ll_operator::PAULI_SECTOR, st.dim, pt, &ll_operator::pauli_sector);
  PauliSectorImage& im = op->pauli_sector;
  im.n_sites = n_sites;
  im.n_down = n_down;
  im.h = st.h;
  im.dim = st.dim;
  pauli_upload(ctx, im.states, st.states, "S_z sector states");
  pauli_upload(ctx, im.lo_rank, st.lo_rank, "S_z sector rank table (low bits)");
  pauli_upload(ctx, im.hi_rank, st.hi_rank, "S_z sector rank table (high bits)");
  *out = op.release();
}

// One momentum block of that sector (pauli_momentum.hip).  One pass over the sector's states in ascending order, on the host: the
// first state of an orbit not seen before is its representative; walking the orbit gives its period R and, for the blocks's
// orbits (m R = 0 mod n_sites), the entries orbit[rank(T^j r)] = (index of r << 5 | j).
template <typename T>
void create_pauli_momentum(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int64_t n_terms,
                           const ll_pauli_term* terms, ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(n_down >= 0 && n_down <= n_sites, "n_down must lie in [0, n_sites] (the number of flipped spins of the sector)");
  pauli_require_momentum<T>(n_sites, momentum);
  pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
  PauliInvariance(n_terms, terms).require_translation(n_sites);
  const SectorTables st = sector_tables(n_sites, n_down);
  auto rot = [&](uint32_t v) { return (uint32_t)ring_rot(v, n_sites); };
  std::vector<uint32_t> orbit((size_t)st.dim, kPauliOrbitExcluded), reps;
  std::vector<uint8_t> orbit_len;
  std::vector<bool> seen((size_t)st.dim, false);
  bool any_short = false;
  for (int64_t i = 0; i < st.dim; ++i) {
    if (seen[(size_t)i]) continue;
    const uint32_t r = st.states[(size_t)i];  // ascending order: the smallest state of a new orbit
    int R = 0;
    for (uint32_t t = r;;) {
      seen[(size_t)st.rank(t)] = true;
      ++R;
      if ((t = rot(t)) == r) break;
    }
    if (((int64_t)momentum * R) % n_sites != 0) continue;  // the orbit's states keep kPauliOrbitExcluded
    const uint64_t idx = reps.size();
    LL_REQUIRE(idx < ((uint64_t)1 << (32 - kPauliOrbitShiftBits)) - 1, "internal: a momentum block of 2^27 states or more");
    uint32_t t = r;
    for (int j = 0; j < R; ++j, t = rot(t)) orbit[(size_t)st.rank(t)] = (uint32_t)(idx << kPauliOrbitShiftBits) | (uint32_t)j;
    reps.push_back(r);
    orbit_len.push_back((uint8_t)R);
    any_short = any_short || R != n_sites;
  }
  static_assert(kPauliMaxSites < (1 << kPauliOrbitShiftBits), "the shift l of an orbit entry needs n_sites < 2^5");
  const int64_t dim = (int64_t)reps.size();
  LL_REQUIRE(dim >= 1, "the momentum block is empty: no orbit of the sector (n_sites " + std::to_string(n_sites) + ", n_down " +
                           std::to_string(n_down) + ") has a length R with momentum * R = 0 (mod n_sites)");
  const std::vector<double> ratio = momentum_ratio_table();
  std::vector<double> phase(2 * (size_t)n_sites);
  momentum_phase_table(n_sites, momentum, phase);
  std::unique_ptr<ll_operator> op = pauli_operator<T>(ctx, ll_operator::PAULI_MOMENTUM, dim, pt, &ll_operator::pauli_momentum);
  PauliMomentumImage& im = op->pauli_momentum;
  im.n_sites = n_sites;
  im.n_down = n_down;
  im.momentum = momentum;
  im.h = st.h;
  im.dim = dim;
  im.sector_dim = st.dim;
  if (any_short)  // the primes q of n_sites: a state has a short orbit iff rotating it by n_sites / q gives it back for one of them
    for (int q = 2, rest = n_sites; rest > 1; ++q)
      if (rest % q == 0) {
        LL_REQUIRE(im.nshort < 3, "internal: more than three primes in n_sites");
        im.short_shift[im.nshort++] = n_sites / q;
        while (rest % q == 0) rest /= q;
      }
  pauli_upload(ctx, im.reps, reps, "momentum block representatives");
  pauli_upload(ctx, im.orbit_len, orbit_len, "momentum block orbit lengths");
  pauli_upload(ctx, im.orbit, orbit, "momentum block orbit table");
  pauli_upload(ctx, im.lo_rank, st.lo_rank, "S_z sector rank table (low bits)");
  pauli_upload(ctx, im.hi_rank, st.hi_rank, "S_z sector rank table (high bits)");
  pauli_upload(ctx, im.ratio, ratio, "momentum block norm ratios");
  pauli_upload(ctx, im.phase, phase, "momentum block phases");
  *out = op.release();
}

// One momentum block of the full 2^n_sites space (pauli_momentum_full.hip): the block of the shift alone — about two steps of
// the necklace enumeration per representative, no pass over the states.
template <typename T>
void create_pauli_momentum_full(ll_context* ctx, int32_t n_sites, int32_t momentum, int64_t n_terms, const ll_pauli_term* terms,
                                ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  pauli_require_momentum<T>(n_sites, momentum);
  PauliInvariance(n_terms, terms).require_translation(n_sites);
  const BlockReps br = block_reps(n_sites, -1, momentum, 0, 0, "internal: a momentum block of 2^27 states or more");
  // never empty: the state 0..01 has the full period n_sites, which every m admits (n_sites = 1: m = 0, and both states have R = 1)
  LL_REQUIRE(!br.reps.empty(), "internal: an empty momentum block of the full space");
  *out = pauli_block_operator<T>(ctx, ll_operator::PAULI_MOMENTUM_FULL, pt, n_sites, -1, momentum, 0, 0, br, momentum_ratio_table(),
                                 ring_phases(n_sites, momentum), "momentum block")
             .release();
}

// One block under momentum, reflection and spin inversion, of the full space or of one sector (pauli_symmetric.hip)
template <typename T>
void create_pauli_symmetric(ll_context* ctx, int32_t n_sites, int32_t n_down, int32_t momentum, int32_t parity, int32_t inversion,
                            int64_t n_terms, const ll_pauli_term* terms, ll_operator** out) {
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(parity >= -1 && parity <= 1, "parity must be 0 (the reflection is not used), +1 or -1");
  LL_REQUIRE(inversion >= -1 && inversion <= 1, "inversion must be 0 (the global spin flip is not used), +1 or -1");
  LL_REQUIRE(n_down >= -1 && n_down <= n_sites,
             "n_down must lie in [-1, n_sites] (-1: the full space; else the number of flipped spins of the sector)");
  pauli_require_momentum<T>(n_sites, momentum);
  LL_REQUIRE(parity == 0 || (2 * momentum) % n_sites == 0,
             "parity != 0 takes momentum 0 and n_sites / 2 only (the reflection maps momentum k to -k: the group of shifts and "
             "the reflection has one-dimensional characters only there); use parity = 0");
  const PauliInvariance inv(n_terms, terms);
  inv.require_translation(n_sites);
  if (parity != 0) inv.require_reflection(n_sites);
  if (inversion != 0) inv.require_inversion();
  if (n_down >= 0) {
    pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
    LL_REQUIRE(inversion == 0 || 2 * n_down == n_sites,
               "inversion != 0 with n_down >= 0 needs 2 n_down = n_sites (the global spin flip maps the sector n_down onto "
               "n_sites - n_down)");
  }
  const BlockReps br = block_reps(n_sites, n_down, momentum, parity, inversion,
                                  "a block of 2^27 - 1 states or more (32-bit indices with room for the search)");
  LL_REQUIRE(!br.reps.empty(), "the block (momentum " + std::to_string(momentum) + ", parity " + std::to_string(parity) +
                                   ", inversion " + std::to_string(inversion) + ", n_down " + std::to_string(n_down) +
                                   ") is empty: no orbit carries this character");
  // ratio[R_a][c] = sqrt(R_a / R_b) for the orbit length R_b = |G| / c of a stabiliser of c elements
  const int G = br.group_size;
  std::vector<double> ratio((size_t)kPauliSymmetricRatioStride * kPauliSymmetricRatioStride, 0.0);
  for (int a = 1; a <= G; ++a)
    for (int c = 1; c <= G; ++c)
      if (G % c == 0) ratio[(size_t)a * kPauliSymmetricRatioStride + (size_t)c] = std::sqrt((double)a / (double)(G / c));
  *out = pauli_block_operator<T>(ctx, ll_operator::PAULI_SYMMETRIC, pt, n_sites, n_down, momentum, parity, inversion, br, ratio,
                                 ring_phases(n_sites, momentum), "symmetry block")
             .release();
}

// One translation block of an Lx x Ly torus, of the full space or of one sector (pauli_torus.hip).  The representatives are
// enumerated on the host in slices of equal top bits (pauli_torus_plan.hpp), at most 16 threads, each state left at its first
// smaller image.
template <typename T>
void create_pauli_torus(ll_context* ctx, int32_t lx, int32_t ly, int32_t n_down, int32_t mx, int32_t my, int64_t n_terms,
                        const ll_pauli_term* terms, ll_operator** out) {
  LL_REQUIRE(lx >= 1 && ly >= 1, "lx and ly must be at least 1 (the extents of the torus)");
  LL_REQUIRE((int64_t)lx * ly <= kPauliMaxSites, "lx * ly must be at most " + std::to_string(kPauliMaxSites) +
                                                     " (the sites of the torus: 2^(lx ly) states, 32-bit local indices)");
  const int n_sites = lx * ly;
  const PauliTables pt = pauli_tables<T>(ctx, n_sites, n_terms, terms, out);
  LL_REQUIRE(n_down >= -1 && n_down <= n_sites,
             "n_down must lie in [-1, lx * ly] (-1: the full space; else the number of flipped spins of the sector)");
  LL_REQUIRE(mx >= 0 && mx < lx, "mx must lie in [0, lx) (the block of k_x = 2 pi mx / lx)");
  LL_REQUIRE(my >= 0 && my < ly, "my must lie in [0, ly) (the block of k_y = 2 pi my / ly)");
  LL_REQUIRE(scalar_traits<T>::is_complex || ((2 * mx) % lx == 0 && (2 * my) % ly == 0),
             "a real storage type takes mx = 0 or lx / 2 and my = 0 or ly / 2 only (the other blocks are complex Hermitian); use a "
             "complex storage type");
  const PauliTorus g(lx, ly);
  const PauliInvariance inv(n_terms, terms);
  inv.require_torus_translation(g, 0);
  inv.require_torus_translation(g, 1);
  if (n_down >= 0) pauli_require_sz_conserving(pt, scalar_traits<T>::is_complex ? 2 : 1);
  // slices of equal top bits, handed out in ascending order and joined in that order
  const int top_bits = std::min(n_sites, 10), low_bits = n_sites - top_bits;
  const uint32_t nslices = (uint32_t)1 << top_bits;
  std::vector<std::vector<uint32_t>> slice_reps(nslices);
  std::vector<std::vector<uint8_t>> slice_len(nslices);
  std::atomic<uint32_t> next{0};
  auto work = [&]() {
    for (uint32_t q; (q = next.fetch_add(1)) < nslices;) pauli_torus_slice(g, n_down, mx, my, q, low_bits, slice_reps[q], slice_len[q]);
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const int nthreads = n_sites < 20 ? 1 : (int)std::min<unsigned>(16u, std::max<unsigned>(1u, hw));
  {
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (std::thread& th : pool) th.join();
  }
  BlockReps br;
  br.group_size = n_sites;
  size_t total = 0;
  for (uint32_t q = 0; q < nslices; ++q) total += slice_reps[q].size();
  LL_REQUIRE(total < (((size_t)1 << 27) - 1), "a block of 2^27 - 1 states or more (32-bit indices with room for the search)");
  LL_REQUIRE(total != 0, "the block (mx " + std::to_string(mx) + ", my " + std::to_string(my) + ", n_down " + std::to_string(n_down) +
                             ") of the " + std::to_string(lx) + " x " + std::to_string(ly) +
                             " torus is empty: no orbit carries this character");
  br.reps.reserve(total);
  br.orbit_len.reserve(total);
  for (uint32_t q = 0; q < nslices; ++q) {
    br.reps.insert(br.reps.end(), slice_reps[q].begin(), slice_reps[q].end());
    br.orbit_len.insert(br.orbit_len.end(), slice_len[q].begin(), slice_len[q].end());
    std::vector<uint32_t>().swap(slice_reps[q]);
    std::vector<uint8_t>().swap(slice_len[q]);
  }
  // ratio[R_a][c] = sqrt(R_a / R_b) for the orbit length R_b = |G| / c of a stabiliser of c elements
  std::vector<double> ratio((size_t)kPauliTorusRatioStride * kPauliTorusRatioStride, 0.0);
  for (int a = 1; a <= n_sites; ++a)
    for (int c = 1; c <= n_sites; ++c)
      if (n_sites % c == 0) ratio[(size_t)a * kPauliTorusRatioStride + (size_t)c] = std::sqrt((double)a / (double)(n_sites / c));
  std::vector<double> phase(2 * (size_t)n_sites);
  torus_phase_table(g, mx, my, phase);
  std::unique_ptr<ll_operator> op =
      pauli_block_operator<T>(ctx, ll_operator::PAULI_TORUS, pt, n_sites, n_down, mx, 0, 0, br, ratio, phase, "torus block");
  op->pauli_block.lx = lx;
  op->pauli_block.ly = ly;
  op->pauli_block.momentum_y = my;
  *out = op.release();
}

template <typename T>
int launch_pauli_op(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s, const ScaleIn<T>* sc) {
  switch (op.kind) {
    case ll_operator::PAULI: return launch_pauli<T>(op, x, y, offset, dot_partials, s, sc);
    case ll_operator::PAULI_SECTOR: return launch_pauli_sector<T>(op, x, y, offset, dot_partials, s, sc);
    case ll_operator::PAULI_MOMENTUM: return launch_pauli_momentum<T>(op, x, y, offset, dot_partials, s, sc);
    case ll_operator::PAULI_MOMENTUM_FULL: return launch_pauli_momentum_full<T>(op, x, y, offset, dot_partials, s, sc);
    case ll_operator::PAULI_SYMMETRIC: return launch_pauli_symmetric<T>(op, x, y, offset, dot_partials, s, sc);
    case ll_operator::PAULI_TORUS: return launch_pauli_torus<T>(op, x, y, offset, dot_partials, s, sc);
    default: LL_REQUIRE(false, "internal: not a Pauli-sum operator"); return 0;
  }
}

#define LL_INST_PAULI_OPERATORS(T)                                                                                               \
  template void create_pauli<T>(ll_context*, int32_t, int64_t, const ll_pauli_term*, ll_operator**);                             \
  template void create_pauli_sector<T>(ll_context*, int32_t, int32_t, int64_t, const ll_pauli_term*, ll_operator**);             \
  template void create_pauli_momentum<T>(ll_context*, int32_t, int32_t, int32_t, int64_t, const ll_pauli_term*, ll_operator**);  \
  template void create_pauli_momentum_full<T>(ll_context*, int32_t, int32_t, int64_t, const ll_pauli_term*, ll_operator**);    \
  template void create_pauli_symmetric<T>(ll_context*, int32_t, int32_t, int32_t, int32_t, int32_t, int64_t, const ll_pauli_term*, \
                                          ll_operator**);                                                                      \
  template void create_pauli_torus<T>(ll_context*, int32_t, int32_t, int32_t, int32_t, int32_t, int64_t, const ll_pauli_term*,   \
                                      ll_operator**);                                                                          \
  template int launch_pauli_op<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const ScaleIn<T>*);
LL_FOR_EACH_SCALAR(LL_INST_PAULI_OPERATORS)

}  // namespace ll
