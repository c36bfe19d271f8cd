// Host-side planning of ll_pauli_block_transfer (kernel: pauli_block_transfer.hip): out = B_t^H (sum_j coef_j P_j) B_s c, a sum of
// Pauli strings applied to a state of one momentum block of a ring (momentum m_s) with the result taken on another (m_t).  Plain
// integers in, plain vectors out — standard headers only, so the arithmetic builds with a host compiler and is checked on the
// CPU, property by property, in tests/cpp/pauli_block_transfer_plan_test.cpp.
//
// B_s c has momentum m_s and B_t^H keeps momentum m_t, so only the part of P that carries q = m_t - m_s (mod L) survives:
//   B_t^H P B_s = B_t^H Pbar_q B_s,   Pbar_q = (1 / L) sum_{j < L} e^(+2 pi i q j / L) [(x, z) both rotated RIGHT by j sites]
// and Pbar_q maps block m_s wholly into block m_t, so the gather of the block kernels applies it (target lanes, source partners).
// A string whose masks have the rotation period r (the smallest r > 0 that gives both masks back; r divides L) meets each of its
// r distinct images L / r times with the phases e^(2 pi i q (j + k r) / L): they add to (L / r) e^(2 pi i q j / L) iff
// q r = 0 (mod L) and to 0 otherwise.  That is the ONE drop rule, decided in integers; a surviving image j < r enters with
//   coef e^(+2 pi i q j / L) / r,
// the phase exact where it lies on an axis.  Equal (x, z) of different caller terms are merged in the caller's order, then i^nY
// is folded in as the operators' term tables fold it.  Strings sorted by x mask, then z mask, grouped by x mask: gx / gptr / tz /
// tc like a Hamiltonian's; tc holds one double per string for the real storage types (2 q = 0 mod L and nY even, the caller's to
// check: every weight is +-real) and (re, im) for the complex ones.
//
// In an S_z sector a string with odd popcount(x) has no partner in the sector: it is left out (pauli_expect_is_zero's rule).
#pragma once

#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace ll {

// v, a mask of L <= 32 sites, rotated right by j sites (0 <= j < L)
inline uint32_t pauli_transfer_rotr(uint32_t v, int j, int L) {
  const uint64_t m = ((uint64_t)1 << L) - 1, w = v;
  return j == 0 ? v : (uint32_t)(((w >> j) | (w << (L - j))) & m);
}
// the smallest r > 0 with both masks rotated by r sites equal to themselves: a divisor of L
inline int pauli_transfer_period(uint32_t x, uint32_t z, int L) {
  for (int r = 1; r < L; ++r)
    if (L % r == 0 && pauli_transfer_rotr(x, r, L) == x && pauli_transfer_rotr(z, r, L) == z) return r;
  return L;
}
// does a string of rotation period r carry momentum q?
inline bool pauli_transfer_carries(int q, int r, int L) { return ((int64_t)q * r) % L == 0; }
// e^(+2 pi i k / L) as (re, im), 0 <= k < L, exact on the axes
inline std::pair<double, double> pauli_transfer_phase(int k, int L) {
  if ((4 * k) % L == 0) {
    const int quarter = 4 * k / L;  // 0 .. 3
    return {quarter == 0 ? 1.0 : quarter == 2 ? -1.0 : 0.0, quarter == 1 ? 1.0 : quarter == 3 ? -1.0 : 0.0};
  }
  const double th = 2.0 * M_PI * (double)k / (double)L;
  return {std::cos(th), std::sin(th)};
}

struct PauliTransferString {
  uint32_t x = 0, z = 0;
  double re = 0.0, im = 0.0;  // the merged weight, i^nY not yet folded in
};
// the strings of Pbar_q of a list of terms, merged, ascending by (x, z)
template <typename Term>
std::vector<PauliTransferString> pauli_block_transfer_strings(int L, int q, bool sector, int64_t n_terms, const Term* terms) {
  std::map<std::pair<uint32_t, uint32_t>, std::pair<double, double>> merged;
  for (int64_t t = 0; t < n_terms; ++t) {
    const uint32_t x = (uint32_t)terms[t].x_mask, z = (uint32_t)terms[t].z_mask;
    if (sector && (__builtin_popcount(x) & 1) != 0) continue;
    const int r = pauli_transfer_period(x, z, L);
    if (!pauli_transfer_carries(q, r, L)) continue;
    for (int j = 0; j < r; ++j) {
      const std::pair<double, double> ph = pauli_transfer_phase((int)(((int64_t)q * j) % L), L);
      const double w = terms[t].coef / (double)r;
      std::pair<double, double>& acc = merged[{pauli_transfer_rotr(x, j, L), pauli_transfer_rotr(z, j, L)}];
      acc.first += w * ph.first;
      acc.second += w * ph.second;
    }
  }
  std::vector<PauliTransferString> out;
  out.reserve(merged.size());
  for (const auto& kv : merged) out.push_back({kv.first.first, kv.first.second, kv.second.first, kv.second.second});
  return out;
}

struct PauliBlockTransferPlan {
  std::vector<uint32_t> gx, tz;  // x mask per group, z mask per string
  std::vector<int32_t> gptr;     // [groups + 1] first string of each group
  std::vector<double> tc;        // per string: weight * i^nY — one double (real types), (re, im) (complex types)
  int64_t ngroups() const { return (int64_t)gx.size(); }
  int64_t nstrings() const { return (int64_t)tz.size(); }
};

// Term: x_mask, z_mask (bits below n_sites <= 30), coef.  q = (m_t - m_s) mod n_sites.  The masks, the coefficients and, for a
// real storage type, 2 q = 0 (mod n_sites) and an even nY are the caller's to validate.
template <typename Term>
PauliBlockTransferPlan pauli_block_transfer_plan(int n_sites, int q, bool complex_storage, bool sector, int64_t n_terms,
                                                 const Term* terms) {
  PauliBlockTransferPlan p;
  for (const PauliTransferString& s : pauli_block_transfer_strings(n_sites, q, sector, n_terms, terms)) {
    if (p.gx.empty() || p.gx.back() != s.x) {
      p.gx.push_back(s.x);
      p.gptr.push_back((int32_t)p.tz.size());
    }
    p.tz.push_back(s.z);
    const int ny = __builtin_popcount(s.x & s.z) & 3;  // times i^nY: 1, i, -1, -i
    double re = s.re, im = s.im;
    if (ny == 1) {
      re = -s.im;
      im = s.re;
    } else if (ny == 2) {
      re = -s.re;
      im = -s.im;
    } else if (ny == 3) {
      re = s.im;
      im = -s.re;
    }
    p.tc.push_back(re + 0.0);  // (never -0.0 from a negated zero part)
    if (complex_storage) p.tc.push_back(im + 0.0);
  }
  p.gptr.push_back((int32_t)p.tz.size());
  return p;
}

// Which pairs of blocks ll_pauli_block_transfer admits.  kind: what the operator is.
enum PauliTransferKind : int {
  kPauliTransferMomentum = 0,      // a momentum block of an S_z sector
  kPauliTransferMomentumFull = 1,  // a momentum block of the full space
  kPauliTransferSymmetric = 2,     // a momentum / reflection / spin-inversion block
  kPauliTransferOther = 3          // anything else
};
struct PauliTransferSide {
  int kind = kPauliTransferOther;
  int n_sites = 0, n_down = -1, momentum = 0;
  int elem_bytes = 0;
  bool is_complex = false;
};
// nullptr: admitted; else why not
inline const char* pauli_block_transfer_fault(const PauliTransferSide& s, const PauliTransferSide& t) {
  if (s.kind == kPauliTransferSymmetric || t.kind == kPauliTransferSymmetric)
    return "a momentum / reflection / spin-inversion block is not admitted: an operator that carries momentum q != 0 does not "
           "commute with the reflection, which needs semi-momentum states (not built); use momentum or full-momentum blocks";
  if (s.kind == kPauliTransferOther || t.kind == kPauliTransferOther)
    return "both operators must be momentum blocks of a sum of Pauli strings (of one S_z sector, or of the full space)";
  if (s.kind != t.kind) return "the two blocks are of different kinds: one of an S_z sector, one of the full space";
  if (s.n_sites != t.n_sites) return "the two blocks differ in n_sites";
  if (s.kind == kPauliTransferMomentum && s.n_down != t.n_down)
    return "the two blocks differ in n_down (a transfer that changes the magnetisation is not built)";
  if (s.elem_bytes != t.elem_bytes || s.is_complex != t.is_complex) return "the two blocks differ in their storage type";
  return nullptr;
}
inline int pauli_block_transfer_q(const PauliTransferSide& s, const PauliTransferSide& t) {
  return ((t.momentum - s.momentum) % s.n_sites + s.n_sites) % s.n_sites;
}

}  // namespace ll
