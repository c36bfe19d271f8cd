// Host-side planning of ll_pauli_expect (kernels: pauli_expect.hip): which observables need a sweep at all, in which order the
// kernels meet them and where every answer goes.  Plain integers in, plain vectors out — standard headers only, so the
// arithmetic builds with a host compiler and is checked on the CPU, property by property, in
// tests/cpp/pauli_expect_plan_test.cpp.
//
// An observable (x, z, coef) is the string P with X on the bits of x alone, Z on the bits of z alone, Y on both, and
//   <psi| coef P |psi> = coef * sum_s Re[ conj(psi(s ^ x)) i^nY (-1)^popcount(s & z) psi(s) ],   nY = popcount(x & z).
// With v(s) = conj(psi(s ^ x)) psi(s), formed once per x mask and state, Re[i^nY v] is Re v, -Im v, -Re v, Im v for
// nY mod 4 = 0, 1, 2, 3: a slot carries the part it sums and the plan folds the sign into the coefficient, so that a kernel
// adds +-(one double) per slot and state and the host multiplies the folded sum once.
//
// Identically zero, answered +0.0 without a sweep:
//   real storage, nY odd     v is real: Re[i^nY v] has no real part (the string is imaginary and antisymmetric)
//   one S_z sector, popcount(x) odd   s ^ x never has as many set bits as s
// The other observables are sorted by x mask (ascending; equal masks keep the caller's order: one group, one partner load) and
// the sorted list is cut into batches of at most `batch` slots, so a group may continue in the next batch.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ll {

constexpr uint32_t kExpectSlotNewGroup = 1u;  // the slot's x mask differs from the slot before it in the batch: load the partner
constexpr uint32_t kExpectSlotImag = 2u;      // the slot sums Im v (complex storage, nY odd), else Re v

// The slots of a measuring call cut into batches of at most `batch`, one sweep each: what both plans (this one and
// pauli_expect_block_plan.hpp) derive from; the planning function counts the slots when it has made them.
struct PauliBatches {
  int64_t slot_count = 0;
  int batch = 0;                       // B: slots per sweep at most
  int64_t nslots() const { return slot_count; }
  int64_t nbatches() const { return batch > 0 ? (slot_count + batch - 1) / batch : 0; }
  int64_t batch_begin(int64_t k) const { return k * batch; }
  int64_t batch_count(int64_t k) const { return std::min<int64_t>(batch, slot_count - k * batch); }
};

struct PauliExpectPlan : PauliBatches {
  int64_t n_obs = 0;
  // per slot, in kernel order
  std::vector<uint32_t> x, z, flags;
  std::vector<double> coef;            // coef * (sign of i^nY on the part the slot sums)
  std::vector<int64_t> obs;            // the caller's index of the slot's observable
  // per observable of the caller
  std::vector<int64_t> slot;           // its slot, -1: identically zero
};

inline bool pauli_expect_is_zero(uint64_t x_mask, uint64_t z_mask, bool complex_storage, bool sector) {
  if (!complex_storage && (__builtin_popcountll(x_mask & z_mask) & 1) != 0) return true;
  if (sector && (__builtin_popcountll(x_mask) & 1) != 0) return true;
  return false;
}
// the slot's part of v and the sign that i^nY gives it
inline void pauli_expect_phase(uint64_t x_mask, uint64_t z_mask, bool* imag, double* sign) {
  const int ny = __builtin_popcountll(x_mask & z_mask) & 3;
  *imag = (ny & 1) != 0;
  *sign = (ny == 1 || ny == 2) ? -1.0 : 1.0;
}

// Term: x_mask, z_mask (at most 32 bits set positions: below n_sites <= 30), coef.  The masks and coefficients are the
// caller's to validate.
template <typename Term>
PauliExpectPlan pauli_expect_plan(bool complex_storage, bool sector, int64_t n_obs, const Term* terms, int batch) {
  PauliExpectPlan p;
  p.batch = batch;
  p.n_obs = n_obs;
  p.slot.assign((size_t)n_obs, -1);
  std::vector<int64_t> order;
  order.reserve((size_t)n_obs);
  for (int64_t j = 0; j < n_obs; ++j)
    if (!pauli_expect_is_zero(terms[j].x_mask, terms[j].z_mask, complex_storage, sector)) order.push_back(j);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return terms[a].x_mask < terms[b].x_mask; });
  const size_t ns = order.size();
  p.slot_count = (int64_t)ns;
  p.x.resize(ns);
  p.z.resize(ns);
  p.flags.resize(ns);
  p.coef.resize(ns);
  p.obs.resize(ns);
  for (size_t k = 0; k < ns; ++k) {
    const int64_t j = order[k];
    const Term& t = terms[j];
    bool imag = false;
    double sign = 1.0;
    pauli_expect_phase(t.x_mask, t.z_mask, &imag, &sign);
    p.x[k] = (uint32_t)t.x_mask;
    p.z[k] = (uint32_t)t.z_mask;
    const bool first = k % (size_t)batch == 0 || p.x[k] != p.x[k - 1];
    p.flags[k] = (first ? kExpectSlotNewGroup : 0u) | (imag ? kExpectSlotImag : 0u);
    p.coef[k] = sign * t.coef;
    p.obs[k] = j;
    p.slot[(size_t)j] = (int64_t)k;
  }
  return p;
}

// the x masks of batch k that touch a bit at or above `bits` (a full-space tile of 2^bits states: the partner tile of such a
// group is read from memory) — G_remote of the byte model
inline int pauli_expect_remote_groups(const PauliExpectPlan& p, int64_t k, int bits) {
  int g = 0;
  for (int64_t i = p.batch_begin(k), e = i + p.batch_count(k); i < e; ++i)
    if ((p.flags[(size_t)i] & kExpectSlotNewGroup) != 0 && (p.x[(size_t)i] >> bits) != 0) ++g;
  return g;
}

}  // namespace ll
