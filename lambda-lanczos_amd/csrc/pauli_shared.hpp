// What the sum-of-Pauli-strings kernels share (pauli.hip: all 2^n_sites states; pauli_basis.hpp and its four policies: an
// indexed basis): the weight of a group of terms as the accumulator's type, the double fma per group, the element-wise /
// 16-byte accesses, the two factors of a momentum block's entry, the sign flip, the rotation within the ring and the search
// of a representative's number.  One definition, so that the kernels form the same sum for a state: same values, same order,
// same bits.
#pragma once
#include "dev_helpers.hpp"
#include "ll_internal.hpp"

namespace ll {

// The full-space kernels (pauli.hip, pauli_expect.hip) stage tiles of 2^b states of T in LDS: the context's pauli_tile_bits, else
// what fills kPauliTileBytes; at most kPauliMaxTileBytes (the LDS a launch may ask for without raising the kernel's limit) and
// never more than the vector
template <typename T> int pauli_tile_bits(const ll_operator& op) {
  int b = op.ctx ? op.ctx->tune.pauli_tile_bits : -1;
  if (b < 0)
    for (b = 0; ((size_t)sizeof(T) << (b + 1)) <= (size_t)kPauliTileBytes;) ++b;
  while (b > 0 && ((size_t)sizeof(T) << b) > (size_t)kPauliMaxTileBytes) --b;
  return std::min(b, op.pauli.n_sites);
}

namespace {
constexpr int kPauliLaneStates = 4;  // states a lane carries through the term loop at a time (accumulators in registers)

// v with its sign flipped where flip = 1
__device__ __forceinline__ double pauli_flip_sign(double v, unsigned flip) {
  return __hiloint2double(__double2hiint(v) ^ (int)(flip << 31), __double2loint(v));
}
__device__ __forceinline__ zc pauli_flip_sign(zc v, unsigned flip) { return zc{pauli_flip_sign(v.re, flip), pauli_flip_sign(v.im, flip)}; }
// coefficient of a term as the accumulator's weight type: one double (real types), (re, im) of c i^nY (complex types)
template <typename A> struct PauliWeight;
template <> struct PauliWeight<double> {
  static __device__ __forceinline__ double load(const double* __restrict__ tc, int t, unsigned flip) {
    return pauli_flip_sign(tc[t], flip);
  }
  static __device__ __forceinline__ void add(double& w, double c, unsigned par) {
    w += pauli_flip_sign(c, par);
  }
};
template <> struct PauliWeight<zc> {
  static __device__ __forceinline__ zc load(const double* __restrict__ tc, int t, unsigned flip) {
    return zc{PauliWeight<double>::load(tc, 2 * t, flip), PauliWeight<double>::load(tc, 2 * t + 1, flip)};
  }
  static __device__ __forceinline__ void add(zc& w, zc c, unsigned par) {
    PauliWeight<double>::add(w.re, c.re, par);
    PauliWeight<double>::add(w.im, c.im, par);
  }
};
__device__ __forceinline__ void pauli_fma(double& acc, double w, double x) { acc = fma(w, x, acc); }
__device__ __forceinline__ void pauli_fma(double& acc, double w, float x) { acc = fma(w, (double)x, acc); }
__device__ __forceinline__ void pauli_fma(zc& acc, zc w, zc x) { fma_acc(acc, w, x); }
__device__ __forceinline__ void pauli_fma(zc& acc, zc w, cf x) { fma_acc(acc, w, to_acc(x)); }
// momentum blocks: w * f * (c + i s); a real weight takes real factors only (creation admits m = 0 and n_sites / 2 for the real
// types: s = 0)
__device__ __forceinline__ double momentum_scale(double w, double f) { return w * f; }
__device__ __forceinline__ zc momentum_scale(zc w, double f) { return zc{w.re * f, w.im * f}; }
__device__ __forceinline__ double momentum_phase(double w, double c, double) { return w * c; }
__device__ __forceinline__ zc momentum_phase(zc w, double c, double s) { return zc{w.re * c - w.im * s, w.re * s + w.im * c}; }
// v, a state of L sites (smask = 2^L - 1), rotated left by r sites, 0 < r < L (L = 1: r = 1, and v comes back)
__device__ __forceinline__ unsigned pauli_rotl(unsigned v, unsigned r, unsigned L, unsigned smask) {
  return ((v << r) | (v >> (L - r))) & smask;
}
// The number of the representative rep in the ascending reps[0 .. dim): start[rep >> prefix_shift] and the entry after it bound
// its bucket, then search_trips branch-free halvings (the count the LARGEST bucket needs, the same for every lane; a lane whose
// bucket is down to one candidate loads nothing more).  Where reps[] does not hold rep, the entry below it in the bucket or the
// bucket's first, never past dim - 1.
__device__ __forceinline__ unsigned pauli_bucket_search(const uint32_t* __restrict__ reps, const uint32_t* __restrict__ start,
                                                        int prefix_shift, int search_trips, unsigned rep, unsigned dim) {
  const unsigned q = rep >> prefix_shift;  // rep < 2^n_sites: q < 2^(n_sites - prefix_shift), start[] holds one more
  unsigned lo = start[q], n = start[q + 1u] - lo;
  for (int t = 0; t < search_trips; ++t) {
    const unsigned half = n >> 1;
    if (half != 0u && reps[lo + half] <= rep) lo += half;
    n -= half;
  }
  return min(lo, dim - 1u);
}

template <typename T, int V> __device__ __forceinline__ void pauli_load(const T* __restrict__ p, T (&r)[V]) {
  if constexpr (V == 1) r[0] = p[0];
  else load_chunk<T, V>(p, r);
}
template <typename T, int V> __device__ __forceinline__ void pauli_store(T* __restrict__ p, const T (&r)[V]) {
  if constexpr (V == 1) p[0] = r[0];
  else store_chunk<T, V>(p, r);
}
// r[v] <- r[v ^ m] for a wave-uniform m < V, one butterfly per bit of m (a register array indexed at run time would go to
// scratch memory)
template <typename T, int V> __device__ __forceinline__ void pauli_xor_permute(T (&r)[V], unsigned m) {
#pragma unroll
  for (int bit = 1; bit < V; bit <<= 1) {
    if (m & bit) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (!(v & bit)) {
          const T a = r[v];
          r[v] = r[v | bit];
          r[v | bit] = a;
        }
      }
    }
  }
}
}  // namespace

}  // namespace ll
