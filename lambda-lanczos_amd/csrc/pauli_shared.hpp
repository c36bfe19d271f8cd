// What the two sum-of-Pauli-strings kernels share (pauli.hip: all 2^n_sites states; pauli_sector.hip: one S_z sector): the
// weight of a group of terms as the accumulator's type, the double fma per group and the element-wise / 16-byte accesses.
// One definition, so that both kernels form the same sum for a state: same values, same order, same bits.
#pragma once
#include "dev_helpers.hpp"
#include "ll_internal.hpp"

namespace ll {

namespace {
constexpr int kPauliLaneStates = 4;  // states a lane carries through the term loop at a time (accumulators in registers)

// coefficient of a term as the accumulator's weight type: one double (real types), (re, im) of c i^nY (complex types)
template <typename A> struct PauliWeight;
template <> struct PauliWeight<double> {
  static __device__ __forceinline__ double load(const double* __restrict__ tc, int t, unsigned flip) {
    return __hiloint2double(__double2hiint(tc[t]) ^ (int)(flip << 31), __double2loint(tc[t]));
  }
  static __device__ __forceinline__ void add(double& w, double c, unsigned par) {
    w += __hiloint2double(__double2hiint(c) ^ (int)(par << 31), __double2loint(c));
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

template <typename T, int V> __device__ __forceinline__ void pauli_load(const T* __restrict__ p, T (&r)[V]) {
  if constexpr (V == 1) r[0] = p[0];
  else load_chunk<T, V>(p, r);
}
template <typename T, int V> __device__ __forceinline__ void pauli_store(T* __restrict__ p, const T (&r)[V]) {
  if constexpr (V == 1) p[0] = r[0];
  else store_chunk<T, V>(p, r);
}
}  // namespace

}  // namespace ll
