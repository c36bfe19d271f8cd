// What the sum-of-Pauli-strings kernels share (pauli.hip: all 2^n_sites states; pauli_sector.hip: one S_z sector;
// pauli_momentum.hip, pauli_momentum_full.hip: one momentum block of a sector / of the full space): the weight of a group of
// terms as the accumulator's type, the double fma per group, the element-wise / 16-byte accesses and the two factors of a
// momentum block's entry.  One definition, so that the kernels form the same sum for a state: same values, same order, same bits.
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
// momentum blocks: w * f * (c + i s); a real weight takes real factors only (creation admits m = 0 and n_sites / 2 for the real
// types: s = 0)
__device__ __forceinline__ double momentum_scale(double w, double f) { return w * f; }
__device__ __forceinline__ zc momentum_scale(zc w, double f) { return zc{w.re * f, w.im * f}; }
__device__ __forceinline__ double momentum_phase(double w, double c, double) { return w * c; }
__device__ __forceinline__ zc momentum_phase(zc w, double c, double s) { return zc{w.re * c - w.im * s, w.re * s + w.im * c}; }

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
