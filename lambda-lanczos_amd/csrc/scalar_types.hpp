// The four storage types, their traits and their conversion to and from std::complex<double>.  Standard headers only: the host
// algebra of raw_basis.hpp and its CPU test build with a plain host compiler.
#pragma once

#include <complex>

namespace ll {

// Device-side complex<double>: interleaved (re, im), 16-byte aligned so that one element is one dwordx4 access.
struct alignas(16) zc {
  double re, im;
};

// Device-side complex<float>: interleaved (re, im), 8-byte aligned.
struct alignas(8) cf {
  float re, im;
};

// `reals` = doubles per REDUCED value (all reductions, coefficients and norms are carried in double / zc whatever the
// storage type: float inputs are widened at the first accumulation, which is at least the reference's accuracy);
// `acc` = that accumulator type.
template <typename T> struct scalar_traits;
template <> struct scalar_traits<double> {
  static constexpr bool is_complex = false;
  static constexpr int reals = 1;
  typedef double acc;
  typedef double real;
};
template <> struct scalar_traits<zc> {
  static constexpr bool is_complex = true;
  static constexpr int reals = 2;
  typedef zc acc;
  typedef double real;
};
template <> struct scalar_traits<float> {
  static constexpr bool is_complex = false;
  static constexpr int reals = 1;
  typedef double acc;
  typedef float real;
};
template <> struct scalar_traits<cf> {
  static constexpr bool is_complex = true;
  static constexpr int reals = 2;
  typedef zc acc;
  typedef float real;
};
template <typename T> using acc_t = typename scalar_traits<T>::acc;
// Explicit instantiation for the four storage types: every translation unit lists the templates it defines ONCE, in a macro
// M(T) per file section, and instantiates them with LL_FOR_EACH_SCALAR(M).
#define LL_FOR_EACH_SCALAR(M) M(double) M(zc) M(float) M(cf)

// Host coefficients are computed in std::complex<double> and stored in T: a real T keeps the real part.
inline std::complex<double> to_z(const double& v) { return {v, 0.0}; }
inline std::complex<double> to_z(const float& v) { return {(double)v, 0.0}; }
inline std::complex<double> to_z(const zc& v) { return {v.re, v.im}; }
inline std::complex<double> to_z(const cf& v) { return {(double)v.re, (double)v.im}; }
inline void from_z(std::complex<double> v, double* o) { *o = v.real(); }
inline void from_z(std::complex<double> v, float* o) { *o = (float)v.real(); }
inline void from_z(std::complex<double> v, zc* o) { *o = zc{v.real(), v.imag()}; }
inline void from_z(std::complex<double> v, cf* o) { *o = cf{(float)v.real(), (float)v.imag()}; }
}  // namespace ll
