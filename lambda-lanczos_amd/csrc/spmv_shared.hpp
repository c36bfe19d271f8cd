// Device pieces shared by the row-block SpMV kernels (spmv_pb.hip: PB phase 2; spmv_tiled.hip; spmv_sym.hip: one-triangle kernel)
// and the kernels that build their images (spmv_image_build.hip):
// workgroup geometry, 16-byte entry quads, the fixed-point rounding of a product and the common epilogue
// (y = row sum + offset x_i, partial Re<x, y> per workgroup).
#pragma once

#include "dev_helpers.hpp"
#include "fixed_round.hpp"

namespace ll {

constexpr int kPbThreads = 1024;
constexpr int kPbWaves = kPbThreads / 64;

__device__ __forceinline__ void lds_add(double* p, double v) { unsafeAtomicAdd(p, v); }
// one element of the storage type into a y slice of doubles (PB phase 2 and the tiled kernel in their floating-point forms)
template <typename T> __device__ __forceinline__ void lds_add_elem(double* lds, int rl, const T& v) {
  if constexpr (scalar_traits<T>::is_complex) {
    lds_add(&lds[2 * rl], (double)v.re);
    lds_add(&lds[2 * rl + 1], (double)v.im);
  } else {
    lds_add(&lds[rl], (double)v);
  }
}
// v * 2^k, exact: the tiled image stores its values scaled by the row's exponent (pb_scatter_kernel<TILED>) and the tiled kernel
// scales the staged x to its fixed-point grid
__device__ __forceinline__ double scale_pow2(double v, int k) { return ldexp(v, k); }
__device__ __forceinline__ float scale_pow2(float v, int k) { return ldexpf(v, k); }
__device__ __forceinline__ zc scale_pow2(zc v, int k) { return zc{ldexp(v.re, k), ldexp(v.im, k)}; }
__device__ __forceinline__ cf scale_pow2(cf v, int k) { return cf{ldexpf(v.re, k), ldexpf(v.im, k)}; }

// Entries are handled in QUADS: every segment is padded to a multiple of 16 entries (zero value, local index 0), so
// a lane always moves four consecutive entries with 16-byte accesses (2 x dwordx4 of values / products, one dwordx2
// of four 16-bit indices), all four share one segment, and every run of products starts and ends on a 128-byte line.
template <typename T> struct quad {
  T e[4];
};
template <typename T> __device__ __forceinline__ quad<T> load_quad(const T* __restrict__ p) {
  constexpr int NCH = (int)(4 * sizeof(T) / 16);  // 16-byte pieces of four entries (float: 1, double / cf: 2, zc: 4)
  const uint4* src = reinterpret_cast<const uint4*>(p);
  uint4 c[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) c[i] = src[i];
  quad<T> q;
  __builtin_memcpy(&q, c, sizeof(q));
  return q;
}
template <typename T> __device__ __forceinline__ void store_quad(T* __restrict__ p, const quad<T>& q) {
  constexpr int NCH = (int)(4 * sizeof(T) / 16);
  uint4 c[NCH];
  __builtin_memcpy(c, &q, sizeof(q));
  uint4* dst = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < NCH; ++i) dst[i] = c[i];
}

__device__ __forceinline__ double pow2(int k) {  // 2^k for |k| <= 1022
  return __longlong_as_double((long long)(1023 + k) << 52);
}

constexpr long long kPbBadProduct = (long long)0x8000000000000000ull;  // "not a finite number below 2^63"
constexpr int kPbXPre = 16;      // rows per lane whose x_i the fixed-point phase 2 holds in registers (row blocks of <= 16 384 rows)
constexpr int kPbXInf = 20000;   // e_x when max|x| is not finite: every row is reported as NaN

// (fixed_round.hpp: rint() to a 64-bit integer in four full-rate additions instead of the six-instruction, mostly quarter-rate
// f64 -> i64 conversion sequence — the same integers, checked value by value on the host in tests/cpp/fixed_round_test.cpp)
__device__ __forceinline__ long long pb_to_fixed(double sc) {
  if (!(fabs(sc) < 9.0e18)) return kPbBadProduct;
  return fixed_round(sc);
}
__device__ __forceinline__ long long pb_to_fixed(double p, int k) {
  return pb_to_fixed(ldexp(p, k));  // v_ldexp_f64: one instruction, no range restrictions
}
// maximum over the workgroup of a per-lane value (result in every lane); scratch: kPbWaves doubles + 1
template <int W = kPbWaves> __device__ __forceinline__ double pb_block_max(double m, double* scratch) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d, 64));
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = scratch[0];
    for (int w = 1; w < W; ++w) t = fmax(t, scratch[w]);
    scratch[W] = t;
  }
  __syncthreads();
  return scratch[W];
}

// the shared epilogue: value(i, x_i) gives row i's sum (x_i: the row's own input element, for the diagonal term that the
// PB image keeps outside its streams); y = value + offset x, partial Re<x, y> per workgroup
template <typename T, typename F, typename G>
__device__ __forceinline__ void pb_phase2_epilogue(int rb, int64_t row0, int rows, const T* __restrict__ xl, T* __restrict__ y,
                                                   double offset, double* __restrict__ dot_partials, double* red,
                                                   const double* __restrict__ xnorm2, F&& value, G&& pre) {
  // value(i, x_i, pre(i)): pre(i) is what row i's value needs from GLOBAL memory besides x_i (its diagonal entry, its exponent).
  // All loads of a round — x_i and pre(i) of EU rows per lane, clamped addresses, no load under a divergent branch — are requested
  // before the first is used: requested inside the per-row `if (i < rows)` they form a chain of one memory latency per row, which
  // made this epilogue 12-17 us per workgroup with nothing else running on the CU.
  const double xs_fac = xnorm2 ? 1.0 / sqrt(*xnorm2) : 1.0;  // unnormalised input (see pb_phase1)
  const int tid = threadIdx.x;
  constexpr int EU = 8;  // rows per lane per round
  double dot_acc = 0.0;
  for (int i0 = tid; i0 < rows; i0 += EU * kPbThreads) {
    T xi[EU];
    decltype(pre(0)) pl[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int i = i0 + u * kPbThreads;
      const int ic = i < rows ? i : rows - 1;
      xi[u] = rmul(xs_fac, xl[row0 + ic]);
      pl[u] = pre(ic);
    }
#pragma unroll
    for (int u = 0; u < EU; ++u) {
      const int i = i0 + u * kPbThreads;
      if (i < rows) {
        const T yi = add(narrow<T>(value(i, xi[u], pl[u])), rmul(offset, xi[u]));
        y[row0 + i] = yi;
        dot_acc += re_cmul(xi[u], yi);
      }
    }
  }
  if (dot_partials) {
    const double v = wave_sum(dot_acc);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int w = 0; w < kPbWaves; ++w) t += red[w];
      dot_partials[rb] = t;
    }
  }
}

}  // namespace ll
