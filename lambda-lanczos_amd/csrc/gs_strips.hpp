// What the Gram-Schmidt / BLAS-1 translation units (kernels.hip, gs_pair.hip, gs_small.hip) share: the strip geometry with its
// loads and stores, the column-sum tail of the multi-dot trips, the grid of a strip walk, the one-sweep form's alpha correction
// (device code: for .hip files only) and, at the end, the host launchers of the small-vector geometry (gs_small.hip) that the
// public launchers of kernels.hip hand short vectors to.
#pragma once

#include "dev_helpers.hpp"
#include "ll_internal.hpp"

namespace ll {

// ================================================================= strip geometry of the BLAS-1 kernels
// A lane keeps PC 16-byte pieces of every vector of its strip in registers (EPT elements), so one strip of one basis vector is
// PC dwordx4 loads per lane.  Lanes are adjacent: the strip of 256 lanes (STREAMING geometry: one workgroup, ELEMS elements)
// or of 64 lanes (SMALL-VECTOR geometry: one wave, WAVE_ELEMS elements; four waves share it and split the basis) is contiguous.
//   PC = 4  64 B per lane, 16 KiB strips: mdot / maxpy / scale / dot / gemv_basis and the sweeps over long vectors.
//   PC = 2  the one-sweep and pair kernels on vectors of 1 .. 3 MB, which have too few 16 KiB strips to occupy the chip
//           (n = 2e5 doubles: 99 workgroups, 2.4 TB/s): twice the workgroups, each wave's chain of trips as long as before but
//           with half the bytes.  Laplacian, window 100, it/s with 4 / 2 / 1 pieces: n = 2.0e5 15.6 k / 18.4 k / 18.2 k,
//           3.6e5 14.0 k / 14.6 k / 13.7 k, 5.0e5 12.1 k / 10.0 k / 11.5 k, 1e6 7.9 k / 7.2 k / 6.9 k, config 3 604 / 589:
//           2 pieces below 200 strips of 16 KiB, 4 from there (profiles/r03_small_vector_kernel_gaps.txt).
//   PC = 1  16 B per lane (2 double / cf, 1 zc, 4 float): the small-vector kernels.
constexpr int kJB = 4;  // basis vectors per trip of the streaming multi-dot / multi-axpy loops

template <typename T, int PC = 4> struct strip {
  static constexpr int EPT = (int)(PC * 16 / sizeof(T));
  static constexpr int ELEMS = kBlock * EPT;
  static constexpr int WAVE_ELEMS = 64 * EPT;
};
// The Gram-Schmidt kernels come in two geometries: STREAMING (kernels.hip, gs_pair.hip; vectors of >= 4 MiB: enough 16 KiB
// strips to fill the chip, every load a full line) and SMALL-VECTOR (gs_small.hip; n <~ 5e5 doubles, the reference's everyday
// sizes).  The boundary is Tuning::blas_small_bytes (LL_BLAS_SMALL_BYTES: 0 = always streaming, huge = always small), handed to
// the launchers by the caller.
inline bool blas_small(int64_t n, size_t elem_bytes, int64_t limit) { return n * (int64_t)elem_bytes < limit; }

// Balanced persistent grid: every workgroup walks the same number of strips (grid-stride), so no tail round.
// (Measured alternative, round 2: equal CONTIGUOUS shares per workgroup instead of strips dealt out round-robin —
// perfectly balanced, but 8 % slower on the Gram-Schmidt kernels (5.35 vs 5.83 TB/s at n = 1e7): with the round-robin
// walk the whole chip sweeps each basis vector front to back, which is what the HBM row buffers like.)
// Grid target: 1024 workgroups, but ONE per CU once a vector has more than ~2.25 16-KiB strips per CU (> 9 MiB): every
// workgroup then sweeps several strips back to back — config 3 (80 MB vectors): 6.0 instead of 5.9 TB/s; the 40 / 20 /
// 10 MB shards of config 4: Gram-Schmidt -13 % / -9 % / -3 % (profiles/r02_strip_grid_sweep.txt).  At 8 MiB (config 2,
// 489 strips) the small grid is 2 % slower: too few strips to balance.
inline int strip_grid(int64_t n, int elems) {
  int64_t strips = (n + elems - 1) / elems;
  if (strips < 1) strips = 1;
  const bool streaming = elems >= 1024;  // the small-vector kernels' strips are 64 .. 256 elements
  const int target = streaming && strips > 2 * kCUs + kCUs / 4 ? kCUs : 1024;
  const int64_t per = (strips + target - 1) / target;
  return (int)((strips + per - 1) / per);
}

// i0: the lane's first element (strip start + lane index * EPT).  A lane's EPT elements are contiguous and lanes are adjacent:
// with PC = 4 the four loads of a wave cover 4 KiB of consecutive memory, each of them touching the same 32 lines (the 2nd to
// 4th hit in L1 / merge with the outstanding misses).  Measured alternatives, round 2 (A/B in one process through a device
// flag): 16-byte pieces laid out so that every single instruction is contiguous over the workgroup, or over the wave: 5.67-5.71
// vs 5.71-5.80 TB/s at n = 1e7 (no gain) and slower at n = 1e6 — this layout stays.  The vector's ragged end is read element by
// element and padded with zeros.
template <typename T, int PC = 4>
__device__ __forceinline__ void load_strip(const T* __restrict__ v, int64_t i0, int64_t n, T (&r)[strip<T, PC>::EPT]) {
  constexpr int EPT = strip<T, PC>::EPT;
  if (i0 + EPT <= n) {
    const uint4* p = reinterpret_cast<const uint4*>(v + i0);
    uint4 c[PC];
#pragma unroll
    for (int e = 0; e < PC; ++e) c[e] = p[e];
    __builtin_memcpy(&r[0], c, sizeof(c));
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e) r[e] = (i0 + e < n) ? v[i0 + e] : zero<T>();
  }
}
template <typename T, int PC = 4>
__device__ __forceinline__ void store_strip(T* __restrict__ v, int64_t i0, int64_t n, const T (&r)[strip<T, PC>::EPT]) {
  constexpr int EPT = strip<T, PC>::EPT;
  if (i0 + EPT <= n) {
    uint4 c[PC];
    __builtin_memcpy(c, &r[0], sizeof(c));
    uint4* p = reinterpret_cast<uint4*>(v + i0);
#pragma unroll
    for (int e = 0; e < PC; ++e) p[e] = c[e];
  } else {
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (i0 + e < n) v[i0 + e] = r[e];
  }
}

// The tail of a multi-dot trip: NV column sums (re / im[b]: this lane's share of column b; im is ignored for real types) are
// reduced over the wave and added to the wave's LDS row, column b at mine_col[reals * b ..].
// Real and imaginary parts go through transposed reductions of their own, at most NV = 4 sums each: with all 2 NV sums (8 or 16
// in the pair sweep, which interleaves two column sets in a tail of its own) in one reduction the compiler sends part of the
// array through scratch memory, a round trip with a full drain of the memory pipeline in every trip (checked in the ISA, round
// 5).  The butterfly adds the lanes in the same order whatever NV and whatever the column's position in the trip: a column's
// bits do not depend on how the stored vectors are cut into trips.
template <typename T, int NV>
__device__ __forceinline__ void add_column_sums(double (&re)[NV], double (&im)[NV], double* mine_col, int lane) {
  constexpr int LPI = 64 / NV;  // lanes that end up holding the same sum
  wave_sum_transposed<NV>(re, lane);
  if constexpr (scalar_traits<T>::is_complex) {
    wave_sum_transposed<NV>(im, lane);
    if ((lane & (LPI - 1)) == 0) {
      mine_col[2 * (lane / LPI)] += re[0];
      mine_col[2 * (lane / LPI) + 1] += im[0];
    }
  } else {
    if ((lane & (LPI - 1)) == 0) mine_col[lane / LPI] += re[0];
  }
}

// ================================================================= loads and stores of the software-pipelined sweeps (gs_pair.hip,
// gs_block.hip)
// Address-space casts for the pipelined sweeps.  A pointer that reaches a load through a table or a lambda has lost what lets
// the compiler pick the cheap instruction: uniform reads of data no kernel writes while it runs (coefficients, the pointer table)
// go through the CONSTANT address space (s_load: scalar cache, no vmcnt slot — a vector load in the middle of a trip would be
// younger than the prefetched strips and turn the trip's wait into a full drain), strips through the GLOBAL one (global_load with
// an SGPR base instead of flat_load, which also occupies the LDS counter).
__device__ __forceinline__ double ld_const(const double* p, int i) {
  return reinterpret_cast<const __attribute__((address_space(4))) double*>(reinterpret_cast<uintptr_t>(p))[i];
}
template <typename T> __device__ __forceinline__ const T* ld_const_ptr(const T* const* tab, int i) {
  return reinterpret_cast<const T*>(reinterpret_cast<const __attribute__((address_space(4))) uintptr_t*>(reinterpret_cast<uintptr_t>(tab))[i]);
}
typedef unsigned int ll_u4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) char* ll_gcp;
typedef __attribute__((address_space(1))) char* ll_gp;
__device__ __forceinline__ uint4 ld_global16(const char* uniform_base, unsigned lane_off) {
  const ll_gcp g = (ll_gcp)uniform_base;  // generic -> global
  const ll_u4v v = *(const __attribute__((address_space(1))) ll_u4v*)(g + lane_off);
  uint4 r;
  __builtin_memcpy(&r, &v, sizeof(r));
  return r;
}
__device__ __forceinline__ void st_global16(char* uniform_base, unsigned lane_off, uint4 x) {
  const ll_gp g = (ll_gp)uniform_base;
  ll_u4v v;
  __builtin_memcpy(&v, &x, sizeof(v));
  *(__attribute__((address_space(1))) ll_u4v*)(g + lane_off) = v;
}
// A strip at a UNIFORM base: whole strips (FULL) through global_load / global_store with an SGPR base and a 32-bit lane offset,
// the vector's ragged last strip through the guarded loads above.
template <typename T, int PC, bool FULL>
__device__ __forceinline__ void load_lstrip_u(const T* __restrict__ v, int64_t base, int64_t n, T (&r)[strip<T, PC>::EPT]) {
  if constexpr (FULL) {
    constexpr int EPT = strip<T, PC>::EPT;
    const char* sb = reinterpret_cast<const char*>(v + base);  // uniform
    const unsigned off = threadIdx.x * (unsigned)(EPT * sizeof(T));
    uint4 c[PC];
#pragma unroll
    for (int e = 0; e < PC; ++e) c[e] = ld_global16(sb, off + 16u * e);
    __builtin_memcpy(&r[0], c, sizeof(c));
  } else {
    load_strip<T, PC>(v, base + (int64_t)threadIdx.x * strip<T, PC>::EPT, n, r);
  }
}
template <typename T, int PC, bool FULL>
__device__ __forceinline__ void store_lstrip_u(T* __restrict__ v, int64_t base, int64_t n, const T (&r)[strip<T, PC>::EPT]) {
  if constexpr (FULL) {
    constexpr int EPT = strip<T, PC>::EPT;
    char* sb = reinterpret_cast<char*>(v + base);
    const unsigned off = threadIdx.x * (unsigned)(EPT * sizeof(T));
    uint4 c[PC];
    __builtin_memcpy(c, &r[0], sizeof(c));
#pragma unroll
    for (int e = 0; e < PC; ++e) st_global16(sb, off + 16u * e, c[e]);
  } else {
    store_strip<T, PC>(v, base + (int64_t)threadIdx.x * strip<T, PC>::EPT, n, r);
  }
}

// alpha of a lagged iteration without the perturbation's terms (see the one-sweep form in kernels.hip):
// <u + e, A (u + e)> = alpha + 2 Re <e, A u> + <e, A e> with <e, A u_{k-1}> = conj(c_{k-2}) beta_{k-2} = conj(g_{k-2}) and
// q = <e, A e> = Re c^H t (lagged_fold_kernel).  Same operations in the sweeps of both geometries and in the fold: same bits.
__device__ __forceinline__ double lagged_alpha(double alpha, double g_last_re, double q) {
  return fma(-2.0, g_last_re, alpha) - q;
}

// ================================================================= the small-vector geometry's launchers (gs_small.hip)
// What launch_mdot / launch_maxpy / launch_lagged (kernels.hip) call for vectors below their small-vector limit; the arguments
// are the kernels'.  Each returns its grid.
template <typename T>
int launch_mdot_small(int64_t n, T* w, const BasisSegs<T>& segs, const ThreeTerm<T>& tt, const NormRefs& pred, int predicated,
                      double* partials, int ncols, hipStream_t s);
template <typename T>
int launch_maxpy_small(int64_t n, T* w, const BasisSegs<T>& segs, const double* h, int nb, const NormRefs& pred, int predicated,
                       double* partials, hipStream_t s);
template <typename T>
int launch_lagged_small(int64_t n, T* w, const BasisSegs<T>& segs, int nb, const Lagged<T>& lg, const ThreeTerm<T>& tt,
                        double* partials, hipStream_t s);

}  // namespace ll
