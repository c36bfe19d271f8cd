// The two-pass Lanczos recurrence without a stored basis (two_pass_run.cpp, expo_two_pass_multi_run.cpp): the plain
// three-term update on UNNORMALISED vectors, once with its coefficient record and norm (pass 1) and once replayed from the record
// while the result — the Ritz vector, or exp(a A) v — is accumulated (pass 2).  Streaming strip kernels in the geometry of
// kernels.hip (strip<T>, 16 KiB strips, balanced persistent grid); both passes go through ONE element update (recur_update), so
// pass 2 reproduces pass 1's vectors bit for bit.
//
// Reference rows:
//   a4     recur_step / recur_accum   three-term update (LL:251-257) on r_k = ||r_k|| u_k
//   a7     recur_step + recur_fold    ||w||^2 (LA:56-60 at LL:262); a8 is left to the next operator kernel (its input scale)
//   a9     recur_accum                Ritz vector sum_k s_k u_k (LL:51-57), one term per replayed iteration; with a complex
//                                     coefficient the Exponentiator's output sum_l coeff[l] u_l (EX:163-170)
//
// Bytes and launches per iteration beyond the operator (s = sizeof(T), n elements):
//   pass 1  recur_step_kernel   reads y, x, p, writes y: 4 s n bytes (3 s n at k = 0), one launch; the fold of the workgroups'
//           partial ||y||^2 and the publish step are recur_fold_kernel, a second launch of ONE workgroup (8 bytes per workgroup
//           of the first).
//   pass 2  recur_accum_kernel  reads y, x, p, psi, writes y, psi: 6 s n bytes (5 s n at k = 0), one launch, no reduction.
//           The complex-coefficient instantiations (T = zc, cf with G = zc) move the same bytes; recur_seed_kernel (psi = g_0 r_0,
//           once per Exponentiator run) reads x and writes psi: 2 s n bytes.
//           recur_accum_multi_kernel (several accumulators, the multi-time Exponentiator) reads y, x, p, writes y, and reads and
//           writes each of the s' ACTIVE accumulators: (4 + 2 s') s n bytes (3 + 2 s' at k = 0), one launch, against 6 s' s n for s'
//           launches of recur_accum_kernel.
// Registers (compiler's resource-usage remarks, gfx950, 256 threads): recur_accum_kernel<T, double> 76 / 72 / 80 / 82 VGPRs for
// d / z / s / c, as before the coefficient type became a parameter; <zc, zc> 72, <cf, zc> 84; recur_seed_kernel 28 to 48.
// recur_accum_multi_kernel<T, G, 2> (two accumulators loaded before the first is stored) 78 / 68 / 98 / 114 VGPRs for d / z / s / c
// (6 / 7 / 4 / 4 waves per SIMD); with one at a time 56 / 54 / 60 / 70, with four 114 / 104 / 136 / 150.  No instantiation uses
// scratch.
// The multi kernel on 256 MiB complex-double vectors (tools/expo_two_pass_multi_rate.py; microseconds per launch, 20
// launches between synchronisations, median of 5, one process per batch size, recur_accum_kernel in the same process first):
//   batch 1: 309 | 316, 415, 635, 1097 for 1, 2, 4, 8 accumulators;  batch 2: 295 | 303, 420, 650, 1067;  batch 4: 293 | 306, 423,
//   628, 1014 — 4.9 to 5.3 TB/s of the byte model throughout.  The batch sizes differ by less than the 5 % between processes on
//   the unchanged single kernel, except at 8 accumulators (batch 4 is 5 % ahead of batch 2); batch 2 stays, for the registers.
//   With ONE accumulator the multi kernel is 3 % slower than recur_accum_kernel in all three: the driver hands launches with one
//   active accumulator to recur_accum_kernel (same bits).
// Kernel times and shares of peak: unmeasured.  Whole passes (tools/two_pass_rate.py): 2 015 and 1 845 it/s on
// 128 MiB vectors with the Pauli-sum operator of 24 sites; the Exponentiator's two passes together (tools/expo_two_pass_rate.py):
// 488 it/s on 256 MiB complex vectors, 11 iterations, against 832 it/s for the stored-basis run.
#include "gs_strips.hpp"

namespace ll {

// y' = y - a x - b p (p == nullptr: y' = y - a x): two products and two subtractions in T, in this order, in both passes
template <typename T> __device__ __forceinline__ T recur_update(T y, T x, T p, double a, double b, bool with_p) {
  T r = sub(y, rmul(a, x));
  if (with_p) r = sub(r, rmul(b, p));
  return r;
}

// One record per iteration k on the device, kRecurRec doubles: alpha_k, a_k, b_k, c_k = ||r_k||^2 (ll_internal.hpp).
// Pass 1.  y holds (A + offset)(x / ||x||) on entry, x = r_k with ||r_k||^2 = rec[k].c, p = r_{k-1} (nullptr at k = 0).
// normalised: x and p have been scaled to unit norm in place (callback operators, whose input the library normalises): then
// a = alpha and b = ||r_k||, else a = alpha / ||r_k|| and b = ||r_k|| / ||r_{k-1}||.
template <typename T>
__global__ __launch_bounds__(kBlock) void recur_step_kernel(int64_t n, T* __restrict__ y, const T* __restrict__ x,
                                                            const T* __restrict__ p, const double* __restrict__ alpha_partials,
                                                            int alpha_nparts, double* __restrict__ rec, int64_t k, int normalised,
                                                            double* __restrict__ partials) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  __shared__ double fold_scratch[5];
  __shared__ double red[4];
  // deferred alpha: every workgroup folds the operator kernel's partials in the same fixed order (ThreeTerm)
  const double alpha = fold_partials_all(alpha_partials, alpha_nparts, fold_scratch);
  double* const mine = rec + kRecurRec * k;
  const double ck = mine[3];
  const double nx = sqrt(ck);
  const double a = normalised ? alpha : alpha / nx;
  const double b = p == nullptr ? 0.0 : (normalised ? nx : sqrt(ck / mine[3 - kRecurRec]));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    mine[0] = alpha;
    mine[1] = a;
    mine[2] = b;
  }
  double nn = 0.0;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t i0 = sidx * ELEMS + (int64_t)threadIdx.x * EPT;
    T yr[EPT], xr[EPT], pr[EPT];
    load_strip<T>(y, i0, n, yr);
    load_strip<T>(x, i0, n, xr);
    if (p) load_strip<T>(p, i0, n, pr);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      yr[e] = recur_update(yr[e], xr[e], p ? pr[e] : xr[e], a, b, p != nullptr);
      nn += abs2(yr[e]);
    }
    store_strip<T>(y, i0, n, yr);
  }
  const double tot = block_sum(nn, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// The fold of pass 1's norm partials (one workgroup, the fixed order of reduce_one_kernel): c_{k+1} = ||r_{k+1}||^2 into the next
// record, and iteration k's scalars (alpha_k, beta_k^2 = c_{k+1}, 0, c_{k+1}) into the pinned host slot.
__global__ __launch_bounds__(kBlock) void recur_fold_kernel(const double* __restrict__ partials, int nparts,
                                                            double* __restrict__ rec, int64_t k, double* __restrict__ host) {
  __shared__ double fold_scratch[5];
  const double tot = fold_partials_all(partials, nparts, fold_scratch);
  if (threadIdx.x == 0) {
    rec[kRecurRec * (k + 1) + 3] = tot;
    host[0] = rec[kRecurRec * k];
    host[1] = tot;
    host[2] = 0.0;
    host[3] = tot;
  }
}

// The accumulate's coefficient g is real (the eigen-solver's Ritz vector) or complex (the Exponentiator's exp(a T_m) e_1 on complex
// vectors): g y in T.  Real: the two real products of rmul.  Complex: g is rounded to T once, then the four products, one subtraction
// and one addition of mul, each rounded on its own (the library is built without contraction).
template <typename T> __device__ __forceinline__ T gmul(double g, T y) { return rmul(g, y); }
__device__ __forceinline__ zc gmul(zc g, zc y) { return mul(g, y); }
__device__ __forceinline__ cf gmul(zc g, cf y) { return mul(cf{(float)g.re, (float)g.im}, y); }

// Pass 2.  The same update with (a, b) READ from the record (a, b given by value when rec == nullptr: the primitives
// ll_recur_accum_* and ll_recur_accum_scaled), then psi += g y with g = gvec[k + 1] (or by value); G = double, or zc on complex
// vectors.  Nothing is recomputed and nothing is reduced over the vector.  Workgroup 0 folds the alpha the operator kernel left
// behind and counts, in *mismatches, the iterations whose alpha differs AS BITS from the recorded one (the replay invariant;
// alpha_partials == nullptr: no check).
template <typename T, typename G>
__global__ __launch_bounds__(kBlock) void recur_accum_kernel(int64_t n, T* __restrict__ y, const T* __restrict__ x,
                                                             const T* __restrict__ p, T* __restrict__ psi,
                                                             const double* __restrict__ rec, const G* __restrict__ gvec,
                                                             int64_t k, double a_val, double b_val, G g_val,
                                                             const double* __restrict__ alpha_partials, int alpha_nparts,
                                                             long long* __restrict__ mismatches) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  const double a = rec ? rec[kRecurRec * k + 1] : a_val;
  const double b = rec ? rec[kRecurRec * k + 2] : b_val;
  const G g = gvec ? gvec[k + 1] : g_val;
  if (alpha_partials != nullptr && blockIdx.x == 0) {  // (uniform over the workgroup)
    __shared__ double fold_scratch[5];
    const double alpha = fold_partials_all(alpha_partials, alpha_nparts, fold_scratch);
    if (threadIdx.x == 0 && __double_as_longlong(alpha) != __double_as_longlong(rec[kRecurRec * k])) *mismatches += 1;
  }
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t i0 = sidx * ELEMS + (int64_t)threadIdx.x * EPT;
    T yr[EPT], xr[EPT], pr[EPT], qr[EPT];
    load_strip<T>(y, i0, n, yr);
    load_strip<T>(x, i0, n, xr);
    if (p) load_strip<T>(p, i0, n, pr);
    load_strip<T>(psi, i0, n, qr);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      yr[e] = recur_update(yr[e], xr[e], p ? pr[e] : xr[e], a, b, p != nullptr);
      qr[e] = add(qr[e], gmul(g, yr[e]));
    }
    store_strip<T>(y, i0, n, yr);
    store_strip<T>(psi, i0, n, qr);
  }
}

// Pass 2 for SEVERAL outputs (ll_expo_two_pass_multi: one Krylov space, one accumulator per time): the update of
// recur_accum_kernel once per strip, then psi_j += g_j y' for the acc.count accumulators that are still active, with the same two
// device functions in the same order, so every psi_j holds the bits recur_accum_kernel gives it alone.  An accumulator that is not
// in the list is not touched.  g_j = gtab[acc.row[j] * ldg + k + 1] (gtab == nullptr: acc.g[j], the primitive
// ll_recur_accum_multi).  The list and the coefficients are uniform reads from the kernel arguments and, for gtab, through the
// constant address space (gs_strips.hpp: a vector load in the middle of the strip would be younger than the strip's loads).
// NB accumulators are loaded before the first of them is stored.  Reads y, x, p, writes y, and reads and writes each active
// psi_j: (4 + 2 count) s n bytes (3 + 2 count at k = 0), one launch.  Workgroup 0: as in recur_accum_kernel.
__device__ __forceinline__ double ld_coeff(const double* p, int64_t i) {
  return reinterpret_cast<const __attribute__((address_space(4))) double*>(reinterpret_cast<uintptr_t>(p))[i];
}
__device__ __forceinline__ zc ld_coeff(const zc* p, int64_t i) {
  const double* d = reinterpret_cast<const double*>(p);
  return zc{ld_coeff(d, 2 * i), ld_coeff(d, 2 * i + 1)};
}
template <typename T, typename G, int NB>
__device__ __forceinline__ void recur_accum_group(const RecurMultiArgs<T, G>& acc, const G* gtab, int64_t ldg, int64_t k, int j0,
                                                  int64_t i0, int64_t n, const T (&yr)[strip<T>::EPT]) {
  constexpr int EPT = strip<T>::EPT;
  T qr[NB][EPT];
#pragma unroll
  for (int b = 0; b < NB; ++b) load_strip<T>(acc.psi[j0 + b], i0, n, qr[b]);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const G g = gtab ? ld_coeff(gtab, (int64_t)acc.row[j0 + b] * ldg + k + 1) : acc.g[j0 + b];
#pragma unroll
    for (int e = 0; e < EPT; ++e) qr[b][e] = add(qr[b][e], gmul(g, yr[e]));
    store_strip<T>(acc.psi[j0 + b], i0, n, qr[b]);
  }
}
template <typename T, typename G, int NB>
__global__ __launch_bounds__(kBlock) void recur_accum_multi_kernel(int64_t n, T* __restrict__ y, const T* __restrict__ x,
                                                                   const T* __restrict__ p, const RecurMultiArgs<T, G> acc,
                                                                   const double* __restrict__ rec, const G* gtab, int64_t ldg,
                                                                   int64_t k, double a_val, double b_val,
                                                                   const double* __restrict__ alpha_partials, int alpha_nparts,
                                                                   long long* __restrict__ mismatches) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  const double a = rec ? rec[kRecurRec * k + 1] : a_val;
  const double b = rec ? rec[kRecurRec * k + 2] : b_val;
  if (alpha_partials != nullptr && blockIdx.x == 0) {  // (uniform over the workgroup)
    __shared__ double fold_scratch[5];
    const double alpha = fold_partials_all(alpha_partials, alpha_nparts, fold_scratch);
    if (threadIdx.x == 0 && __double_as_longlong(alpha) != __double_as_longlong(rec[kRecurRec * k])) *mismatches += 1;
  }
  const int count = acc.count;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t i0 = sidx * ELEMS + (int64_t)threadIdx.x * EPT;
    T yr[EPT], xr[EPT], pr[EPT];
    load_strip<T>(y, i0, n, yr);
    load_strip<T>(x, i0, n, xr);
    if (p) load_strip<T>(p, i0, n, pr);
#pragma unroll
    for (int e = 0; e < EPT; ++e) yr[e] = recur_update(yr[e], xr[e], p ? pr[e] : xr[e], a, b, p != nullptr);
    store_strip<T>(y, i0, n, yr);
    int j = 0;
    for (; j + NB <= count; j += NB) recur_accum_group<T, G, NB>(acc, gtab, ldg, k, j, i0, n, yr);
    if constexpr (NB > 2)
      if (j + 2 <= count) {
        recur_accum_group<T, G, 2>(acc, gtab, ldg, k, j, i0, n, yr);
        j += 2;
      }
    if constexpr (NB > 1)
      if (j < count) recur_accum_group<T, G, 1>(acc, gtab, ldg, k, j, i0, n, yr);
  }
}

// The first term of pass 2's sum where g is not a real host value: psi = g x, out of place, with the product of the accumulate.
// Reads x, writes psi: 2 s n bytes, once per run.
template <typename T, typename G>
__global__ __launch_bounds__(kBlock) void recur_seed_kernel(int64_t n, T* __restrict__ psi, const T* __restrict__ x, G g) {
  constexpr int EPT = strip<T>::EPT;
  constexpr int ELEMS = strip<T>::ELEMS;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t i0 = sidx * ELEMS + (int64_t)threadIdx.x * EPT;
    T xr[EPT], qr[EPT];
    load_strip<T>(x, i0, n, xr);
#pragma unroll
    for (int e = 0; e < EPT; ++e) qr[e] = gmul(g, xr[e]);
    store_strip<T>(psi, i0, n, qr);
  }
}

template <typename T>
int launch_recur_step(int64_t n, T* y, const T* x, const T* p, const double* alpha_partials, int alpha_nparts, double* rec,
                      int64_t k, bool normalised, double* partials, hipStream_t s) {
  const int grid = strip_grid(n, strip<T>::ELEMS);
  hipLaunchKernelGGL((recur_step_kernel<T>), dim3(grid), dim3(kBlock), 0, s, n, y, x, p, alpha_partials, alpha_nparts, rec, k,
                     normalised ? 1 : 0, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
void launch_recur_fold(const double* partials, int nparts, double* rec, int64_t k, double* host_mapped, hipStream_t s) {
  hipLaunchKernelGGL(recur_fold_kernel, dim3(1), dim3(kBlock), 0, s, partials, nparts, rec, k, host_mapped);
  LL_HIP(hipGetLastError());
}
template <typename T, typename G>
void launch_recur_accum(int64_t n, T* y, const T* x, const T* p, T* psi, const double* rec, const G* gvec, int64_t k, double a,
                        double b, G g, const double* alpha_partials, int alpha_nparts, long long* mismatches, hipStream_t s) {
  static_assert(std::is_same<G, double>::value || scalar_traits<T>::is_complex, "a complex coefficient needs complex vectors");
  hipLaunchKernelGGL((recur_accum_kernel<T, G>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, y, x, p, psi, rec,
                     gvec, k, a, b, g, alpha_partials, alpha_nparts, mismatches);
  LL_HIP(hipGetLastError());
}
template <typename T>
void launch_recur_accum_multi(int64_t n, T* y, const T* x, const T* p, const RecurMultiArgs<T, typename RecurCoeff<T>::type>& acc,
                              const double* rec, const typename RecurCoeff<T>::type* gtab, int64_t ldg, int64_t k, double a,
                              double b, const double* alpha_partials, int alpha_nparts, long long* mismatches, hipStream_t s) {
  typedef typename RecurCoeff<T>::type G;
  hipLaunchKernelGGL((recur_accum_multi_kernel<T, G, kRecurMultiBatch>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n,
                     y, x, p, acc, rec, gtab, ldg, k, a, b, alpha_partials, alpha_nparts, mismatches);
  LL_HIP(hipGetLastError());
}
template <typename T, typename G> void launch_recur_seed(int64_t n, T* psi, const T* x, G g, hipStream_t s) {
  static_assert(std::is_same<G, double>::value || scalar_traits<T>::is_complex, "a complex coefficient needs complex vectors");
  hipLaunchKernelGGL((recur_seed_kernel<T, G>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, psi, x, g);
  LL_HIP(hipGetLastError());
}

// accumulate: a real coefficient on every storage type (the eigen-solver's Ritz vector; the primitive ll_recur_accum_*), a complex
// one on the complex types; seed: the Exponentiator's coefficient type only (RecurCoeff<T>)
#define LL_INST_RECUR_ACCUM(T, G)                                                                                                \
  template void launch_recur_accum<T, G>(int64_t, T*, const T*, const T*, T*, const double*, const G*, int64_t, double, double, \
                                         G, const double*, int, long long*, hipStream_t);
#define LL_INST_RECUR_SEED(T, G) template void launch_recur_seed<T, G>(int64_t, T*, const T*, G, hipStream_t);
#define LL_INST_RECUR(T)                                                                                                       \
  template int launch_recur_step<T>(int64_t, T*, const T*, const T*, const double*, int, double*, int64_t, bool, double*,      \
                                    hipStream_t);                                                                              \
  LL_INST_RECUR_ACCUM(T, double)
LL_FOR_EACH_SCALAR(LL_INST_RECUR)
#define LL_INST_RECUR_MULTI(T)                                                                                                   \
  template void launch_recur_accum_multi<T>(int64_t, T*, const T*, const T*, const RecurMultiArgs<T, RecurCoeff<T>::type>&,      \
                                            const double*, const RecurCoeff<T>::type*, int64_t, int64_t, double, double,         \
                                            const double*, int, long long*, hipStream_t);
LL_FOR_EACH_SCALAR(LL_INST_RECUR_MULTI)
LL_INST_RECUR_SEED(double, double)
LL_INST_RECUR_SEED(float, double)
LL_INST_RECUR_ACCUM(zc, zc)
LL_INST_RECUR_SEED(zc, zc)
LL_INST_RECUR_ACCUM(cf, zc)
LL_INST_RECUR_SEED(cf, zc)

}  // namespace ll
