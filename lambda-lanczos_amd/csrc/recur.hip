// The two-pass Lanczos recurrence without a stored basis (two_pass_run.cpp, expo_two_pass_run.cpp): the plain
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
// Registers (compiler's resource-usage remarks, gfx950, 256 threads): recur_accum_kernel<T, double> 76 / 72 / 80 / 82 VGPRs for
// d / z / s / c, as before the coefficient type became a parameter; <zc, zc> 72, <cf, zc> 84; recur_seed_kernel 28 to 48.  No
// instantiation uses scratch.
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
namespace {
template <typename T, typename G>
void launch_recur_accum_g(int64_t n, T* y, const T* x, const T* p, T* psi, const double* rec, const G* gvec, int64_t k, double a,
                          double b, G g, const double* alpha_partials, int alpha_nparts, long long* mismatches, hipStream_t s) {
  hipLaunchKernelGGL((recur_accum_kernel<T, G>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, y, x, p, psi, rec,
                     gvec, k, a, b, g, alpha_partials, alpha_nparts, mismatches);
  LL_HIP(hipGetLastError());
}
template <typename T, typename G> void launch_recur_seed_g(int64_t n, T* psi, const T* x, G g, hipStream_t s) {
  hipLaunchKernelGGL((recur_seed_kernel<T, G>), dim3(strip_grid(n, strip<T>::ELEMS)), dim3(kBlock), 0, s, n, psi, x, g);
  LL_HIP(hipGetLastError());
}
}  // namespace
template <typename T>
void launch_recur_accum(int64_t n, T* y, const T* x, const T* p, T* psi, const double* rec, const double* gvec, int64_t k,
                        double a, double b, double g, const double* alpha_partials, int alpha_nparts, long long* mismatches,
                        hipStream_t s) {
  launch_recur_accum_g<T, double>(n, y, x, p, psi, rec, gvec, k, a, b, g, alpha_partials, alpha_nparts, mismatches, s);
}
template <typename T>
void launch_recur_accum_cplx(int64_t n, T* y, const T* x, const T* p, T* psi, const double* rec, const zc* gvec, int64_t k,
                             double a, double b, zc g, const double* alpha_partials, int alpha_nparts, long long* mismatches,
                             hipStream_t s) {
  static_assert(scalar_traits<T>::is_complex, "a complex coefficient needs complex vectors");
  launch_recur_accum_g<T, zc>(n, y, x, p, psi, rec, gvec, k, a, b, g, alpha_partials, alpha_nparts, mismatches, s);
}
template <typename T> void launch_recur_seed(int64_t n, T* psi, const T* x, double g, hipStream_t s) {
  launch_recur_seed_g<T, double>(n, psi, x, g, s);
}
template <typename T> void launch_recur_seed_cplx(int64_t n, T* psi, const T* x, zc g, hipStream_t s) {
  static_assert(scalar_traits<T>::is_complex, "a complex coefficient needs complex vectors");
  launch_recur_seed_g<T, zc>(n, psi, x, g, s);
}

#define LL_INST_RECUR(T)                                                                                                       \
  template int launch_recur_step<T>(int64_t, T*, const T*, const T*, const double*, int, double*, int64_t, bool, double*,      \
                                    hipStream_t);                                                                              \
  template void launch_recur_accum<T>(int64_t, T*, const T*, const T*, T*, const double*, const double*, int64_t, double,      \
                                      double, double, const double*, int, long long*, hipStream_t);
LL_FOR_EACH_SCALAR(LL_INST_RECUR)
// the Exponentiator's coefficients: real on real vectors, complex on complex ones
template void launch_recur_seed<double>(int64_t, double*, const double*, double, hipStream_t);
template void launch_recur_seed<float>(int64_t, float*, const float*, double, hipStream_t);
#define LL_INST_RECUR_CPLX(T)                                                                                                  \
  template void launch_recur_accum_cplx<T>(int64_t, T*, const T*, const T*, T*, const double*, const zc*, int64_t, double,     \
                                           double, zc, const double*, int, long long*, hipStream_t);                           \
  template void launch_recur_seed_cplx<T>(int64_t, T*, const T*, zc, hipStream_t);
LL_INST_RECUR_CPLX(zc)
LL_INST_RECUR_CPLX(cf)

}  // namespace ll
