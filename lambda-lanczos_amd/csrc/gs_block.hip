// UP TO EIGHT Lanczos iterations per sweep over a RAW basis (the "block" form), streaming geometry: the prediction through the
// recorded tridiagonal, the software-pipelined sweep and the fold.  Executable specification, launch by launch, with the
// derivation and the numbers: tools/block_gs_model.py (profiles/block_gs_model.txt).  The raw three-term update between the
// operator applications is pair_three_term_kernel (gs_pair.hip).
//
// The stored vectors are never rewritten: the basis holds a_0, a_1, ..., every a_j the raw three-term vector of its iteration,
// unnormalised.  Beside them the loop keeps rho_j^2 (squared norm of the part of a_j orthogonal to its predecessors) and the
// measured, eps-sized coefficients C_j[l] = <u_l, a_j>, l < j (rows of a packed triangle, row j at reals * j (j - 1) / 2).  The
// orthonormal u_j = (a_j - sum_l C_j[l] u_l) / rho_j exist only implicitly; consumers transform their coefficient vectors to
// first order in C (LoopState::ritz_basis, LoopState::block_flush).  State between blocks: a_0 .. a_k stored, alpha_0 ..
// alpha_{k-1}, beta_j = rho_{j+1} recorded.  One block of m <= 8 iterations (eight: real double only, behind the host's guard, kBlock8Tau):
//   m x (operator kernel on x / |x|, fused dot e_s; pair_three_term_kernel: b_s = y - e_s x - |x| x_prev, |b_s|^2)
//   block_predict_kernel   alpha_k from e_0; p_s = predicted components of b_s along u_0 .. u_k; the compensation coefficients
//   block_sweep_kernel     ONE pass over a_0 .. a_k: <a_j, b_s> for all j, s; b_{m-1} and b_{m-2} (BOTH operands of the next block's
//                          first three-term update) lose their predicted components; the Gram matrix of the new vectors; writes
//                          only those two vectors
//   block_fold_kernel      rows k+1 .. k+m of C, their rho^2, alpha_{k+1} .. alpha_{k+m-1}, beta_k .. beta_{k+m-1}, the gate values
// Reference rows: a4 (three-term, LL:251-257), a5-a7 (Gram-Schmidt and norm, LL:259-262), m iterations at a time.
#include <algorithm>

#include "gs_strips.hpp"

namespace ll {

namespace {
// sums over the workgroup of two values at once, returned to every thread.  sh: 8 doubles of LDS.
__device__ __forceinline__ void block_sum2_all(double& a, double& b, double* sh) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sh[wave] = a;
    sh[4 + wave] = b;
  }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}
__device__ __forceinline__ void block_max2_all(double& a, double& b, double* sh) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    a = fmax(a, __shfl_down(a, d, 64));
    b = fmax(b, __shfl_down(b, d, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sh[wave] = a;
    sh[4 + wave] = b;
  }
  __syncthreads();
  a = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  b = fmax(fmax(sh[4], sh[5]), fmax(sh[6], sh[7]));
}
// entry i of (T v) over the first m Lanczos vectors (reals numbers per column); alpha_{m-1} may not be recorded yet
__device__ __forceinline__ double block_tri_row(const double* __restrict__ ha, const double* __restrict__ hb, const double* v, int i,
                                                int reals, int m, double alpha_last) {
  const int j = i / reals;
  double t = (j == m - 1 ? alpha_last : ha[j]) * v[i];
  if (j >= 1) t = fma(hb[j - 1], v[i - reals], t);
  if (j + 1 < m) t = fma(hb[j], v[i + reals], t);
  return t;
}
__device__ __forceinline__ size_t block_row_at(int reals, int j) { return (size_t)reals * (size_t)j * (size_t)(j - 1) / 2; }
}  // namespace

// Entering the form from the one-sweep state: u_0 .. u_{k-1} complete in the basis (rho = 1, rows of zeros, of which only row
// k - 1 is ever read), a_k raw with its measured coefficients g (reals * k) and rho_k^2 = *c1.
__global__ __launch_bounds__(256) void block_enter_kernel(int k, int reals, const double* __restrict__ g, const double* __restrict__ c1,
                                                          double* __restrict__ rho2, double* __restrict__ cpk) {
  const int tid = threadIdx.x;
  for (int j = tid; j < k; j += 256) rho2[j] = 1.0;
  if (tid == 0) rho2[k] = *c1;
  double* rk1 = cpk + block_row_at(reals, k - 1);
  for (int i = tid; i < reals * (k - 1); i += 256) rk1[i] = 0.0;
  double* rk = cpk + block_row_at(reals, k);
  for (int i = tid; i < reals * k; i += 256) rk[i] = g[i];
}
void launch_block_enter(int k, int reals, const double* g, const double* c1, double* rho2, double* cpk, hipStream_t s) {
  hipLaunchKernelGGL(block_enter_kernel, dim3(1), dim3(256), 0, s, k, reals, g, c1, rho2, cpk);
  LL_HIP(hipGetLastError());
}

// The components of b_0 .. b_{m-1} along u_0 .. u_k (W = k + 1 columns), predicted through the recorded tridiagonal from the known
// coefficient vectors of the two seed inputs (one workgroup).  d_j = C_j / rho_j: the input a_j / rho_j WITHOUT its own O(1) entry.
//   alpha_k = e_0 - 2 Re C_k[k-1] - d_k^H T d_k
//   p_0 = T d_k - e_0 d_k - rho_k d_{k-1}, row k += alpha_k - e_0      (the O(1) self entries cancel exactly in beta_{k-1} = rho_k)
//   p_s = (T p_{s-1} - e_s p_{s-1}) / |b_{s-1}| - |b_{s-1}| (s == 1 ? d_k : p_{s-2} / |b_{s-2}|)
//   prA = p_{m-1}[j] / rho_j, prB = p_{m-2}[j] / rho_j: what the sweep multiplies a_j with
__global__ __launch_bounds__(256) void block_predict_kernel(int k, int m, int reals, BlockScalars sc, const double* __restrict__ rho2,
                                                            const double* __restrict__ cpk, double* __restrict__ hist_alpha,
                                                            const double* __restrict__ hist_beta, double* __restrict__ dk,
                                                            double* __restrict__ p, int pstride, double* __restrict__ prA,
                                                            double* __restrict__ prB) {
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int W = k + 1, RW = reals * W;
  const double* ck = cpk + block_row_at(reals, k);
  const double* ck1 = cpk + block_row_at(reals, k - 1);
  const double rk = sqrt(rho2[k]), rk1 = sqrt(rho2[k - 1]);
  const double ik = 1.0 / rk, ik1 = 1.0 / rk1;
  const double e0 = *sc.e[0];
  for (int i = tid; i < RW; i += 256) dk[i] = i < reals * k ? ck[i] * ik : 0.0;
  __syncthreads();
  double qa = 0.0, zero_ = 0.0;
  for (int i = tid; i < reals * k; i += 256) qa = fma(dk[i], block_tri_row(hist_alpha, hist_beta, dk, i, reals, k, hist_alpha[k - 1]), qa);
  block_sum2_all(qa, zero_, red);
  const double ake = -2.0 * ck[reals * (k - 1)] - qa;  // alpha_k - e_0, formed from the eps-sized numbers
  const double alpha_k = e0 + ake;
  if (tid == 0) hist_alpha[k] = alpha_k;
  for (int i = tid; i < RW; i += 256) {
    const double t = block_tri_row(hist_alpha, hist_beta, dk, i, reals, W, alpha_k);
    const double d1 = i < reals * (k - 1) ? ck1[i] * ik1 : 0.0;
    double v = t - e0 * dk[i] - rk * d1;
    if (i == reals * k) v += ake;
    p[i] = v;
  }
  __syncthreads();
  for (int s = 1; s < m; ++s) {
    const double* in = p + (size_t)(s - 1) * pstride;
    const double nin = sqrt(*sc.nsq[s - 1]), inv = 1.0 / nin;
    const double* prev = s == 1 ? dk : p + (size_t)(s - 2) * pstride;
    const double pinv = s == 1 ? 1.0 : 1.0 / sqrt(*sc.nsq[s - 2]);
    const double es = *sc.e[s];
    double* out = p + (size_t)s * pstride;
    for (int i = tid; i < RW; i += 256) {
      const double t = block_tri_row(hist_alpha, hist_beta, in, i, reals, W, alpha_k);
      out[i] = (t - es * in[i]) * inv - nin * (prev[i] * pinv);
    }
    __syncthreads();
  }
  for (int i = tid; i < RW; i += 256) {
    const double ir = 1.0 / sqrt(rho2[i / reals]);
    prA[i] = p[(size_t)(m - 1) * pstride + i] * ir;
    prB[i] = m >= 2 ? p[(size_t)(m - 2) * pstride + i] * ir : 0.0;
  }
}
void launch_block_predict(int k, int m, int reals, const BlockScalars& sc, const double* rho2, const double* cpk, double* hist_alpha,
                          const double* hist_beta, double* dk, double* p, int pstride, double* prA, double* prB, hipStream_t s) {
  hipLaunchKernelGGL(block_predict_kernel, dim3(1), dim3(256), 0, s, k, m, reals, sc, rho2, cpk, hist_alpha, hist_beta, dk, p, pstride, prA,
                     prB);
  LL_HIP(hipGetLastError());
}

// wave_sum_transposed<8> (dev_helpers.hpp) without the LDS crossbar and with fewer instructions: the exchanges across 32 and 16
// lanes are gfx950's v_permlane32_swap / v_permlane16_swap (the upper rows of x change places with the lower rows of y: x + y is
// then the sum of x in the lower rows and of y in the upper rows), those inside a row of 16 are DPP moves.  The trips of the sweep
// of eight are bound by their instruction count, and 20 shuffle-adds through ds_bpermute with their selects were half of it
// (2.2 TB/s with them, 5.3 TB/s without: DESIGN_EXPERIMENTS E23).  On return a[0] of lane L is the full sum of accumulator L / 8, in a fixed order.
template <int CTRL> __device__ __forceinline__ double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void swap_add32(double& x, double y) {
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  x = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap_add16(double& x, double y) {
  const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  x = __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void wave_sum_transposed8(double (&a)[8], int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) swap_add32(a[i], a[i + 4]);
#pragma unroll
  for (int i = 0; i < 2; ++i) swap_add16(a[i], a[i + 2]);
  const bool upper = (lane & 8) != 0;
  const double keep = upper ? a[1] : a[0], send = upper ? a[0] : a[1];
  double v = keep + dpp_move<0x128>(send);  // row_ror:8: lane ^ 8
  v += dpp_move<0x141>(v);                  // row_half_mirror: lane i of eight <-> 7 - i
  v += dpp_move<0x4e>(v);                   // quad_perm [2, 3, 0, 1]: lane ^ 2
  v += dpp_move<0xb1>(v);                   // quad_perm [1, 0, 3, 2]: lane ^ 1
  a[0] = v;
}

// The same trip for EIGHT new vectors, two pieces per lane, REAL double only (the complex sweep of eight needs 264 registers — one
// wave per SIMD — and complex passes keep blocks of four: LoopState::enqueue_block_f64).  The compensations first; then the column sets in two halves of four, the
// 4 NV sums of a half in ONE transposing reduction (4 NV - 1 + log2(64 / (4 NV)) shuffle-adds against 6 x 4 for a reduction per set:
// with two pieces per lane a trip has half the elements to spread them over) — all eight at once do not fit the registers beside the
// strips.  Accumulator v * 4 + i of a half ends up in lanes 64 / (4 NV) * (v * 4 + i) ..
template <typename T, int NV, int PC>
__device__ __forceinline__ void block_trip_compute8(const T (&ur)[NV][strip<T, PC>::EPT], int nv, const T (&b)[8][strip<T, PC>::EPT],
                                                    T (&cA)[strip<T, PC>::EPT], T (&cB)[strip<T, PC>::EPT],
                                                    const double* __restrict__ prAc, const double* __restrict__ prBc, double* mine,
                                                    int setstride, int lane) {
  constexpr int EPT = strip<T, PC>::EPT;
  constexpr int H = 4, NF = H * NV, LPF = 64 / NF;
  static_assert(!scalar_traits<T>::is_complex && NF == 8, "the sweep of eight: real double, two stored vectors per trip");
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int vv = v < nv ? v : nv - 1;
    const bool real = v < nv;  // (uniform: scalar selects)
    const double xa = ld_const(prAc, vv), xb = ld_const(prBc, vv);
    const double ca = real ? xa : 0.0, cb = real ? xb : 0.0;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      fnma_acc(cA[e], ca, ur[v][e]);
      fnma_acc(cB[e], cb, ur[v][e]);
    }
  }
  const int f = lane / LPF, fv = f / H, fi = f % H;
#pragma unroll
  for (int h = 0; h < 8 / H; ++h) {
    double fs[NF];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
#pragma unroll
      for (int i = 0; i < H; ++i) {
        double sm = 0.0;
#pragma unroll
        for (int e = 0; e < EPT; ++e) cfma_acc(sm, ur[v][e], b[h * H + i][e]);
        fs[v * H + i] = sm;
      }
    }
    wave_sum_transposed8(fs, lane);
    if ((lane & (LPF - 1)) == 0 && fv < nv) mine[(h * H + fi) * setstride + fv] += fs[0];
    __builtin_amdgcn_sched_barrier(0);  // (the halves one after the other: their accumulators share registers)
  }
}

// One trip of the block sweep: NV stored strips; M measured column sets (against the RAW new vectors), two compensations.
// nv <= NV of the strips are real (a prefix), like in pair_trip_compute.
template <typename T, int NV, int PC, int M>
__device__ __forceinline__ void block_trip_compute(const T (&ur)[NV][strip<T, PC>::EPT], int nv, const T (&b)[M][strip<T, PC>::EPT],
                                                   T (&cA)[strip<T, PC>::EPT], T (&cB)[strip<T, PC>::EPT],
                                                   const double* __restrict__ prAc, const double* __restrict__ prBc, double* mine,
                                                   int setstride, int lane) {
  constexpr int EPT = strip<T, PC>::EPT;
  if constexpr (M == 8) {
    block_trip_compute8<T, NV, PC>(ur, nv, b, cA, cB, prAc, prBc, mine, setstride, lane);
    return;
  }
  double sre[M][NV], sim[M][NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    acc_t<T> ca, cb;
    const int vv = v < nv ? v : nv - 1;
    const bool real = v < nv;  // (uniform: scalar selects)
    if constexpr (scalar_traits<T>::is_complex) {
      const double xa = ld_const(prAc, 2 * vv), ya = ld_const(prAc, 2 * vv + 1), xb = ld_const(prBc, 2 * vv), yb = ld_const(prBc, 2 * vv + 1);
      ca = zc{real ? xa : 0.0, real ? ya : 0.0};
      cb = zc{real ? xb : 0.0, real ? yb : 0.0};
    } else {
      const double xa = ld_const(prAc, vv), xb = ld_const(prBc, vv);
      ca = real ? xa : 0.0;
      cb = real ? xb : 0.0;
    }
    acc_t<T> sm[M];
#pragma unroll
    for (int i = 0; i < M; ++i) sm[i] = zero<acc_t<T>>();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      fnma_acc(cA[e], ca, ur[v][e]);
      if constexpr (M >= 2) fnma_acc(cB[e], cb, ur[v][e]);
#pragma unroll
      for (int i = 0; i < M; ++i) cfma_acc(sm[i], ur[v][e], b[i][e]);
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if constexpr (scalar_traits<T>::is_complex) {
        sre[i][v] = sm[i].re;
        sim[i][v] = sm[i].im;
      } else {
        sre[i][v] = sm[i];
        sim[i][v] = 0.0;
      }
    }
  }
  constexpr int LPI = 64 / NV;  // lanes that end up holding the same sum
#pragma unroll
  for (int i = 0; i < M; ++i) {
    wave_sum_transposed<NV>(sre[i], lane);
    if constexpr (scalar_traits<T>::is_complex) wave_sum_transposed<NV>(sim[i], lane);
  }
  if ((lane & (LPI - 1)) == 0 && lane / LPI < nv) {
    const int v = lane / LPI;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if constexpr (scalar_traits<T>::is_complex) {
        mine[i * setstride + 2 * v] += sre[i][0];
        mine[i * setstride + 2 * v + 1] += sim[i][0];
      } else {
        mine[i * setstride + v] += sre[i][0];
      }
    }
  }
}

// Partial columns per workgroup: [<a_j, b_s>: R * W per s, s-major][Gram: <v_s', v_s>, s' < s (R each, s-major)][|v_s|^2: M], with
// v_s the new vectors AS WRITTEN (the last two compensated).  The strip walk, the pointer table and the software pipeline are
// pair_sweep_pipe_kernel's (gs_pair.hip); there are no late updates: nothing stored is written.  A sweep over more stored
// vectors than one workgroup's LDS holds columns for is split into launches over consecutive ranges [col0, col0 + Wl) of them;
// between launches the two partly compensated vectors travel through bv.part (the raw ones stay in their slots until the last
// launch: every launch measures against the raw vectors).
template <typename T, int PC, int M, int JB>
__global__ __launch_bounds__(kBlock) void block_sweep_kernel(int64_t n, const T* const* __restrict__ vtab, int W, int col0, int Wl, int flags,
                                                             BlockVecs<T> bv, const double* __restrict__ prA,
                                                             const double* __restrict__ prB, double* __restrict__ partials) {
  constexpr int EPT = strip<T, PC>::EPT;
  constexpr int ELEMS = strip<T, PC>::ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  constexpr int NG = R * M * (M - 1) / 2 + M;
  const bool first = (flags & kPairFirst) != 0, last = (flags & kPairLast) != 0;
  const int ncols = M * R * W + NG;
  const int lcols = M * R * Wl + (last ? NG : 0);
  extern __shared__ double lds[];  // [4 waves][lcols]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < 4 * lcols; i += kBlock) lds[i] = 0.0;
  __syncthreads();
  double* mine = lds + (size_t)wave * lcols;
  double* tail = mine + M * R * Wl;
  const T* const* tab = vtab + col0;
  const double *prAc = prA + R * col0, *prBc = prB + R * col0;
  const int ntrips = (Wl + JB - 1) / JB;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  T* const outA = last ? bv.b[M - 1] : bv.part[0];
  T* const outB = last ? bv.b[M >= 2 ? M - 2 : 0] : bv.part[1];

  auto do_strip = [&](auto full_c, const int64_t base) {
    constexpr bool FULL = decltype(full_c)::value;
    T b[M][EPT], cA[EPT], cB[EPT];
#pragma unroll
    for (int i = 0; i < M; ++i) load_lstrip_u<T, PC, FULL>(bv.b[i], base, n, b[i]);
    auto issue = [&](T (&buf)[JB][EPT], int t) {
      const T* ptr[JB];
#pragma unroll
      for (int v = 0; v < JB; ++v) ptr[v] = ld_const_ptr<T>(tab, min(JB * t + v, Wl - 1));  // uniform; beyond the end: the last stored vector again
#pragma unroll
      for (int v = 0; v < JB; ++v) load_lstrip_u<T, PC, FULL>(ptr[v], base, n, buf[v]);
    };
    T ua[JB][EPT], ub[JB][EPT];
    if (ntrips > 0) {
      __builtin_amdgcn_sched_barrier(0);
      issue(ua, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (first) {
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        cA[e] = b[M - 1][e];
        cB[e] = b[M >= 2 ? M - 2 : 0][e];
      }
    } else {  // (uniform) the two compensated vectors as the launch before left them
      load_lstrip_u<T, PC, FULL>(bv.part[0], base, n, cA);
      if constexpr (M >= 2) load_lstrip_u<T, PC, FULL>(bv.part[1], base, n, cB);
    }
    for (int t = 0; t < ntrips; t += 2) {
      __builtin_amdgcn_sched_barrier(0);
      issue(ub, t + 1);
      __builtin_amdgcn_sched_barrier(0);
      block_trip_compute<T, JB, PC, M>(ua, min(JB, Wl - JB * t), b, cA, cB, prAc + R * JB * t, prBc + R * JB * t, mine + R * JB * t, R * Wl, lane);
      if (t + 1 >= ntrips) break;
      __builtin_amdgcn_sched_barrier(0);
      issue(ua, t + 2);
      __builtin_amdgcn_sched_barrier(0);
      block_trip_compute<T, JB, PC, M>(ub, min(JB, Wl - JB * (t + 1)), b, cA, cB, prAc + R * JB * (t + 1), prBc + R * JB * (t + 1),
                                       mine + R * JB * (t + 1), R * Wl, lane);
    }
    store_lstrip_u<T, PC, FULL>(outA, base, n, cA);
    if constexpr (M >= 2) store_lstrip_u<T, PC, FULL>(outB, base, n, cB);
    if (!last) return;
    // the Gram matrix of the new vectors as written
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      b[M - 1][e] = cA[e];
      if constexpr (M >= 2) b[M - 2][e] = cB[e];
    }
    if constexpr (M == 8) {
      // 28 products and 8 norms per strip (real double only): two transposing reductions of 16 and four wave sums instead of 36 wave
      // sums.  The products (pair (i, ip) at i (i - 1) / 2 + ip) 0 .. 15; then the products 16 .. 27 followed by |v_0|^2 .. |v_3|^2
      // (one of 32 does not fit the registers beside the eight strips); |v_4|^2 .. |v_7|^2 by themselves.
      constexpr int NP = M * (M - 1) / 2;
      static_assert(NP + 4 == 32 && !scalar_traits<T>::is_complex, "the Gram triangle of eight and four norms fill two reductions of 16");
      const int f = lane >> 2;  // the accumulator of a reduction of 16 whose sum this lane holds
      auto half = [&](auto first_c) {
        constexpr int FIRST = decltype(first_c)::value;
        double ga[16];
        int a = 0;
#pragma unroll
        for (int i = 1; i < M; ++i) {
#pragma unroll
          for (int ip = 0; ip < i; ++ip) {
            if (a >= FIRST && a < FIRST + 16) {
              double g = 0.0;
#pragma unroll
              for (int e = 0; e < EPT; ++e) cfma_acc(g, b[ip][e], b[i][e]);
              ga[a - FIRST] = g;
            }
            ++a;
          }
        }
        if constexpr (FIRST == 16) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            double n0 = 0.0;
#pragma unroll
            for (int e = 0; e < EPT; ++e) n0 += abs2(b[i][e]);
            ga[NP - 16 + i] = n0;
          }
        }
        wave_sum_transposed<16>(ga, lane);
        if ((lane & 3) == 0) tail[FIRST + f] += ga[0];  // (28 .. 31: |v_0|^2 .. |v_3|^2, which follow the products)
        if constexpr (FIRST == 16) {
#pragma unroll
          for (int i = 4; i < M; ++i) {
            double nn = 0.0;
#pragma unroll
            for (int e = 0; e < EPT; ++e) nn += abs2(b[i][e]);
            nn = wave_sum(nn);
            if (lane == 0) tail[NP + i] += nn;
          }
        }
      };
      __builtin_amdgcn_sched_barrier(0);
      half(std::integral_constant<int, 0>{});
      __builtin_amdgcn_sched_barrier(0);  // (the halves one after the other: their accumulators share registers)
      half(std::integral_constant<int, 16>{});
      return;
    }
    int at = 0;
#pragma unroll
    for (int i = 1; i < M; ++i) {
#pragma unroll
      for (int ip = 0; ip < i; ++ip) {
        acc_t<T> g = zero<acc_t<T>>();
#pragma unroll
        for (int e = 0; e < EPT; ++e) cfma_acc(g, b[ip][e], b[i][e]);
        const acc_t<T> gs = wave_sum(g);
        if (lane == 0) {
          if constexpr (scalar_traits<T>::is_complex) {
            tail[at] += gs.re;
            tail[at + 1] += gs.im;
          } else {
            tail[at] += gs;
          }
        }
        at += R;
      }
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
      double nn = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) nn += abs2(b[i][e]);
      nn = wave_sum(nn);
      if (lane == 0) tail[at + i] += nn;
    }
  };
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t base = sidx * ELEMS;
    if (base + ELEMS <= n) do_strip(std::true_type{}, base);
    else do_strip(std::false_type{}, base);
  }
  __syncthreads();
  // this launch's columns into the sweep's layout
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < lcols; i += kBlock) {
    const double v = (lds[i] + lds[lcols + i]) + (lds[2 * lcols + i] + lds[3 * lcols + i]);
    int g;
    if (i < M * R * Wl) {
      const int set = i / (R * Wl);
      g = set * R * W + R * col0 + (i - set * R * Wl);
    } else {
      g = M * R * W + (i - M * R * Wl);
    }
    out[g] = v;
  }
}
constexpr int kBlockJB = 2;  // stored vectors per trip (two trips resident, like kPipeJB)
template <typename T, int PC, int M>
static void block_sweep_launch(int grid, size_t lds_bytes, hipStream_t s, int64_t n, const T* const* vtab, int W, int col0, int Wl, int flags,
                               const BlockVecs<T>& bv, const double* prA, const double* prB, double* partials) {
  hipLaunchKernelGGL((block_sweep_kernel<T, PC, M, kBlockJB>), dim3(grid), dim3(kBlock), lds_bytes, s, n, vtab, W, col0, Wl, flags, bv, prA, prB,
                     partials);
}
template <typename T>
int launch_block_sweep(int64_t n, const T* const* vtab, int W, int m, const BlockVecs<T>& bv, const double* prA, const double* prB,
                       double* partials, int pieces, int per_launch, hipStream_t s) {
  constexpr int R = scalar_traits<T>::reals;
  LL_REQUIRE(m == 1 || m == 2 || m == 4 || m == 8, "internal: block sweep of 1, 2, 4 or 8 iterations");
  const int64_t strips16k = (n * (int64_t)sizeof(T) + 16383) / 16384;
  int pc = strips16k >= kLaggedFullStrips ? 4 : 2;
  if (pieces == 2 || pieces == 4) pc = pieces;
  // Eight new strips of four pieces are 64 VGPRs more than the 228 of <double, 4, 4, 2>: beyond the 256 that two waves per SIMD
  // leave.  Eight always run with two pieces per lane (8 KiB strips; profiles/block_gs_registers.txt).
  if (m == 8) pc = 2;
  const int grid = pc == 4 ? strip_grid(n, strip<T, 4>::ELEMS) : strip_grid(n, strip<T, 2>::ELEMS);
  const int ng = R * m * (m - 1) / 2 + m;
  per_launch = std::max(1, std::min(per_launch, block_sweep_max_vecs<T>(m)));
  for (int col0 = 0; col0 < W; col0 += per_launch) {
    const int Wl = std::min(per_launch, W - col0);
    const int flags = (col0 == 0 ? kPairFirst : 0) | (col0 + Wl == W ? kPairLast : 0);
    const size_t lds_bytes = (size_t)4 * (size_t)(m * R * Wl + ((flags & kPairLast) ? ng : 0)) * sizeof(double);
#define LL_BLOCK_SWEEP(PC_, M_) block_sweep_launch<T, PC_, M_>(grid, lds_bytes, s, n, vtab, W, col0, Wl, flags, bv, prA, prB, partials)
    if (pc == 4) {
      if (m == 4) LL_BLOCK_SWEEP(4, 4);
      else if (m == 2) LL_BLOCK_SWEEP(4, 2);
      else LL_BLOCK_SWEEP(4, 1);
    } else {
      if (m == 8) {
        if constexpr (scalar_traits<T>::is_complex) LL_REQUIRE(false, "internal: the block sweep of eight is built for real double only");
        else LL_BLOCK_SWEEP(2, 8);
      } else if (m == 4) LL_BLOCK_SWEEP(2, 4);
      else if (m == 2) LL_BLOCK_SWEEP(2, 2);
      else LL_BLOCK_SWEEP(2, 1);
    }
#undef LL_BLOCK_SWEEP
    LL_HIP(hipGetLastError());
  }
  return grid;
}

// The fold of a block (one workgroup), new vector by new vector (s = 0 .. m-1, index j = k + 1 + s).  cols: the folded columns of
// the sweep.  For every new vector:
//   raw coefficients (what the operator saw): M[l, s] / rho_l for the stored columns (C^H c is of second order), the exact recursion
//     c[l] = (M[l, s] - C_l^H c[:l]) / rho_l for the two seeds l = k - 1, k
//   row j of C: the raw ones, minus p_s for the two compensated vectors (by linearity: the vector as written); the in-block
//     predecessors by the exact recursion on the Gram matrix
//   rho_j^2 = |v_s|^2 - |C_j|^2, beta_{j-1} = rho_j
//   alpha_{j-1} (s >= 1), from e_s and the RAW coefficients of the previous new vector:
//     e_s |b_{s-1}|^2 = rho^2 alpha + 2 rho^2 Re c[j-2] + c^H T c
//   the gate value: the largest coefficient of the vector, raw or as written, relative to the vector
// and the four scalars of iteration j (alpha_{j-1}, rho_j^2, |v_s|^2, rho_j^2) in its host slot.
__global__ __launch_bounds__(256) void block_fold_kernel(const double* __restrict__ cols, int k, int m, int reals, BlockScalars sc,
                                                         const double* __restrict__ p, int pstride, double* __restrict__ rho2,
                                                         double* __restrict__ cpk, double* __restrict__ hist_alpha,
                                                         double* __restrict__ hist_beta, double* __restrict__ raw0,
                                                         double* __restrict__ raw1, BlockHost host) {
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int W = k + 1, RW = reals * W;
  const double* tail = cols + (size_t)m * RW;
  const double* diag = tail + reals * m * (m - 1) / 2;
  for (int s = 0; s < m; ++s) {
    const int j = k + 1 + s;
    double* raw = (s & 1) ? raw1 : raw0;           // raw coefficients of this vector, reals * j
    const double* rawp = (s & 1) ? raw0 : raw1;    // ... of the previous new vector, reals * (j - 1)
    double* row = cpk + block_row_at(reals, j);
    const double* ms = cols + (size_t)s * RW;
    const double* ps = p + (size_t)s * pstride;
    const bool comp = s == m - 1 || s == m - 2;
    const double nn = diag[s], nraw2 = *sc.nsq[s];
    for (int i = tid; i < RW; i += 256) raw[i] = ms[i] / sqrt(rho2[i / reals]);
    __syncthreads();
    for (int col = k - 1; col <= k; ++col) {  // the two seeds, in order
      const double* cr = cpk + block_row_at(reals, col);
      double dre = 0.0, dim = 0.0;
      for (int l = tid; l < col; l += 256) {
        if (reals == 2) {
          const double ar = cr[2 * l], ai = cr[2 * l + 1], br = raw[2 * l], bi = raw[2 * l + 1];
          dre += ar * br + ai * bi;
          dim += ar * bi - ai * br;
        } else {
          dre += cr[l] * raw[l];
        }
      }
      block_sum2_all(dre, dim, red);
      if (tid == 0) {
        const double ir = 1.0 / sqrt(rho2[col]);
        raw[reals * col] = (ms[reals * col] - dre) * ir;
        if (reals == 2) raw[2 * col + 1] = (ms[2 * col + 1] - dim) * ir;
      }
      __syncthreads();
    }
    double mxr = 0.0, mxc = 0.0, cc = 0.0;
    for (int i = tid; i < RW; i += 256) {
      const double v = comp ? raw[i] - ps[i] : raw[i];
      row[i] = v;
      mxr = fmax(mxr, fabs(raw[i]));
      mxc = fmax(mxc, fabs(v));
      cc = fma(v, v, cc);
    }
    __syncthreads();
    for (int sp = 0; sp < s; ++sp) {  // in-block predecessors, in order
      const int col = k + 1 + sp;
      const double* cr = cpk + block_row_at(reals, col);
      double dre = 0.0, dim = 0.0;
      for (int l = tid; l < col; l += 256) {
        if (reals == 2) {
          const double ar = cr[2 * l], ai = cr[2 * l + 1], br = row[2 * l], bi = row[2 * l + 1];
          dre += ar * br + ai * bi;
          dim += ar * bi - ai * br;
        } else {
          dre += cr[l] * row[l];
        }
      }
      block_sum2_all(dre, dim, red);
      const double* g = tail + reals * (s * (s - 1) / 2 + sp);
      const double ir = 1.0 / sqrt(rho2[col]);
      const double vre = (g[0] - dre) * ir, vim = reals == 2 ? (g[1] - dim) * ir : 0.0;
      if (tid == 0) {
        row[reals * col] = vre;
        raw[reals * col] = vre;
        if (reals == 2) {
          row[2 * col + 1] = vim;
          raw[2 * col + 1] = vim;
        }
        const double a = fmax(fabs(vre), fabs(vim));
        mxr = fmax(mxr, a);
        mxc = fmax(mxc, a);
        cc += vre * vre + vim * vim;
      }
      __syncthreads();
    }
    double zero_ = 0.0;
    block_sum2_all(cc, zero_, red);
    block_max2_all(mxr, mxc, red);
    double r2 = nn - cc;
    r2 = r2 > 0.0 ? r2 : 0.0;
    // alpha of the previous new vector (index j - 1), from this step's e and that vector's raw coefficients
    double alpha_pub;
    if (s == 0) {
      alpha_pub = hist_alpha[k];
    } else {
      double qb = 0.0;
      for (int i = tid; i < reals * (j - 1); i += 256)
        qb = fma(rawp[i], block_tri_row(hist_alpha, hist_beta, rawp, i, reals, j - 1, hist_alpha[j - 2]), qb);
      block_sum2_all(qb, zero_, red);
      const double rp2 = rho2[j - 1];
      alpha_pub = rp2 > 0.0 ? (*sc.e[s] * *sc.nsq[s - 1] - 2.0 * rp2 * rawp[reals * (j - 2)] - qb) / rp2 : 0.0;
    }
    __syncthreads();  // (everything above has read rho2 / hist_* as the previous step left them)
    if (tid == 0) {
      rho2[j] = r2;
      hist_beta[j - 1] = sqrt(r2);
      if (s > 0) hist_alpha[j - 1] = alpha_pub;
      double gate = 1.0;
      if (nn > 0.0 && nraw2 > 0.0) gate = fmax(mxr / sqrt(nraw2), mxc / sqrt(nn));
      host.slot[s][0] = alpha_pub;
      host.slot[s][1] = r2;
      host.slot[s][2] = nn;
      host.slot[s][3] = r2;
      *host.gate[s] = gate;
    }
    __syncthreads();
  }
}
void launch_block_fold(const double* cols, int k, int m, int reals, const BlockScalars& sc, const double* p, int pstride, double* rho2,
                       double* cpk, double* hist_alpha, double* hist_beta, double* raw0, double* raw1, const BlockHost& host, hipStream_t s,
                       hipEvent_t stop) {
  LL_LAUNCH_STOP(stop, block_fold_kernel, dim3(1), dim3(256), 0, s, cols, k, m, reals, sc, p, pstride, rho2, cpk, hist_alpha, hist_beta, raw0,
                 raw1, host);
  LL_HIP(hipGetLastError());
}

template int launch_block_sweep<double>(int64_t, const double* const*, int, int, const BlockVecs<double>&, const double*, const double*,
                                        double*, int, int, hipStream_t);
template int launch_block_sweep<zc>(int64_t, const zc* const*, int, int, const BlockVecs<zc>&, const double*, const double*, double*, int, int,
                                    hipStream_t);

}  // namespace ll
