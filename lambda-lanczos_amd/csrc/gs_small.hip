// The SMALL-VECTOR geometry of all three Gram-Schmidt forms (vectors below Tuning::blas_small_bytes, 4 MiB): multi-dot and
// multi-axpy (two sweeps), the one-sweep (lagged) form and the pair form.  The streaming geometry of the same forms and the
// launchers that choose between the two are in kernels.hip (mdot, maxpy, lagged) and gs_pair.hip (pair).
//
// Reference rows:
//   a4        mdot_small (prologue)    three-term update (LL:251-257, EX:112-118)
//   a5/a6     mdot_small + maxpy_small Gram-Schmidt against locked + Krylov vectors (LA:132-144 at LL:259-260, EX:121)
//   a7        maxpy_small (epilogue)   ||w||^2 (LA:56-60 at LL:262, EX:145)
#include <algorithm>

#include "gs_strips.hpp"

namespace ll {

// ================================================================= small-vector Gram-Schmidt kernels (vectors < 4 MiB)
// With few strips the streaming kernels are a latency / instruction chain: ONE wave walks all k basis vectors of
// its strip (n = 1e4, k = 100: 28 us for 8 MB that the chip reads in under 7 us, tools/small_strip_probe.hip).  Here a
// workgroup is four waves on the SAME strip of 64 lanes x 16 B (n = 1e4 doubles: 79 workgroups instead of 5); the trips
// of kSmallJB basis vectors are dealt round-robin to the waves, so each wave walks a quarter of the basis:
//   multi-dot : every basis vector belongs to exactly one wave -> no cross-wave sums; the kSmallJB (x2) per-lane
//               partial products of a trip are transposed through a per-wave LDS tile and each column is summed by
//               four lanes (16 reads + 2 quad shuffles instead of 6 dependent shuffle steps per vector);
//   multi-axpy: every wave accumulates its share of sum_j h_j u_j, wave 0 adds the four shares in a fixed order,
//               updates w and accumulates ||w||^2.
// All sums have a fixed order: bit-reproducible like the streaming kernels (the two geometries differ from each other
// in the last bits, each is deterministic).
constexpr int kSmallJB = 8;
constexpr int kSmallTileRow = 65;  // doubles per row of the transpose tile (64 lanes + 1: conflict-free columns)

// LDS traffic between the lanes of ONE wave: the hardware executes a wave's LDS instructions in order; these keep the
// compiler from moving accesses across the hand-over point.
__device__ __forceinline__ void wave_lds_handover() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ __launch_bounds__(kBlock) void mdot_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs, ThreeTerm<T> tt,
                                                            NormRefs pred, int predicated, double* __restrict__ partials,
                                                            int ncols) {
  constexpr int EPT = strip<T, 1>::EPT;
  constexpr int ELEMS = strip<T, 1>::WAVE_ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  extern __shared__ double lds[];   // [ncols] column sums of the workgroup, then one [16][65] transpose tile per wave
  if (predicated && !second_pass_due(pred)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cols = lds;
  double* tile = lds + ((ncols + 15) & ~15) + wave * (16 * kSmallTileRow);
  for (int i = tid; i < ncols; i += kBlock) cols[i] = 0.0;
  __syncthreads();

  double alpha = 0.0, beta = 0.0;
  const bool do_tt = tt.u_cur != nullptr;
  if (do_tt) {
    if (tt.alpha_partials) {  // deferred alpha (ThreeTerm)
      __shared__ double fold_scratch[5];
      alpha = fold_partials_all(tt.alpha_partials, tt.alpha_nparts, fold_scratch);
      if (blockIdx.x == 0 && tid == 0) *tt.alpha_out = alpha;
    } else {
      alpha = *tt.alpha;
    }
    if (tt.u_prev) beta = sqrt(final_norm2(tt.prev));
  }
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {  // same trip count for every wave of the workgroup
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    T wr[EPT];
    load_strip<T, 1>(w, i0, n, wr);
    if (do_tt) {  // every wave forms the same three-term strip; wave 0 stores it once all four have read w
      T uc[EPT];
      load_strip<T, 1>(tt.u_cur, i0, n, uc);
      if (tt.u_prev) {
        T up[EPT];
        load_strip<T, 1>(tt.u_prev, i0, n, up);
#pragma unroll
        for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, up[e])), rmul(alpha, uc[e]));
      } else {
#pragma unroll
        for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, uc[e]));
      }
      __syncthreads();
      if (wave == 0) store_strip<T, 1>(w, i0, n, wr);
    }
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_strip<T, 1>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b) {
          acc_t<T> acc = zero<acc_t<T>>();
          if (b < nv) {
#pragma unroll
            for (int e = 0; e < EPT; ++e) cfma_acc(acc, ur[b][e], wr[e]);
          }
          if constexpr (scalar_traits<T>::is_complex) {
            tile[(2 * b) * kSmallTileRow + lane] = acc.re;
            tile[(2 * b + 1) * kSmallTileRow + lane] = acc.im;
          } else {
            tile[b * kSmallTileRow + lane] = acc;
          }
        }
        wave_lds_handover();
        // column i of the tile (16 slots, NA of them used) is summed by the four lanes 4i .. 4i+3, 16 entries each
        const int i = lane >> 2, q = lane & 3;
        double sum = 0.0;
        if (i < nv * R) {
          const double* row = tile + i * kSmallTileRow + q * 16;
#pragma unroll
          for (int t = 0; t < 16; ++t) sum += row[t];
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if (q == 0 && i < nv * R) cols[col0 + R * j + i] += sum;  // this column belongs to this wave alone
        wave_lds_handover();
      }
      col0 += R * cnt;
    }
    if (wave == 0) {
      double nn = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) nn += abs2(wr[e]);
      nn = wave_sum(nn);
      if (lane == 0) cols[ncols - 1] += nn;
    }
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock) out[i] = cols[i];
}

// dst[j] = sum_b partials[b * ncols + j], j < ncols, formed by the WHOLE workgroup in exactly the order of
// reduce_cols_kernel (16 columns x 16 row lanes per pass, four chains per lane, rows folded 0..15): the fold of the
// multi-dot's partials without its launch, for grids small enough that every workgroup can afford to redo it.
__device__ __forceinline__ void fold_cols_into_lds(const double* __restrict__ partials, int nparts, int ncols, double* dst) {
  __shared__ double sm[16][17];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  for (int j0 = 0; j0 < ncols; j0 += 16) {
    const int j = j0 + cx;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (j < ncols) {
      int b = ry;
      for (; b + 48 < nparts; b += 64) {
        a0 += partials[(size_t)b * ncols + j];
        a1 += partials[(size_t)(b + 16) * ncols + j];
        a2 += partials[(size_t)(b + 32) * ncols + j];
        a3 += partials[(size_t)(b + 48) * ncols + j];
      }
      for (; b < nparts; b += 16) a0 += partials[(size_t)b * ncols + j];
    }
    __syncthreads();  // the previous pass has been read out
    sm[ry][cx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (ry == 0 && j < ncols) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) t += sm[r][cx];
      dst[j] = t;
    }
  }
  __syncthreads();
}

// FOLD: h is not given; the kernel folds the multi-dot's partials `mp` ([mparts][R*nb + 1]: coefficients, then ||w||^2)
// itself — every workgroup, same order — and workgroup 0 stores the coefficients to h_out and ||w||^2 to *c0_out.
template <typename T, bool FOLD>
__global__ __launch_bounds__(kBlock) void maxpy_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs,
                                                             const double* __restrict__ h, int nb, NormRefs pred,
                                                             int predicated, double* __restrict__ partials,
                                                             const double* __restrict__ mp, int mparts,
                                                             double* __restrict__ h_out, double* __restrict__ c0_out) {
  constexpr int EPT = strip<T, 1>::EPT;
  constexpr int ELEMS = strip<T, 1>::WAVE_ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  extern __shared__ double lds[];  // [R*nb (+1)] coefficients, then the four waves' shares [4][64][EPT*R]
  if (predicated && !second_pass_due(pred)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if constexpr (FOLD) {
    fold_cols_into_lds(mp, mparts, R * nb + 1, lds);
    if (blockIdx.x == 0) {
      for (int i = tid; i < R * nb; i += kBlock) h_out[i] = lds[i];
      if (tid == 0 && c0_out) *c0_out = lds[R * nb];
    }
  } else {
    for (int i = tid; i < R * nb; i += kBlock) lds[i] = h[i];
  }
  double* share = lds + ((R * nb + 1 + 15) & ~15);
  __syncthreads();
  double nn = 0.0;
  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    acc_t<T> delta[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) delta[e] = zero<acc_t<T>>();
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_strip<T, 1>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) {
            const double* hc = lds + col0 + R * (j + b);
            acc_t<T> hj;
            if constexpr (scalar_traits<T>::is_complex) hj = zc{hc[0], hc[1]};
            else hj = hc[0];
#pragma unroll
            for (int e = 0; e < EPT; ++e) fma_acc(delta[e], hj, to_acc(ur[b][e]));
          }
      }
      col0 += R * cnt;
    }
    double* mine = share + ((size_t)wave * 64 + lane) * (EPT * R);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if constexpr (scalar_traits<T>::is_complex) {
        mine[2 * e] = delta[e].re;
        mine[2 * e + 1] = delta[e].im;
      } else {
        mine[e] = delta[e];
      }
    }
    __syncthreads();
    if (wave == 0) {
      T wr[EPT];
      load_strip<T, 1>(w, i0, n, wr);
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        acc_t<T> tot;
        const double* s0 = share + ((size_t)0 * 64 + lane) * (EPT * R);
        const double* s1 = share + ((size_t)1 * 64 + lane) * (EPT * R);
        const double* s2 = share + ((size_t)2 * 64 + lane) * (EPT * R);
        const double* s3 = share + ((size_t)3 * 64 + lane) * (EPT * R);
        if constexpr (scalar_traits<T>::is_complex)
          tot = zc{(s0[2 * e] + s1[2 * e]) + (s2[2 * e] + s3[2 * e]), (s0[2 * e + 1] + s1[2 * e + 1]) + (s2[2 * e + 1] + s3[2 * e + 1])};
        else
          tot = (s0[e] + s1[e]) + (s2[e] + s3[e]);
        wr[e] = narrow<T>(sub(to_acc(wr[e]), tot));
      }
      store_strip<T, 1>(w, i0, n, wr);
#pragma unroll
      for (int e = 0; e < EPT; ++e) nn += abs2(wr[e]);
    }
    __syncthreads();  // the shares are rewritten by the next strip
  }
  if (wave == 0) {
    const double tot = wave_sum(nn);
    if (lane == 0) partials[blockIdx.x] = tot;
  }
}

static int small_lagged_lds_doubles(int ncols, int ept_times_reals) {
  return ((ncols + 15) & ~15) + 4 * 16 * kSmallTileRow + 2 * kBlock * ept_times_reals;
}
// One-sweep Gram-Schmidt (lagged_kernel's algebra, see there) in the SMALL-VECTOR geometry: four waves share a strip of
// 64 lanes x 16 B and split the basis between them (trips of kSmallJB vectors dealt round-robin).  Every wave takes the
// coefficients <u_j, wr> of its vectors (LDS-transposed column sums, as in mdot_small_kernel) and accumulates its share
// of sum g_j u_j (late update of u_{k-1}) and of sum d_j u_j (compensation of w); wave 0 adds the four shares in a fixed
// order (as in maxpy_small_kernel), finishes u_{k-1} and w, and takes the last coefficient and ||w||^2.
// Compiled for workgroups of up to 1024 lanes although it is launched with kBlock: the register budget this kernel has always
// been built with (128 VGPRs, 4 waves per SIMD; float spills 2 VGPRs to 12 B of scratch per lane).  With kBlock the compiler
// takes 130 / 131 VGPRs for float / cf: no scratch, but 3 waves per SIMD — which of the two is faster on the small Laplacians
// is not measured yet.
template <typename T>
__global__ __launch_bounds__(1024) void lagged_small_kernel(int64_t n, T* __restrict__ w, BasisSegs<T> segs, int nb,
                                                              Lagged<T> lg, const double* __restrict__ g,
                                                              const double* __restrict__ t, ThreeTerm<T> tt,
                                                              double* __restrict__ partials) {
  constexpr int EPT = strip<T, 1>::EPT;
  constexpr int ELEMS = strip<T, 1>::WAVE_ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = R * (nb + 1) + 1;
  extern __shared__ double lds[];  // [ncols] column sums, one [16][65] tile per wave, the waves' shares of the two updates
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cols = lds;
  double* tile = lds + ((ncols + 15) & ~15) + wave * (16 * kSmallTileRow);
  double* share_u = lds + ((ncols + 15) & ~15) + 4 * (16 * kSmallTileRow);
  double* share_w = share_u + (size_t)kBlock * EPT * R;
  for (int i = tid; i < ncols; i += kBlock) cols[i] = 0.0;
  double alpha;
  if (tt.alpha_partials) {
    __shared__ double fold_scratch[5];
    alpha = fold_partials_all(tt.alpha_partials, tt.alpha_nparts, fold_scratch);
    if (blockIdx.x == 0 && tid == 0) *tt.alpha_out = alpha;  // as measured; lagged_fold_kernel corrects it in place
  } else {
    alpha = *tt.alpha;
  }
  alpha = lagged_alpha(alpha, g[R * (nb - 1)], t[R * (nb + 1)]);
  const double beta = sqrt(*lg.beta2), s = 1.0 / beta;
  const double as = alpha * s;
  acc_t<T> dlast;
  if constexpr (scalar_traits<T>::is_complex) dlast = zc{t[R * nb], t[R * nb + 1]};
  else dlast = t[R * nb];
  __syncthreads();

  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {  // same trip count for every wave of the workgroup
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    T wr[EPT], rr[EPT];
    load_strip<T, 1>(w, i0, n, wr);
    load_strip<T, 1>(lg.r, i0, n, rr);
    if (tt.u_prev) {
      T up[EPT];
      load_strip<T, 1>(tt.u_prev, i0, n, up);
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(sub(wr[e], rmul(beta, up[e])), rmul(alpha, rmul(s, rr[e])));
    } else {
#pragma unroll
      for (int e = 0; e < EPT; ++e) wr[e] = sub(wr[e], rmul(alpha, rmul(s, rr[e])));
    }
    acc_t<T> du[EPT], dw[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      du[e] = zero<acc_t<T>>();
      dw[e] = zero<acc_t<T>>();
    }
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_strip<T, 1>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b) {
          acc_t<T> acc = zero<acc_t<T>>();
          if (b < nv) {
            const double* gc = g + col0 + R * (j + b);
            const double* tc = t + col0 + R * (j + b);
            acc_t<T> gj, dj;
            if constexpr (scalar_traits<T>::is_complex) {
              gj = zc{gc[0], gc[1]};
              dj = zc{fma(-as, gj.re, tc[0]), fma(-as, gj.im, tc[1])};
            } else {
              gj = gc[0];
              dj = fma(-as, gj, tc[0]);
            }
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
              cfma_acc(acc, ur[b][e], wr[e]);
              fma_acc(du[e], gj, to_acc(ur[b][e]));
              fma_acc(dw[e], dj, to_acc(ur[b][e]));
            }
          }
          if constexpr (scalar_traits<T>::is_complex) {
            tile[(2 * b) * kSmallTileRow + lane] = acc.re;
            tile[(2 * b + 1) * kSmallTileRow + lane] = acc.im;
          } else {
            tile[b * kSmallTileRow + lane] = acc;
          }
        }
        wave_lds_handover();
        const int i = lane >> 2, q = lane & 3;
        double sum = 0.0;
        if (i < nv * R) {
          const double* row = tile + i * kSmallTileRow + q * 16;
#pragma unroll
          for (int tt2 = 0; tt2 < 16; ++tt2) sum += row[tt2];
        }
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if (q == 0 && i < nv * R) cols[col0 + R * j + i] += sum;  // this column belongs to this wave alone
        wave_lds_handover();
      }
      col0 += R * cnt;
    }
    double* mu = share_u + ((size_t)wave * 64 + lane) * (EPT * R);
    double* mw = share_w + ((size_t)wave * 64 + lane) * (EPT * R);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if constexpr (scalar_traits<T>::is_complex) {
        mu[2 * e] = du[e].re;
        mu[2 * e + 1] = du[e].im;
        mw[2 * e] = dw[e].re;
        mw[2 * e + 1] = dw[e].im;
      } else {
        mu[e] = du[e];
        mw[e] = dw[e];
      }
    }
    __syncthreads();
    if (wave == 0) {
      T uc[EPT], wp[EPT];
      acc_t<T> last = zero<acc_t<T>>();
      double nn = 0.0;
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        acc_t<T> su, sw;
        auto at = [&](const double* base, int wv, int idx) { return base[((size_t)wv * 64 + lane) * (EPT * R) + idx]; };
        if constexpr (scalar_traits<T>::is_complex) {
          su = zc{(at(share_u, 0, 2 * e) + at(share_u, 1, 2 * e)) + (at(share_u, 2, 2 * e) + at(share_u, 3, 2 * e)),
                  (at(share_u, 0, 2 * e + 1) + at(share_u, 1, 2 * e + 1)) + (at(share_u, 2, 2 * e + 1) + at(share_u, 3, 2 * e + 1))};
          sw = zc{(at(share_w, 0, 2 * e) + at(share_w, 1, 2 * e)) + (at(share_w, 2, 2 * e) + at(share_w, 3, 2 * e)),
                  (at(share_w, 0, 2 * e + 1) + at(share_w, 1, 2 * e + 1)) + (at(share_w, 2, 2 * e + 1) + at(share_w, 3, 2 * e + 1))};
        } else {
          su = (at(share_u, 0, e) + at(share_u, 1, e)) + (at(share_u, 2, e) + at(share_u, 3, e));
          sw = (at(share_w, 0, e) + at(share_w, 1, e)) + (at(share_w, 2, e) + at(share_w, 3, e));
        }
        uc[e] = rmul(s, narrow<T>(sub(to_acc(rr[e]), su)));
        wp[e] = narrow<T>(sub(to_acc(wr[e]), sw));
        fnma_acc(wp[e], dlast, uc[e]);
        cfma_acc(last, uc[e], wp[e]);
        nn += abs2(wp[e]);
      }
      store_strip<T, 1>(lg.u_out, i0, n, uc);
      store_strip<T, 1>(w, i0, n, wp);
      if constexpr (scalar_traits<T>::is_complex) {
        const double lr = wave_sum(last.re), li = wave_sum(last.im);
        if (lane == 0) {
          cols[R * nb] += lr;
          cols[R * nb + 1] += li;
        }
      } else {
        const double lr = wave_sum(last);
        if (lane == 0) cols[R * nb] += lr;
      }
      nn = wave_sum(nn);
      if (lane == 0) cols[ncols - 1] += nn;
    }
    __syncthreads();  // the shares are rewritten by the next strip
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock) out[i] = cols[i];
}

// The pair sweep (pair_sweep_kernel's algebra, see there) in the SMALL-VECTOR geometry — vectors of 320 KiB .. 1 MiB, where the
// reference's users live (n = 4e4 .. 1.3e5 doubles): four waves share a strip of 64 lanes x 16 B and split the stored vectors
// between them (trips of kSmallJB vectors dealt round-robin).  Every wave takes the measured coefficients <u_j, r3>, <u_j, r4 raw>
// of its vectors (LDS-transposed column sums, as in mdot_small_kernel) and accumulates its shares of the three updates
// sum g1_j u_j, sum g2_j u_j (late updates of u_P, u_{P+1}) and sum p4_j u_j (compensation of the next operator input); wave 0
// adds the four shares in a fixed order, finishes the three strips and takes the in-strip dots.  One launch (no split: the
// launcher refuses more columns than the LDS holds and the loop keeps the one-sweep form there).  Partial columns in the layout
// of pair_sweep_kernel: [m3: R P][m4: R P][<u_P,r3>][<u_{P+1},r3>][<u_P,r4>][<u_{P+1},r4>][<r3,r4>] (R each) [|r4|^2].
static int small_pair_lds_doubles(int ncols, int ept_times_reals) {
  return ((ncols + 15) & ~15) + 4 * 16 * kSmallTileRow + 3 * kBlock * ept_times_reals;
}
template <typename T>
__global__ __launch_bounds__(kBlock) void pair_small_kernel(int64_t n, BasisSegs<T> segs, int P, const T* r1, const T* __restrict__ r2,
                                                            const T* __restrict__ r3, T* __restrict__ r4, T* uP_out,
                                                            T* __restrict__ uQ_out, const double* __restrict__ g1,
                                                            const double* __restrict__ g2, const double* __restrict__ gam,
                                                            const double* __restrict__ p4, const double* __restrict__ rho1sq,
                                                            const double* __restrict__ rho2sq, const double* __restrict__ e2,
                                                            const double* __restrict__ n3sq, double* __restrict__ partials) {
  // (r1 may alias uP_out: entering the pair form, u_{k-2} is already complete and is rewritten with zero coefficients)
  constexpr int EPT = strip<T, 1>::EPT;
  constexpr int ELEMS = strip<T, 1>::WAVE_ELEMS;
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = 2 * R * P + 5 * R + 1;
  extern __shared__ double lds[];  // [ncols] column sums, one [16][65] tile per wave, the waves' shares of the three updates
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* cols = lds;
  double* tile = lds + ((ncols + 15) & ~15) + wave * (16 * kSmallTileRow);
  double* share1 = lds + ((ncols + 15) & ~15) + 4 * (16 * kSmallTileRow);
  double* share2 = share1 + (size_t)kBlock * EPT * R;
  double* share4 = share2 + (size_t)kBlock * EPT * R;
  for (int i = tid; i < ncols; i += kBlock) cols[i] = 0.0;
  const double s1 = 1.0 / sqrt(*rho1sq), s2 = 1.0 / sqrt(*rho2sq);
  const double n3 = sqrt(*n3sq);
  const double ca = *e2 / n3, cb = n3 * s2;
  acc_t<T> gm;
  if constexpr (scalar_traits<T>::is_complex) gm = zc{gam[0], gam[1]};
  else gm = gam[0];
  double* tail = cols + 2 * R * P;
  __syncthreads();

  const int64_t nstrips = (n + ELEMS - 1) / ELEMS;
  for (int64_t sidx = blockIdx.x; sidx < nstrips; sidx += gridDim.x) {  // same trip count for every wave of the workgroup
    const int64_t i0 = sidx * ELEMS + (int64_t)lane * EPT;
    T a1[EPT], a2[EPT], b3[EPT], b4r[EPT];
    load_strip<T, 1>(r1, i0, n, a1);
    load_strip<T, 1>(r2, i0, n, a2);
    load_strip<T, 1>(r3, i0, n, b3);
    load_strip<T, 1>(r4, i0, n, b4r);
#pragma unroll
    for (int e = 0; e < EPT; ++e) b4r[e] = sub(sub(b4r[e], rmul(ca, b3[e])), rmul(cb, a2[e]));
    acc_t<T> d1[EPT], d2[EPT], d4[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) d1[e] = d2[e] = d4[e] = zero<acc_t<T>>();
    int trip = 0, col0 = 0;
    for (int sg = 0; sg < segs.nseg; ++sg) {
      const T* ub = segs.base[sg];
      const int cnt = segs.count[sg];
      for (int j = 0; j < cnt; j += kSmallJB, ++trip) {
        if ((trip & 3) != wave) continue;
        const int nv = min(kSmallJB, cnt - j);
        T ur[kSmallJB][EPT];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b)
          if (b < nv) load_strip<T, 1>(ub + (int64_t)(j + b) * segs.ld, i0, n, ur[b]);
        acc_t<T> s3[kSmallJB], s4[kSmallJB];
#pragma unroll
        for (int b = 0; b < kSmallJB; ++b) {
          s3[b] = zero<acc_t<T>>();
          s4[b] = zero<acc_t<T>>();
          if (b < nv) {
            const int c = col0 + R * (j + b);
            acc_t<T> c1, c2, c4;
            if constexpr (scalar_traits<T>::is_complex) {
              c1 = zc{g1[c], g1[c + 1]};
              c2 = zc{g2[c], g2[c + 1]};
              c4 = zc{p4[c], p4[c + 1]};
            } else {
              c1 = g1[c];
              c2 = g2[c];
              c4 = p4[c];
            }
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
              cfma_acc(s3[b], ur[b][e], b3[e]);
              cfma_acc(s4[b], ur[b][e], b4r[e]);
              fma_acc(d1[e], c1, to_acc(ur[b][e]));
              fma_acc(d2[e], c2, to_acc(ur[b][e]));
              fma_acc(d4[e], c4, to_acc(ur[b][e]));
            }
          }
        }
        // the trip's column sums through the wave's transpose tile (16 rows): <u_j, r3> first, then <u_j, r4 raw>
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
          for (int b = 0; b < kSmallJB; ++b) {
            const acc_t<T> v = which == 0 ? s3[b] : s4[b];
            if constexpr (scalar_traits<T>::is_complex) {
              tile[(2 * b) * kSmallTileRow + lane] = v.re;
              tile[(2 * b + 1) * kSmallTileRow + lane] = v.im;
            } else {
              tile[b * kSmallTileRow + lane] = v;
            }
          }
          wave_lds_handover();
          const int i = lane >> 2, q = lane & 3;
          double sum = 0.0;
          if (i < nv * R) {
            const double* row = tile + i * kSmallTileRow + q * 16;
#pragma unroll
            for (int t2 = 0; t2 < 16; ++t2) sum += row[t2];
          }
          sum += __shfl_xor(sum, 1, 64);
          sum += __shfl_xor(sum, 2, 64);
          if (q == 0 && i < nv * R) cols[which * R * P + col0 + R * j + i] += sum;  // this column belongs to this wave alone
          wave_lds_handover();
        }
      }
      col0 += R * cnt;
    }
    double* m1 = share1 + ((size_t)wave * 64 + lane) * (EPT * R);
    double* m2 = share2 + ((size_t)wave * 64 + lane) * (EPT * R);
    double* m4 = share4 + ((size_t)wave * 64 + lane) * (EPT * R);
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if constexpr (scalar_traits<T>::is_complex) {
        m1[2 * e] = d1[e].re;
        m1[2 * e + 1] = d1[e].im;
        m2[2 * e] = d2[e].re;
        m2[2 * e + 1] = d2[e].im;
        m4[2 * e] = d4[e].re;
        m4[2 * e + 1] = d4[e].im;
      } else {
        m1[e] = d1[e];
        m2[e] = d2[e];
        m4[e] = d4[e];
      }
    }
    __syncthreads();
    if (wave == 0) {
      T u1[EPT], u2[EPT], b4[EPT];
      acc_t<T> t3p = zero<acc_t<T>>(), t3q = zero<acc_t<T>>(), t4p = zero<acc_t<T>>(), t4q = zero<acc_t<T>>(),
               d34 = zero<acc_t<T>>();
      double nn = 0.0;
      auto total = [&](const double* base, int idx) {
        auto at = [&](int wv) { return base[((size_t)wv * 64 + lane) * (EPT * R) + idx]; };
        return (at(0) + at(1)) + (at(2) + at(3));
      };
#pragma unroll
      for (int e = 0; e < EPT; ++e) {
        acc_t<T> t1, t2, t4;
        if constexpr (scalar_traits<T>::is_complex) {
          t1 = zc{total(share1, 2 * e), total(share1, 2 * e + 1)};
          t2 = zc{total(share2, 2 * e), total(share2, 2 * e + 1)};
          t4 = zc{total(share4, 2 * e), total(share4, 2 * e + 1)};
        } else {
          t1 = total(share1, e);
          t2 = total(share2, e);
          t4 = total(share4, e);
        }
        u1[e] = rmul(s1, narrow<T>(sub(to_acc(a1[e]), t1)));
        T h2 = narrow<T>(sub(to_acc(a2[e]), t2));
        fnma_acc(h2, gm, u1[e]);
        u2[e] = rmul(s2, h2);
        b4[e] = narrow<T>(sub(to_acc(b4r[e]), t4));
        cfma_acc(t3p, u1[e], b3[e]);
        cfma_acc(t3q, u2[e], b3[e]);
        cfma_acc(t4p, u1[e], b4[e]);
        cfma_acc(t4q, u2[e], b4[e]);
        cfma_acc(d34, b3[e], b4[e]);
        nn += abs2(b4[e]);
      }
      store_strip<T, 1>(uP_out, i0, n, u1);
      store_strip<T, 1>(uQ_out, i0, n, u2);
      store_strip<T, 1>(r4, i0, n, b4);
      const acc_t<T> sums[5] = {wave_sum(t3p), wave_sum(t3q), wave_sum(t4p), wave_sum(t4q), wave_sum(d34)};
      nn = wave_sum(nn);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 5; ++c) {
          if constexpr (scalar_traits<T>::is_complex) {
            tail[2 * c] += sums[c].re;
            tail[2 * c + 1] += sums[c].im;
          } else {
            tail[c] += sums[c];
          }
        }
        tail[5 * R] += nn;
      }
    }
    __syncthreads();  // the shares are rewritten by the next strip
  }
  __syncthreads();
  double* out = partials + (size_t)blockIdx.x * ncols;
  for (int i = tid; i < ncols; i += kBlock) out[i] = cols[i];
}
template <typename T> bool pair_small_fits(int P) {
  constexpr int R = scalar_traits<T>::reals;
  return (size_t)small_pair_lds_doubles(2 * R * P + 5 * R + 1, (int)(16 / sizeof(T)) * R) * sizeof(double) <= (size_t)64 * 1024;
}
// false: more columns than one workgroup's LDS holds in this geometry (nothing was launched)
template <typename T>
bool launch_pair_sweep_small(int64_t n, const BasisSegs<T>& segs, int P, const T* r1, const T* r2, const T* r3, T* r4, T* uP_out,
                             T* uQ_out, const double* g1, const double* g2, const double* gam, const double* p4, const double* rho1sq,
                             const double* rho2sq, const double* e2, const double* n3sq, double* partials, int* grid_out,
                             hipStream_t s) {
  constexpr int R = scalar_traits<T>::reals;
  const int ncols = 2 * R * P + 5 * R + 1;
  const size_t lds_bytes = (size_t)small_pair_lds_doubles(ncols, (int)(16 / sizeof(T)) * R) * sizeof(double);
  if (!pair_small_fits<T>(P)) return false;  // (64 KiB, the default limit: no opt-in needed; P <= ~1240 real columns)
  const int grid = strip_grid(n, strip<T, 1>::WAVE_ELEMS);
  hipLaunchKernelGGL((pair_small_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, segs, P, r1, r2, r3, r4, uP_out, uQ_out, g1, g2,
                     gam, p4, rho1sq, rho2sq, e2, n3sq, partials);
  LL_HIP(hipGetLastError());
  *grid_out = grid;
  return true;
}

// ---- the small-vector halves of launch_mdot / launch_maxpy / launch_lagged (kernels.hip; declared in gs_strips.hpp)
template <typename T>
int launch_mdot_small(int64_t n, T* w, const BasisSegs<T>& segs, const ThreeTerm<T>& tt, const NormRefs& pred, int predicated,
                      double* partials, int ncols, hipStream_t s) {
  const int grid = strip_grid(n, strip<T, 1>::WAVE_ELEMS);
  const size_t lds_bytes = ((size_t)((ncols + 15) & ~15) + 4 * 16 * kSmallTileRow) * sizeof(double);
  hipLaunchKernelGGL((mdot_small_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, tt, pred, predicated, partials, ncols);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T> static size_t maxpy_small_lds_bytes(int nb) {
  constexpr int R = scalar_traits<T>::reals;
  return ((size_t)((R * nb + 1 + 15) & ~15) + (size_t)kBlock * strip<T, 1>::EPT * R) * sizeof(double);
}
template <typename T>
int launch_maxpy_small(int64_t n, T* w, const BasisSegs<T>& segs, const double* h, int nb, const NormRefs& pred, int predicated,
                       double* partials, hipStream_t s) {
  const int grid = strip_grid(n, strip<T, 1>::WAVE_ELEMS);
  hipLaunchKernelGGL((maxpy_small_kernel<T, false>), dim3(grid), dim3(kBlock), maxpy_small_lds_bytes<T>(nb), s, n, w, segs, h, nb, pred,
                     predicated, partials, nullptr, 0, nullptr, nullptr);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T>
int launch_lagged_small(int64_t n, T* w, const BasisSegs<T>& segs, int nb, const Lagged<T>& lg, const ThreeTerm<T>& tt,
                        double* partials, hipStream_t s) {
  constexpr int R = scalar_traits<T>::reals;
  const int grid = strip_grid(n, strip<T, 1>::WAVE_ELEMS);
  const size_t lds_bytes = (size_t)small_lagged_lds_doubles(R * (nb + 1) + 1, strip<T, 1>::EPT * R) * sizeof(double);
  hipLaunchKernelGGL((lagged_small_kernel<T>), dim3(grid), dim3(kBlock), lds_bytes, s, n, w, segs, nb, lg, lg.g, lg.t, tt, partials);
  LL_HIP(hipGetLastError());
  return grid;
}

// The multi-axpy that folds the multi-dot's partials itself (small-vector geometry only): true when the fused kernel was
// launched — the caller then skips launch_reduce_cols.  Worth it while every workgroup's redundant fold (mparts * ncols
// loads) stays well below the ~10 us a separate fold launch costs in a launch-bound loop.
template <typename T>
bool launch_maxpy_folding(int64_t n, T* w, const BasisSegs<T>& segs, const double* mdot_partials, int mparts, double* h_out,
                          double* c0_out, double* partials, int64_t small_bytes, int* grid_out, hipStream_t s) {
  int nb = 0;
  for (int i = 0; i < segs.nseg; ++i) nb += segs.count[i];
  constexpr int R = scalar_traits<T>::reals;
  if (!blas_small(n, sizeof(T), small_bytes) || (long long)mparts * (R * nb + 1) > 32768) return false;
  const int grid = strip_grid(n, strip<T, 1>::WAVE_ELEMS);
  hipLaunchKernelGGL((maxpy_small_kernel<T, true>), dim3(grid), dim3(kBlock), maxpy_small_lds_bytes<T>(nb), s, n, w, segs, nullptr, nb,
                     NormRefs{nullptr, nullptr, nullptr, 1}, 0, partials, mdot_partials, mparts, h_out, c0_out);
  LL_HIP(hipGetLastError());
  *grid_out = grid;
  return true;
}
#define LL_INST_SMALL(T)                                                                                                       \
  template int launch_mdot_small<T>(int64_t, T*, const BasisSegs<T>&, const ThreeTerm<T>&, const NormRefs&, int, double*, int,   \
                                    hipStream_t);                                                                                \
  template int launch_maxpy_small<T>(int64_t, T*, const BasisSegs<T>&, const double*, int, const NormRefs&, int, double*,        \
                                     hipStream_t);                                                                               \
  template bool launch_maxpy_folding<T>(int64_t, T*, const BasisSegs<T>&, const double*, int, double*, double*, double*,         \
                                        int64_t, int*, hipStream_t);                                                             \
  template int launch_lagged_small<T>(int64_t, T*, const BasisSegs<T>&, int, const Lagged<T>&, const ThreeTerm<T>&, double*,     \
                                      hipStream_t);                                                                              \
  template bool pair_small_fits<T>(int);                                                                                         \
  template bool launch_pair_sweep_small<T>(int64_t, const BasisSegs<T>&, int, const T*, const T*, const T*, T*, T*, T*,          \
                                           const double*, const double*, const double*, const double*, const double*,           \
                                           const double*, const double*, const double*, double*, int*, hipStream_t);
LL_FOR_EACH_SCALAR(LL_INST_SMALL)

}  // namespace ll
