// Propagation-blocked SpMV for gfx950 (a1/a2/a3: mv_mul LL:243 / EX:108, offset update LL:244-246, alpha dot LL:248).
// (Its matrix image is planned on the host, spmv_plan.hpp, and built on the device, spmv_image_build.hip; the 2-D tiled
// kernel for matrices with column locality is spmv_tiled.hip.)
//
// Measured on MI355X (profiles/r01_gather_probe.txt): a gather that misses the CU's 32 KiB L1 moves a whole 128-byte
// line for 8 useful bytes and the chip sustains only 57 G such gathers/s from an 80 MB x (217 G/s from an L2-resident
// table).  For a matrix without column locality (BASELINE config 3: 1.5e8 gathers) that caps ANY gather-based CSR
// kernel at >= 0.69 ms per SpMV (measured: 2.7 ms CSR-stream) while the matrix itself streams in 0.35 ms.
//
// These kernels therefore never gather from global memory.  The same matrix is stored in two sweeps' order (built
// once at upload, on the device) and one SpMV is two fully coalesced streaming kernels with LDS-resident slices:
//   phase 1 (one workgroup per COLUMN block): the x slice of the block is loaded into LDS; the block's entries
//            (value, 16-bit local column) stream in, ordered by destination row block; product = value * x_lds[col]
//            is written to the product buffer P at its position in row-block order (contiguous runs of one segment
//            = one (column block, row block) pair);
//   phase 2 (one workgroup per ROW block): the y slice lives in LDS; the row block's range of P and the 16-bit
//            local row indices stream in (perfectly sequential) and are added into the slice with ds_add_f64; the
//            epilogue adds offset*x_i (a2), writes y once and accumulates Re(conj(x_i) y_i) (a3).
// HBM traffic is 2*sizeof(T) + sizeof(T) + 4 bytes per nonzero (28 B for fp64 against 12 B for CSR) but every byte
// is streamed at full line efficiency and every x/y element is touched in LDS.
//
// Determinism: the LDS adds of phase 2 are issued WAVE BY WAVE in a fixed order (the 16 waves of the workgroup take
// turns inside every trip, a barrier between turns), so every y_i is summed in the same order on every launch: the
// kernel is bit-reproducible like every other reduction of the library (LL_PB_PHASE2=atomic restores the arrival-order
// adds for A/B timing).  The next trip's loads are in flight while the turns run, so the turns cost no bandwidth.
//
// Column blocks carry their own x-slice offset, so one image serves the single-GPU case (x in place), the sharded
// case (own columns from the local shard, the other ranks' columns from the gathered buffer, launched separately so
// that own-column work overlaps the all-gather) and a gather that arrives in several chunks.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <string>

#include "dev_helpers.hpp"
#include "fixed_round.hpp"
#include "ll_internal.hpp"
#include "spmv_shared.hpp"

namespace ll {

// ================================================================= software pipelines of the two phases
// One workgroup owns a CU (its LDS slice is > 100 KB), so nothing but the workgroup's own 16 waves hides memory latency:
// every lane keeps D trips of loads in flight in a STATIC ring of register slots — the trip loop is unrolled D times and
// every slot index is a compile-time constant, so a trip is consumed while the D - 1 requested after it are still in
// flight and the compiler can wait for exactly the oldest one (s_waitcnt vmcnt(N)).  (Rounds 1-2 rotated the slots by
// register copies at the end of every trip; a copy of slot d+1 needs ITS data, so every trip ended with a full drain of
// the memory pipeline and the stream and the LDS work ran one after the other.)
// Every vector-memory instruction of the trip loops is UNCONDITIONAL and sits in uniform straight-line code: a lane
// beyond the end of its range re-reads the range's last quad (a cache hit) and stores to a dump quad behind the image,
// only the LDS work is predicated.  With loads under divergent branches the number of outstanding loads is unknown at
// compile time and every wait degenerates to vmcnt(0) again.
// The quads of a workgroup's range are dealt out in WAVE CHUNKS (64 lanes x U quads) from a counter in LDS instead of
// by a fixed stride: the hardware favours a workgroup's oldest waves, so with a fixed partition wave 0 is done long
// before wave 15 (measured: 94 us against 160 us in phase 1) and the tail of every workgroup runs with a fraction of its
// loads in flight.  The first D - 1 chunks of every wave are fixed (they are requested before the counter is live).
template <int U, int W = kPbWaves> struct WaveChunks {  // W: waves of the workgroup
  static constexpr int kQuads = 64 * U;  // quads per chunk
  unsigned* ctr;                         // LDS: chunks handed out so far (starts at (D - 1) * W)
  long long g0;
  __device__ __forceinline__ long long fixed(int d) const { return g0 + (long long)((threadIdx.x >> 6) + d * W) * kQuads; }
  __device__ __forceinline__ long long grab() const {
    unsigned c = 0;
    if ((threadIdx.x & 63) == 0) c = atomicAdd(ctr, 1u);
    c = (unsigned)__builtin_amdgcn_readfirstlane((int)c);
    return g0 + (long long)c * kQuads;
  }
};
template <typename T, int D, int TH = kPbThreads> struct ColStream {  // phase 1: (4 values, 4 local columns) per lane per trip; TH lanes
  quad<T> v[D];
  ushort4 c[D];
  long long base[D];  // first quad of the chunk held in each slot
  const T* val;
  const ushort4* col;
  long long g1, glast;  // end of the range; last valid quad (>= its first quad; the image is padded behind its end)
  WaveChunks<1, TH / 64> chunks;
  __device__ __forceinline__ void issue(int slot, long long cbase) {
    base[slot] = cbase;
    const long long g = cbase + (threadIdx.x & 63);
    const long long gc = g < glast ? g : glast;
    v[slot] = load_quad<T>(val + 4 * gc);
    c[slot] = col[gc];
  }
  __device__ __forceinline__ void prologue() {
#pragma unroll
    for (int d = 0; d < D - 1; ++d) issue(d, chunks.fixed(d));
  }
  // consume(values, columns, quad index of this lane) for every chunk this wave gets; the counter must be live.
  // (The D phases are spelled out — slot indices must be compile-time constants, and a `return` inside a `#pragma
  // unroll` loop keeps the compiler from unrolling it.)
  template <int PH, typename F> __device__ __forceinline__ bool step(F&& consume) {
    const long long cur = base[PH];
    if (cur >= g1) return false;  // wave-uniform; chunks are handed out in ascending order
    issue((PH + D - 1) % D, chunks.grab());
    consume(v[PH], c[PH], cur + (threadIdx.x & 63));
    return true;
  }
  // (Measured and rejected in round 5: TWO rounds of the ring per loop iteration.  The waitcnt pass merges the pending loads of
  // the loop's two entries conservatively at its header, which costs a full drain in the first trip behind it — once per D
  // trips; with two rounds per iteration it is once per 2 D, yet config 3's SpMV came out 1 % slower on the same box,
  // 0.911 against 0.899 ms, profiles/r05_pb_ring_two_rounds_ab.txt: the other 15 waves of the workgroup cover the drain.)
  template <typename F> __device__ __forceinline__ void run(F&& consume) {
    static_assert(D >= 2 && D <= 4, "pipeline depth");
    for (;;) {
      if (!step<0>(consume)) return;
      if (!step<1>(consume)) return;
      if constexpr (D > 2) {
        if (!step<2>(consume)) return;
      }
      if constexpr (D > 3) {
        if (!step<3>(consume)) return;
      }
    }
  }
};
// phase 2: U x (4 products, 4 local rows) per lane per trip.  DYN: wave chunks as above; otherwise the fixed stride of
// the whole workgroup (the wave-ordered form needs every wave in every trip).
template <typename T, int U, int D, bool DYN> struct RowStream {
  quad<T> p[D][U];
  ushort4 r[D][U];
  long long base[D];
  const T* P;
  const ushort4* row;
  long long g1, glast;  // end of the range; last valid quad (>= the first quad: the image is padded behind its end)
  WaveChunks<U> chunks;
  static constexpr long long kTrip = (long long)U * kPbThreads;
  __device__ __forceinline__ long long quad_of(long long cbase, int u) const {
    return DYN ? cbase + (threadIdx.x & 63) + (long long)u * 64 : cbase + threadIdx.x + (long long)u * kPbThreads;
  }
  __device__ __forceinline__ void issue(int slot, long long cbase) {
    base[slot] = cbase;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long g = quad_of(cbase, u);
      const long long gc = g < glast ? g : glast;
      p[slot][u] = load_quad<T>(P + 4 * gc);
      r[slot][u] = row[gc];
    }
  }
  __device__ __forceinline__ void prologue() {
#pragma unroll
    for (int d = 0; d < D - 1; ++d) issue(d, DYN ? chunks.fixed(d) : chunks.g0 + d * kTrip);
  }
  // consume(products, rows, quad indices of this lane) for every trip; DYN: the counter must be live
  long long next_static;
  template <int PH, typename F> __device__ __forceinline__ bool step(F&& consume) {
    const long long cur = base[PH];
    if (cur >= g1) return false;  // uniform over the wave (DYN) / the workgroup
    long long nxt;
    if constexpr (DYN) nxt = chunks.grab();
    else {
      nxt = next_static;
      next_static += kTrip;
    }
    issue((PH + D - 1) % D, nxt);
    long long g[U];
#pragma unroll
    for (int u = 0; u < U; ++u) g[u] = quad_of(cur, u);
    consume(p[PH], r[PH], g);
    return true;
  }
  template <typename F> __device__ __forceinline__ void run(F&& consume) {
    static_assert(D >= 2 && D <= 4, "pipeline depth");
    next_static = chunks.g0 + (D - 1) * kTrip;
    for (;;) {
      if (!step<0>(consume)) return;
      if (!step<1>(consume)) return;
      if constexpr (D > 2) {
        if (!step<2>(consume)) return;
      }
      if constexpr (D > 3) {
        if (!step<3>(consume)) return;
      }
    }
  }
};


// ---- fixed-point sums (LL_PB_PHASE2=fixed, the default)
// Integer addition is associative, so if every product is first rounded to a fixed-point grid the LDS adds may arrive in
// ANY order — all waves add concurrently like in the arrival-order form — and the result is still the same bits on every
// launch, for every kernel geometry and every partition of the matrix.
//   grid of row i:  q_i = 2^(E_i - 62),  E_i = er_i + e_x + 1,  sum_j |a_ij| < 2^er_i (computed when the image is built),
//   max_k |x_k| < 2^e_x, so that the exact sum of the row, scaled by 1/q_i, fits a 64-bit integer with room to spare.
// Error per row: each product is rounded to q_i once (<= q_i / 2), the sum itself is exact:
//   |y_i - exact| <= nnz_i * 2^-63 * 2^E_i  <=  nnz_i * 2^-60 * (sum_j |a_ij|) max|x|      (lanczos_hip.h states this bound)
// — finer than the unit roundoff of a double-precision sum of terms of that size, and far below eps * ||A|| ||x||, the
// scale that matters to the Lanczos recurrence; NOT component-wise accurate for rows whose terms are all tiny against
// (sum_j |a_ij|) max|x| (LL_PB_PHASE2=ordered is).
// Phase 1 writes fl(a_ij x_j) and the maximum of |x| over its slice; phase 2 looks up the row's exponent per entry, scales,
// rounds and adds.  Rows that meet an Inf / NaN are reported as NaN.
// (Round 3 measured a PRE-SCALED form — image values a_ij 2^-er_i, max|x| known before phase 1, 64-bit integers in P,
// phase 2 a pure stream with one integer atomic per entry: the LDS work of phase 2 turned out to be free (removing the adds
// altogether changes nothing, profiles/r03_spmv_variants.txt runs C and G) while the float -> int64 conversion makes
// phase 1 borderline ALU-bound; no gain, removed again.)

// ================================================================= phase 1
// Workgroup b handles column block blk_first + b: the block's entries (4 values + 4 local columns per lane and trip)
// stream in, ordered by destination row block; product = value * x_lds[col] goes to the product buffer P at its position
// in row-block order.  The first D - 1 trips are requested before the x slice is staged.
// blockmax (nullable; fixed-point phase 2) receives the maximum of |x| over the slice.
template <typename T, int D, int TH>
__global__ __launch_bounds__(TH) void pb_phase1(int nrb, int blk_first, const int64_t* __restrict__ xoff,
                                                        const int32_t* __restrict__ ncols_tab,
                                                        const int64_t* __restrict__ seg_q,     // [ncb][nrb+1]
                                                        const int64_t* __restrict__ seg_dest,  // [ncb][nrb]
                                                        const T* __restrict__ val, const ushort4* __restrict__ col,
                                                        const T* __restrict__ xsrc, T* __restrict__ P, int cb_cols,
                                                        double* __restrict__ blockmax, long long p_dump,
                                                        const double* __restrict__ xnorm2) {
  extern __shared__ double lds[];
  // xnorm2 (nullable): the input is an UNNORMALISED vector w with ||w||^2 = *xnorm2 (lagged Gram-Schmidt, kernels.hip / gs_pair.hip): the
  // slice is scaled by 1 / ||w|| while it is staged
  const double xs_fac = xnorm2 ? 1.0 / sqrt(*xnorm2) : 1.0;
  __shared__ double bm_red[TH / 64 + 1];
  __shared__ unsigned chunk_ctr;
  T* xs = reinterpret_cast<T*>(lds);                                               // [cb_cols]
  long long* qs = reinterpret_cast<long long*>(reinterpret_cast<char*>(lds) +
                                              (((size_t)cb_cols * sizeof(T) + 15) & ~(size_t)15));  // [nrb + 1]
  long long* db = qs + (nrb + 1);                                                  // [nrb]
  const int tid = threadIdx.x;
  const int c = blk_first + blockIdx.x;
  const int64_t* sq = seg_q + (size_t)c * (nrb + 1);
  const long long g0 = sq[0] >> 2, g1 = sq[nrb] >> 2;

  ColStream<T, D, TH> st;
  st.val = val;
  st.col = col;
  st.g1 = g1;
  st.glast = g1 > g0 ? g1 - 1 : g0;
  st.chunks.ctr = &chunk_ctr;
  st.chunks.g0 = g0;
  st.prologue();
  if (tid == 0) chunk_ctr = (D - 1) * (TH / 64);  // (published by the barriers below)
  {  // stage the x slice (16-byte loads when the slice is 16-byte aligned) and the segment tables.  All loads of a batch are
    // requested before the first LDS store (clamped addresses, no load under a divergent branch): a load -> store loop
    // per piece is a chain of memory latencies — 9-17 us per workgroup with nothing else running on the CU.
    const int ncols = ncols_tab[c];
    const T* src = xsrc + xoff[c];
    constexpr int V = (int)(16 / sizeof(T));
    if (V >= 1 && ncols >= V && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const int nv = ncols / V;
      const uint4* s4 = reinterpret_cast<const uint4*>(src);
      uint4* d4 = reinterpret_cast<uint4*>(xs);
      constexpr int SB = 7;  // 7 x 1024 x 16 B = 112 KiB: every slice in one batch (256 lanes: 28 KiB, more than their slices)
      for (int i0 = 0; i0 < nv; i0 += SB * TH) {
        uint4 piece[SB];
#pragma unroll
        for (int b = 0; b < SB; ++b) {
          const int i = i0 + b * TH + tid;
          piece[b] = s4[i < nv ? i : nv - 1];
        }
#pragma unroll
        for (int b = 0; b < SB; ++b) {
          const int i = i0 + b * TH + tid;
          if (xnorm2) {
            T el[V];
            __builtin_memcpy(el, &piece[b], sizeof(uint4));
#pragma unroll
            for (int q = 0; q < V; ++q) el[q] = rmul(xs_fac, el[q]);
            __builtin_memcpy(&piece[b], el, sizeof(uint4));
          }
          if (i < nv) d4[i] = piece[b];
        }
      }
      for (int i = nv * V + tid; i < ncols; i += TH) xs[i] = rmul(xs_fac, src[i]);
    } else {
      for (int i = tid; i < ncols; i += TH) xs[i] = rmul(xs_fac, src[i]);
    }
    const int64_t* sd = seg_dest + (size_t)c * nrb;
    for (int i0 = 0; i0 <= nrb; i0 += 2 * TH) {
      long long tq[2], td[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int i = i0 + b * TH + tid;
        tq[b] = sq[i <= nrb ? i : nrb];
        td[b] = sd[i < nrb ? i : (nrb > 0 ? nrb - 1 : 0)];
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int i = i0 + b * TH + tid;
        if (i <= nrb) qs[i] = tq[b];
        if (i < nrb) db[i] = td[b];
      }
    }
  }
  __syncthreads();
  if (blockmax != nullptr) {  // the largest |x| of the slice (phase 2 needs max |x| over all columns)
    double m = 0.0;
    const int ncols = ncols_tab[c];
    for (int i = tid; i < ncols; i += TH) m = fmax(m, abs1(xs[i]));
    m = pb_block_max<TH / 64>(m, bm_red);
    if (tid == 0) blockmax[c] = m;  // NaN in the slice: fmax drops it; the products carry it into P and phase 2 reports it
  }
  int r = 0;
  T* const dump = P + p_dump;  // where lanes beyond the block's last quad store (a quad behind the image)
  auto consume = [&](const quad<T>& v, const ushort4& cl, long long g) {
    const long long qq = 4 * g;
    while (r + 1 < nrb && qq >= qs[r + 1]) ++r;
    const unsigned short cc[4] = {cl.x, cl.y, cl.z, cl.w};
    quad<T> pr;
#pragma unroll
    for (int e = 0; e < 4; ++e) pr.e[e] = mul(v.e[e], xs[cc[e]]);
    store_quad<T>(g < g1 ? P + db[r] + (qq - qs[r]) : dump, pr);
  };
  st.run(consume);
}

// ================================================================= phase 2
// One workgroup per ROW block (y slice in LDS): the block's range of P and of the 16-bit local rows streams in and is
// added into the slice; the epilogue adds offset * x_i (a2), writes y once and accumulates Re(conj(x_i) y_i) (a3).
// Floating-point sums.  ORDERED: the 16 waves add in turn (a barrier between turns) — a fixed order, so every y_i is the
// same bits on every launch, and component-wise accurate like the reference's fp64 mv_mul; otherwise arrival order
// (LL_PB_PHASE2=atomic: not reproducible, A/B timing reference).
template <typename T, bool ORDERED, int D>
__global__ __launch_bounds__(kPbThreads) void pb_phase2(int rb_rows, int64_t n_local,
                                                        const int64_t* __restrict__ rptr,  // [nrb + 1]
                                                        const ushort4* __restrict__ row, const T* __restrict__ P,
                                                        const T* __restrict__ xl, T* __restrict__ y, double offset,
                                                        double* __restrict__ dot_partials, const double* __restrict__ xnorm2,
                                                        const T* __restrict__ diag) {
  constexpr int R = scalar_traits<T>::reals;
  constexpr int U = 2;
  extern __shared__ double lds[];  // [rb_rows * R]
  __shared__ double red[kPbWaves];
  const int tid = threadIdx.x, wave = tid >> 6;
  const int rb = blockIdx.x;
  const int64_t row0 = (int64_t)rb * rb_rows;
  const int rows = (int)min((int64_t)rb_rows, n_local - row0);
  const long long g0 = rptr[rb] >> 2, g1 = rptr[rb + 1] >> 2;
  __shared__ unsigned chunk_ctr;
  RowStream<T, U, D, !ORDERED> st;
  st.P = P;
  st.row = row;
  st.g1 = g1;
  st.glast = g1 > g0 ? g1 - 1 : g0;
  st.chunks.ctr = &chunk_ctr;
  st.chunks.g0 = g0;
  st.prologue();
  if (tid == 0) chunk_ctr = (D - 1) * kPbWaves;
  for (int i = tid; i < rb_rows * R; i += kPbThreads) lds[i] = 0.0;
  __syncthreads();
  st.run([&](const quad<T>(&p)[U], const ushort4(&r)[U], const long long(&g)[U]) {
    auto add_mine = [&]() {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (g[u] < g1) {
          lds_add_elem<T>(lds, r[u].x, p[u].e[0]);
          lds_add_elem<T>(lds, r[u].y, p[u].e[1]);
          lds_add_elem<T>(lds, r[u].z, p[u].e[2]);
          lds_add_elem<T>(lds, r[u].w, p[u].e[3]);
        }
      }
    };
    if constexpr (ORDERED) {
      for (int w = 0; w < kPbWaves; ++w) {
        if (wave == w) add_mine();
        __syncthreads();
      }
    } else {
      add_mine();
    }
  });
  __syncthreads();
  pb_phase2_epilogue<T>(
      rb, row0, rows, xl, y, offset, dot_partials, red, xnorm2,
      [&](int i, const T& xi, const T& dg) {
        acc_t<T> a;
        if constexpr (scalar_traits<T>::is_complex) a = zc{lds[2 * i], lds[2 * i + 1]};
        else a = lds[i];
        if (diag) a = add(a, to_acc(mul(dg, xi)));  // the diagonal entry, kept outside the streams (spmv_image_build.hip pb_diag_kernel)
        return a;
      },
      [&](int i) { return diag ? diag[row0 + i] : zero<T>(); });
}

// Fixed-point sums (see above): P holds fl(a_ij x_j) in the storage type.
template <typename T, int D>
__global__ __launch_bounds__(kPbThreads) void pb_phase2_fixed(int rb_rows, int64_t n_local, int ncb,
                                                              const int64_t* __restrict__ rptr,
                                                              const ushort4* __restrict__ row, const T* __restrict__ P,
                                                              const int16_t* __restrict__ rexp,
                                                              const double* __restrict__ blockmax,
                                                              const T* __restrict__ xl, T* __restrict__ y, double offset,
                                                              double* __restrict__ dot_partials,
                                                              const double* __restrict__ xnorm2, int xprefetch,
                                                              const T* __restrict__ diag) {
  constexpr int R = scalar_traits<T>::reals;
  constexpr int U = 2;
  extern __shared__ double lds_raw[];
  long long* acc = reinterpret_cast<long long*>(lds_raw);                   // [rb_rows * R]
  int16_t* ex = reinterpret_cast<int16_t*>(acc + (size_t)rb_rows * R);      // [rb_rows]: 62 - E_i, or kBadRow
  __shared__ double red[kPbWaves + 1];
  constexpr int kBadRow = 32767;
  const int tid = threadIdx.x;
  const int rb = blockIdx.x;
  const int64_t row0 = (int64_t)rb * rb_rows;
  const int rows = (int)min((int64_t)rb_rows, n_local - row0);
  const long long g0 = rptr[rb] >> 2, g1 = rptr[rb + 1] >> 2;
  __shared__ unsigned chunk_ctr;
  // The epilogue needs x_i of the block's rows (offset term, alpha).  Requested HERE, before the stream's first trips and
  // held in registers: the loads are older than every load of the stream, so they have arrived long before the epilogue,
  // which otherwise spends 3-4 dependent rounds of global loads per workgroup with nothing else running on the CU
  // (8-byte types with at most kPbXPre rows per lane; LL_PB_XPRE=0 in the launcher: load them in the epilogue, round-3 form).
  T xpre[kPbXPre];
  if constexpr (sizeof(T) <= 8) {
    if (xprefetch) {
#pragma unroll
      for (int u = 0; u < kPbXPre; ++u) {
        const int i = tid + u * kPbThreads;
        xpre[u] = xl[row0 + (i < rows ? i : rows - 1)];
      }
    }
  }
  RowStream<T, U, D, true> st;
  st.P = P;
  st.row = row;
  st.g1 = g1;
  st.glast = g1 > g0 ? g1 - 1 : g0;
  st.chunks.ctr = &chunk_ctr;
  st.chunks.g0 = g0;
  st.prologue();
  if (tid == 0) chunk_ctr = (D - 1) * kPbWaves;
  {  // exponent of max |x| over ALL columns (every column block left its slice maximum)
    double m = 0.0;
    for (int i = tid; i < ncb; i += kPbThreads) m = fmax(m, blockmax[i]);
    for (int i = tid; i < rb_rows * R; i += kPbThreads) acc[i] = 0;
    const double t = pb_block_max(m, red);
    int e_x = -2000;  // x == 0: any scale does
    if (t > 0.0 && isfinite(t)) (void)frexp(t, &e_x);  // t < 2^e
    else if (!(t == 0.0)) e_x = kPbXInf;               // Inf: every row of the block is reported as NaN
    for (int i = tid; i < rb_rows; i += kPbThreads) {
      int k = kBadRow;
      if (i < rows) {
        const int er = rexp[row0 + i];
        if (er != 32767 && e_x != kPbXInf) k = max(-1000, min(1000, 62 - (er + e_x + 1)));
      } else {
        k = 0;
      }
      ex[i] = (int16_t)k;
    }
    __syncthreads();
  }
  st.run([&](const quad<T>(&p)[U], const ushort4(&r)[U], const long long(&g)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (g[u] < g1) {
        const unsigned short rr[4] = {r[u].x, r[u].y, r[u].z, r[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = ex[rr[e]];
          const double sc = pow2(k == kBadRow ? 0 : k);
          long long w[R];
          if constexpr (scalar_traits<T>::is_complex) {
            w[0] = pb_to_fixed((double)p[u].e[e].re * sc);
            w[1] = pb_to_fixed((double)p[u].e[e].im * sc);
          } else {
            w[0] = pb_to_fixed((double)p[u].e[e] * sc);
          }
          bool ok = true;
#pragma unroll
          for (int q = 0; q < R; ++q) {
            if (w[q] == kPbBadProduct) ok = false;
            else atomicAdd(reinterpret_cast<unsigned long long*>(&acc[R * rr[e] + q]), (unsigned long long)w[q]);
          }
          if (!ok) ex[rr[e]] = (int16_t)kBadRow;  // the row's result is NaN (same value from every writer)
        }
      }
    }
  });
  __syncthreads();
  // (the row's diagonal entry is kept outside the streams, spmv_image_build.hip pb_diag_kernel: its product joins the row's integers here —
  // rounded to the same grid, added to the same sum: the same bits as if it had travelled through the product buffer)
  auto value = [&](int i, const T& xi, const T& dg) {  // dg: the row's diagonal entry (requested ahead, see the epilogue)
    int k = ex[i];
    long long s[R];
#pragma unroll
    for (int q = 0; q < R; ++q) s[q] = acc[R * i + q];
    if (diag != nullptr && k != kBadRow) {
      const T p = mul(dg, xi);
      const double sc = pow2(k);
      long long w[R];
      if constexpr (scalar_traits<T>::is_complex) {
        w[0] = pb_to_fixed((double)p.re * sc);
        w[1] = pb_to_fixed((double)p.im * sc);
      } else {
        w[0] = pb_to_fixed((double)p * sc);
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        if (w[q] == kPbBadProduct) k = kBadRow;
        else s[q] = (long long)((unsigned long long)s[q] + (unsigned long long)w[q]);
      }
    }
    const double back = k == kBadRow ? __longlong_as_double(0x7ff8000000000000ll) : pow2(-k);  // NaN for unusable rows
    acc_t<T> a;
    if constexpr (scalar_traits<T>::is_complex) a = zc{(double)s[0] * back, (double)s[1] * back};
    else a = (double)s[0] * back;
    return a;
  };
  if constexpr (sizeof(T) <= 8) {
    if (xprefetch) {  // same arithmetic, same order of the per-lane dot sum (rows tid, tid + 1024, ...) as the loading form
      const double xs_fac = xnorm2 ? 1.0 / sqrt(*xnorm2) : 1.0;
      double dot_acc = 0.0;
      // the diagonal entries of the lane's rows in one batch (clamped addresses, no load under the per-row branch): the ring's
      // registers are free here; requested row by row they were a chain of up to 13 memory latencies — the 17 us of this epilogue
      T dgs[kPbXPre];
#pragma unroll
      for (int u = 0; u < kPbXPre; ++u) {
        const int i = tid + u * kPbThreads;
        dgs[u] = diag ? diag[row0 + (i < rows ? i : rows - 1)] : zero<T>();
      }
#pragma unroll
      for (int u = 0; u < kPbXPre; ++u) {
        const int i = tid + u * kPbThreads;
        if (i < rows) {
          const T xi = rmul(xs_fac, xpre[u]);
          const T yi = add(narrow<T>(value(i, xi, dgs[u])), rmul(offset, xi));
          y[row0 + i] = yi;
          dot_acc += re_cmul(xi, yi);
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
      return;
    }
  }
  pb_phase2_epilogue<T>(rb, row0, rows, xl, y, offset, dot_partials, red, xnorm2, value,
                        [&](int i) { return diag ? diag[row0 + i] : zero<T>(); });
}

// ================================================================= launchers
namespace {
// trips of loads in flight per lane: three in both phases (two for the 16-byte types in phase 2, where a third trip spills
// registers).  Measured on config 3 (profiles/r03_spmv_variants.txt): 3/3 0.898 ms, 2/2 0.937, 4/3 0.892, 3/2 0.890, 2/3
// 0.889 on one box — beyond two trips the differences are inside the 2-4 % position noise of one process.
template <typename T> constexpr int pb_depth2() { return sizeof(T) < 16 ? 3 : 2; }
constexpr int kPbDepth1 = 3;

template <typename T> void pb_opt_in_lds() {
  static std::atomic<unsigned long long> mask{0};
  once_per_device(mask, [] {
    constexpr int D2 = pb_depth2<T>();
    pb_opt_in(&pb_phase1<T, kPbDepth1, kPbThreads>);
    pb_opt_in(&pb_phase1<T, kPbDepth1, 256>);
    pb_opt_in(&pb_phase1<T, kPbDepth1, 512>);
    pb_opt_in(&pb_phase2<T, false, D2>);
    pb_opt_in(&pb_phase2<T, true, D2>);
    pb_opt_in(&pb_phase2_fixed<T, D2>);
  });
}

template <typename T>
void phase1_launch(const ll_operator& op, int blk_first, int blk_count, const T* xsrc, const double* xnorm2, hipStream_t s) {
  const size_t lds1 = (((size_t)op.pb.cb_cols * sizeof(T) + 15) & ~(size_t)15) + (size_t)(2 * op.pb.nrb + 1) * sizeof(long long);
  double* bm = op.pb.phase2 == LL_PB_FIXED ? op.pb.blockmax.get() : nullptr;
#define LL_PB_LAUNCH1(TH)                                                                                                              \
  hipLaunchKernelGGL((pb_phase1<T, kPbDepth1, TH>), dim3(blk_count), dim3(TH), lds1, s, op.pb.nrb, blk_first, op.pb.xoff.get(),        \
                     op.pb.ncols.get(), op.pb.segq.get(), op.pb.segdest.get(), (const T*)op.pb.val, (const ushort4*)op.pb.col, xsrc,   \
                     (T*)op.pb.prod, op.pb.cb_cols, bm, (long long)op.pb.entries, xnorm2)
  // Fewer lanes per workgroup for the thin column blocks of a sharded image: at N = 8 a block holds 16 K entries — four trips of
  // 1024 lanes, two of them requested by the prologue: the ring never reaches its steady state — but 8 trips of 512 lanes
  // (measured on config 4's shards through the stand-in transport, profiles/r05_shard_phase1_lanes.txt: 60.8 -> 41.9 us per
  // launch at N = 8 with the same 68 KB slices; smaller slices with more workgroups per CU lose to their segment count)
  if (op.pb.threads1 == 256) LL_PB_LAUNCH1(256);
  else if (op.pb.threads1 == 512) LL_PB_LAUNCH1(512);
  else LL_PB_LAUNCH1(kPbThreads);
#undef LL_PB_LAUNCH1
  LL_HIP(hipGetLastError());
}
}  // namespace

template <typename T>
void launch_pb_phase1(const ll_operator& op, int blk_first, int blk_count, const T* xsrc, hipStream_t s, const double* xnorm2) {
  if (blk_count <= 0 || op.pb.nrb <= 0) return;
  pb_opt_in_lds<T>();
  phase1_launch<T>(op, blk_first, blk_count, xsrc, xnorm2, s);
}

template <typename T>
int launch_pb_phase2(const ll_operator& op, const T* x_local, T* y, double offset, double* dot_partials,
                     hipStream_t s, const double* xnorm2) {
  if (op.pb.nrb <= 0) return 0;
  pb_opt_in_lds<T>();
  const dim3 grid(op.pb.nrb), block(kPbThreads);
  constexpr int D2 = pb_depth2<T>();
  if (op.pb.phase2 == LL_PB_FIXED) {  // order-independent fixed-point sums, LATE form
    const size_t ldsf = (size_t)op.pb.rb_rows * (sizeof(acc_t<T>) + sizeof(int16_t)) + 16;
    hipLaunchKernelGGL((pb_phase2_fixed<T, D2>), grid, block, ldsf, s, op.pb.rb_rows, op.n_local, op.pb.ncb, op.pb.rptr.get(),
                       (const ushort4*)op.pb.row, (const T*)op.pb.prod, op.pb.rexp.get(), op.pb.blockmax.get(), x_local, y,
                       offset, dot_partials, xnorm2, (op.pb.xpre && op.pb.rb_rows <= kPbXPre * kPbThreads) ? 1 : 0,
                       (const T*)op.pb.diag.get());
  } else {
    const size_t lds2 = (size_t)op.pb.rb_rows * sizeof(acc_t<T>);
    if (op.pb.phase2 == LL_PB_ORDERED)
      hipLaunchKernelGGL((pb_phase2<T, true, D2>), grid, block, lds2, s, op.pb.rb_rows, op.n_local, op.pb.rptr.get(),
                         (const ushort4*)op.pb.row, (const T*)op.pb.prod, x_local, y, offset, dot_partials, xnorm2,
                         (const T*)op.pb.diag.get());
    else
      hipLaunchKernelGGL((pb_phase2<T, false, D2>), grid, block, lds2, s, op.pb.rb_rows, op.n_local, op.pb.rptr.get(),
                         (const ushort4*)op.pb.row, (const T*)op.pb.prod, x_local, y, offset, dot_partials, xnorm2,
                         (const T*)op.pb.diag.get());
  }
  LL_HIP(hipGetLastError());
  return op.pb.nrb;
}

template <typename T>
int launch_spmv_pb(const ll_operator& op, const T* x_gathered, const T* x_own, const T* x_local, T* y, double offset,
                   double* dot_partials, hipStream_t s, const double* xnorm2) {
  launch_pb_phase1<T>(op, 0, op.pb.own_count, x_own, s, xnorm2);
  for (int c = 0; c < op.pb.gather.nchunks; ++c)
    launch_pb_phase1<T>(op, op.pb.chunk_first[c], op.pb.chunk_count[c], x_gathered, s, xnorm2);
  return launch_pb_phase2<T>(op, x_local, y, offset, dot_partials, s, xnorm2);
}
#define LL_INST_PB(T)                                                                                              \
  template void launch_pb_phase1<T>(const ll_operator&, int, int, const T*, hipStream_t, const double*);            \
  template int launch_pb_phase2<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const double*);  \
  template int launch_spmv_pb<T>(const ll_operator&, const T*, const T*, const T*, T*, double, double*, hipStream_t, \
                                 const double*);
LL_FOR_EACH_SCALAR(LL_INST_PB)

}  // namespace ll
