// 2-D tiled SpMV for gfx950 (a1/a2/a3 like the propagation-blocked kernels of spmv_pb.hip): the kernel for matrices with column
// locality, its max|x| pre-pass and their launchers.  The image is planned on the host (spmv_plan.hpp) and built on the device
// (spmv_image_build.hip).
#include <algorithm>
#include <atomic>

#include "dev_helpers.hpp"
#include "fixed_round.hpp"
#include "ll_internal.hpp"
#include "spmv_shared.hpp"

namespace ll {

// (third candidate of the creation-time timing, LL_SPMV_TILED)
// Propagation blocking pays a 16 B/nnz round trip of the products through memory because, for a matrix WITHOUT column
// locality, the x values a row block needs are spread over the whole vector.  When the columns of a row block fall into
// few column tiles (bands, stencils, lattices — every operator the reference itself ships: sample3_dynamic.cpp:17-22,
// exponentiator_test.cpp:113-121) both slices fit the LDS at once and nothing has to leave the CU:
//   one workgroup per ROW block (y slice = 64-bit fixed-point accumulators in LDS, as in pb_phase2_fixed);
//   it walks the block's NON-EMPTY column tiles (16 KiB of x each, double-buffered in LDS, re-staged from L2 / Infinity
//   Cache: neighbouring row blocks share their tiles) and streams the tile's entries — value + 16-bit local column +
//   16-bit local row = 12 B/nnz for fp64, the algorithmic bytes of CSR — multiplying out of one LDS slice and adding
//   into the other.  No global gather, no product buffer: HBM sees the matrix once, x a few times, y once.
// Pipeline: every lane keeps D trips of entry loads in flight in a static ring (as in spmv_pb.hip); the NEXT tile's x piece
// (16 bytes per lane) is requested one tile ahead and parked in registers; one workgroup barrier per tile.
// Sums: the same order-independent fixed-point scheme as pb_phase2_fixed, with the per-row exponent folded into the
// stored values when the image is built (a power of two: exact) — so the integers that are added are the ones the PB
// kernel adds, the result does not depend on the tile geometry, and the accuracy class is the NORM-wise one stated in
// lanczos_hip.h.  max|x| over the whole vector comes from a small pre-pass (tl_xmax_kernel: one read of x).
// (kTlTileBytes, one x tile = one 16-byte piece per lane of the workgroup, and kTlSlots, the x tiles resident in LDS: spmv_plan.hpp —
// the row-block length of the image follows from them)
constexpr int kTlXmaxParts = kXmaxParts;
constexpr int kTlDepth = 3;
constexpr int kTlNewPerTrip = 2;  // x tiles a trip may bring in

template <typename T>
__global__ __launch_bounds__(256) void tl_xmax_kernel(long long n, const T* __restrict__ x, double* __restrict__ parts, int aligned) {
  __shared__ double red[4];
  constexpr int V = 16 / (int)sizeof(T);  // elements per 16-byte piece
  constexpr int U = 4;                     // pieces per lane and trip, all requested before the first is used
  double m = 0.0;
  const long long nv = aligned ? n / V : 0;  // whole pieces (the vector is 16-byte aligned)
  const uint4* x4 = reinterpret_cast<const uint4*>(x);
  const long long stride = (long long)gridDim.x * 256;
  for (long long i0 = (long long)blockIdx.x * 256 + threadIdx.x; i0 < nv; i0 += U * stride) {
    uint4 piece[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long i = i0 + u * stride;
      piece[u] = x4[i < nv ? i : nv - 1];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      T el[V];
      __builtin_memcpy(el, &piece[u], sizeof(uint4));
#pragma unroll
      for (int q = 0; q < V; ++q) m = fmax(m, abs1(el[q]));
    }
  }
  for (long long i = nv * V + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) m = fmax(m, abs1(x[i]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  // (an Inf in x survives fmax; a NaN is dropped here and reaches the rows it touches through its products)
  if (threadIdx.x == 0) parts[blockIdx.x] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// ORDERED: component-wise accurate floating-point sums (ll_csr_options.accuracy = LL_ACCURACY_COMPONENTWISE, LL_PB_PHASE2=ordered)
// instead of the fixed-point ones — the y slice holds doubles, every product fl(a_ij 2^-e_i x_j) is added with ds_add_f64, the 16 waves
// of the workgroup in turn (a barrier between turns, as in pb_phase2<ORDERED>): a fixed order, so the result is the same bits on every
// launch, and its error is the reference's own fp64 row loop's, gamma_n sum_j |a_ij x_j| (the row's power-of-two scale is exact).  No
// max|x| pre-pass, no grid scale on the staged x.
template <typename T, int D, bool ALIGNED, bool ORDERED>
__global__ __launch_bounds__(kPbThreads) void tl_spmv_kernel(int rb_rows, int64_t n_local, int64_t n_cols,
                                                             const int32_t* __restrict__ tfirst,   // [nrb + 1]
                                                             const int32_t* __restrict__ tcol,     // [ntiles]
                                                             const int64_t* __restrict__ tquad,    // [ntiles + 1]
                                                             const T* __restrict__ val, const uint4* __restrict__ idx,
                                                             const int16_t* __restrict__ rexp,
                                                             const double* __restrict__ xmax_parts, int n_xmax,
                                                             const T* __restrict__ x, const T* __restrict__ xl,
                                                             T* __restrict__ y, double offset,
                                                             double* __restrict__ dot_partials,
                                                             const double* __restrict__ xnorm2, int xcd_order,
                                                             const int32_t* __restrict__ rb_map, int rb_first, int64_t col0) {
  // Sharded contexts launch the kernel twice: x holds the global columns [col0, n_cols) — the rank's own shard
  // for the row blocks whose tiles are all own-column tiles (they run under the all-gather), the gathered vector (col0 = 0) for
  // the others — and rb_map[rb_first + i] is the i-th row block of the launch.  Single GPU: rb_map = nullptr, col0 = 0.
  constexpr int R = scalar_traits<T>::reals;
  constexpr int C = kTlTileBytes / (int)sizeof(T);  // columns per tile
  constexpr int V = 16 / (int)sizeof(T);            // elements per 16-byte piece
  extern __shared__ double lds_raw[];
  long long* acc = reinterpret_cast<long long*>(lds_raw);                        // [rb_rows * R]
  T* xs = reinterpret_cast<T*>(acc + (size_t)rb_rows * R);                       // [kTlSlots][C]
  unsigned* bad = reinterpret_cast<unsigned*>(xs + kTlSlots * C);                       // [(rb_rows + 31) / 32] rows that met Inf / NaN
  __shared__ double red[kPbWaves + 1];
  const int tid = threadIdx.x;
  // XCD-aware row-block order: workgroups with equal blockIdx % 8 share an XCD and its L2, and neighbouring row blocks share
  // most of their x tiles (94 % for the banded config 3) — so every XCD takes a CONTIGUOUS eighth of the row blocks: the
  // 32 blocks it runs at a time then stage their tiles out of its own L2 instead of each fetching them through the fabric.
  int rb = blockIdx.x;
  if (xcd_order) {
    const int nb = gridDim.x, q = nb / kXcds, r = nb % kXcds;
    const int x = blockIdx.x % kXcds, l = blockIdx.x / kXcds;
    rb = x * q + min(x, r) + l;  // XCD x owns q + (x < r) consecutive blocks; a bijection on [0, nb)
  }
  if (rb_map) rb = rb_map[rb_first + rb];
  const int64_t row0 = (int64_t)rb * rb_rows;
  const int rows = (int)min((int64_t)rb_rows, n_local - row0);
  const int t0 = tfirst[rb], t1 = tfirst[rb + 1];
  const double xs_fac = xnorm2 ? 1.0 / sqrt(*xnorm2) : 1.0;  // unnormalised input (see pb_phase1)
  const long long q_begin = tquad[t0];
  // (the planner works on 32-bit quad numbers RELATIVE to the row block's first quad: its comparisons are scalar instructions;
  // 64-bit compares go through vector-register temporaries)
  const int q_end = (int)(tquad[t1] - q_begin);
  const int q_last = q_end > 0 ? q_end - 1 : 0;  // (the image is padded by one quad behind its end)

  // ---- trips.  A trip is kPbThreads consecutive quads of the row block's stream, WHEREVER the tile boundaries fall: a lane's
  // quad belongs to one tile (tiles are whole quads), the lanes of a trip to up to three consecutive tiles of the block's list.
  // (Round 5's first form ended every trip at the end of its tile: the tiles of the banded config 3 hold 0.75 trips, a quarter of
  // the lane slots of every trip carried no entry.)  Tile number tau of the list lives in slot (tau - t0) % kTlSlots of the x ring
  // in LDS.  A trip brings in at most kTlNewPerTrip new tiles — one 16-byte piece per lane and new tile, requested with the trip's
  // entries and parked in registers until the trip is consumed — and never more than the ring has room for next to the tiles of the
  // trip before it (which slower waves may still be reading): span(k) + new(k + 1) <= kTlSlots consecutive tiles, hence distinct
  // slots; a trip that would need more ends early, at a tile boundary.  ONE barrier per trip (new tiles visible; every wave has left
  // the trip before the previous one).  The planner below is uniform over the workgroup and runs at REQUEST time, D - 1 trips ahead.
  struct Plan {
    int q0, q1;  // quads [q0, q1) of the stream (relative to q_begin)
    int e1, e2;  // ends of tiles a and a + 1: a lane's tile is a + (g >= e1) + (g >= e2)
    int a;       // tile of the trip's first quad
    int first_new, n_new;
  };
  int pq = 0;       // next quad to plan
  int pcur = t0;    // tile that holds pq
  int pb = t0 - 1;  // last tile some earlier trip brought in
  int pspan = 0;    // tiles of the trip before
  auto tq = [&](int t) { return (int)(tquad[t] - q_begin); };
  auto plan = [&]() {
    Plan p;
    p.q0 = pq;
    p.a = pcur;
    p.first_new = pb + 1;
    if (pq >= q_end) {  // beyond the row block: nothing valid (q0 >= q_end ends the loop when it is consumed)
      p.q1 = pq;
      p.e1 = p.e2 = pq;
      p.n_new = 0;
      return p;
    }
    const int cap = min(kTlNewPerTrip, kTlSlots - pspan);  // >= 1: a trip spans at most three tiles
    const int bmax = min(t1 - 1, pb + cap);
    const int end = min(pq + kPbThreads, q_end);
    const int e1 = tq(min(pcur + 1, t1)), e2 = tq(min(pcur + 2, t1)), e3 = tq(min(pcur + 3, t1));
    int b = pcur;
    int eb = e1;
    if (b < bmax && eb < end) {
      ++b;
      eb = e2;
      if (b < bmax && eb < end) {
        ++b;
        eb = e3;
      }
    }
    p.e1 = e1;
    p.e2 = e2;
    p.q1 = min(end, eb);
    p.n_new = max(0, b - pb);
    pspan = b - pcur + 1;
    pb = max(pb, b);
    pq = p.q1;
    pcur = p.q1 == eb ? b + 1 : b;
    return p;
  };
  quad<T> v[D];
  uint4 ix[D], xp[D][kTlNewPerTrip];
  int gq[D];
  Plan pl[D];
  int ctn[D][kTlNewPerTrip];  // column tiles of the (up to) two new tiles of the trip
  // Every trip requests the SAME loads, unconditionally and in straight-line code — the lane's quad of values (2 x 16 B), its packed
  // indices (16 B) and its 16-byte piece of each of the trip's new x tiles (a trip with fewer new tiles requests its last one again:
  // a cache hit) — so the compiler can wait for exactly the oldest trip (s_waitcnt vmcnt(N), see spmv_pb.hip).
  auto issue = [&](int slot) {
    const Plan p = plan();
    pl[slot] = p;
    const int g = p.q0 + tid;
    const long long gc = q_begin + (g < q_last ? g : q_last);
    gq[slot] = g;
    v[slot] = load_quad<T>(val + 4 * gc);
    ix[slot] = idx[gc];
#pragma unroll
    for (int j = 0; j < kTlNewPerTrip; ++j) {
      // (a row block without tiles reads the table's padding entry; elements beyond the vector's end are never referenced)
      const int tj = max(t0, min(p.first_new + min(j, max(p.n_new - 1, 0)), t1 - 1));
      const int ct = tcol[tj];
      ctn[slot][j] = ct;
      const long long off = (long long)ct * C + (long long)tid * V;
      if constexpr (ALIGNED) {
        // a piece that would reach beyond the end is read V-aligned from the last whole piece position that is still inside
        // (n_cols >= V is guaranteed by the launcher) and shifted into place below (store_piece)
        // (... and never from in front of the buffer: only a re-requested or padding tile can lie there, and it is never stored)
        const long long lim = n_cols - V;
        const long long o = off <= lim ? off : lim;
        xp[slot][j] = *reinterpret_cast<const uint4*>(x + ((o >= col0 ? o : col0) - col0));
      } else {
        T el[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const long long o = off + q < n_cols ? off + q : n_cols - 1;
          el[q] = x[(o >= col0 ? o : col0) - col0];
        }
        __builtin_memcpy(&xp[slot][j], el, sizeof(uint4));
      }
    }
  };
  // (double / complex<double>: the scale 2^kx of the fixed-point grid rides on the staged x elements — one exact scaling per
  // element and tile instead of one v_ldexp_f64 per entry; |kx| <= 1000 and every product below 2^-1022 rounds to the integer 0
  // either way, so the integers are the same.  The float types keep the scaling behind their float product, whose underflow
  // threshold is within reach of the scale.)
  constexpr bool kFoldScale = sizeof(typename scalar_traits<T>::real) == 8 && !ORDERED;
  int kx = 0;  // set below, before the first tile is staged
  auto store_piece = [&](int tile, int ct, uint4 piece) {
    const int buf = (tile - t0) & (kTlSlots - 1);
    T el[V];
    __builtin_memcpy(el, &piece, sizeof(uint4));
    if constexpr (ALIGNED) {
      const long long off = (long long)ct * C + (long long)tid * V;
      const int d = (int)max(0ll, off - (n_cols - V));  // the piece was read d elements further left (only at the vector's end)
      if (d > 0) {
        T sh[V];
#pragma unroll
        for (int q = 0; q < V; ++q) sh[q] = zero<T>();
#pragma unroll
        for (int q = 0; q < V; ++q)
          if (q + d < V) sh[q] = el[q + d];
#pragma unroll
        for (int q = 0; q < V; ++q) el[q] = sh[q];
      }
    }
    if (xnorm2) {
#pragma unroll
      for (int q = 0; q < V; ++q) el[q] = rmul(xs_fac, el[q]);
    }
    if constexpr (kFoldScale) {
#pragma unroll
      for (int q = 0; q < V; ++q) el[q] = scale_pow2(el[q], kx);
    }
    uint4 out;
    __builtin_memcpy(&out, el, sizeof(uint4));
    reinterpret_cast<uint4*>(xs + (size_t)buf * C)[tid] = out;
  };
  // ---- accumulators, scale of the fixed-point grid
  for (int i = tid; i < rb_rows * R; i += kPbThreads) acc[i] = 0;
  for (int i = tid; i < (rb_rows + 31) / 32; i += kPbThreads) bad[i] = 0u;
  int e_x = -2000;  // x == 0: any scale does
  if constexpr (!ORDERED) {
    double m = 0.0;
    for (int i = tid; i < n_xmax; i += kPbThreads) m = fmax(m, xmax_parts[i]);
    const double t = pb_block_max(m, red) * xs_fac;  // (ends with a barrier: the LDS stores above are visible)
    if (t > 0.0 && isfinite(t)) (void)frexp(t, &e_x);
    else if (!(t == 0.0)) e_x = kPbXInf;
    // integer = (PRE-SCALED value * x) * 2^kx; row i's sum is acc_i * 2^(er_i - kx)   (pb_phase2_fixed: k = 62 - (er + e_x + 1))
    kx = e_x == kPbXInf ? 0 : max(-1000, min(1000, 61 - e_x));
  } else {
    __syncthreads();  // the accumulators are zero before the first add
  }
  double* const accd = reinterpret_cast<double*>(acc);  // ORDERED: the same slice as doubles
  const int wave = tid >> 6;

  // (No branch on `valid`: a lane beyond the end of its trip holds a re-read of a valid quad and adds ZERO to that quad's
  // rows — every trip then waits for and uses its loads on every path, which keeps the wait counts of the ring exact.)
  auto consume = [&](const quad<T>& vv, const uint4& ii, bool valid, int buf) {
    const T* xb = xs + (size_t)buf * C;
    const unsigned w4[4] = {ii.x, ii.y, ii.z, ii.w};
    if constexpr (ORDERED) {
      T pe[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) pe[e] = mul(vv.e[e], xb[w4[e] & 0xffffu]);
      for (int w = 0; w < kPbWaves; ++w) {  // the waves add in turn: a fixed order (Inf / NaN travel through the sums by themselves)
        if (wave == w && valid) {
#pragma unroll
          for (int e = 0; e < 4; ++e) lds_add_elem<T>(accd, (int)(w4[e] >> 16), pe[e]);
        }
        __syncthreads();
      }
      return;
    }
    // the four x elements first, in one batch of LDS reads: behind the first atomic the compiler may not move a read of the
    // same LDS array forward (it cannot prove that xs and acc do not overlap), and entry by entry every read's latency is exposed
    T xe[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) xe[e] = xb[w4[e] & 0xffffu];
    unsigned badmask = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned lr = w4[e] >> 16;
      const T p = mul(vv.e[e], xe[e]);
      double pr[R];
      if constexpr (scalar_traits<T>::is_complex) {
        pr[0] = (double)p.re;
        pr[1] = (double)p.im;
      } else {
        pr[0] = (double)p;
      }
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const double sc = kFoldScale ? pr[q] : ldexp(pr[q], kx);
        const bool good = fabs(sc) < 9.0e18;  // false for Inf / NaN too; fixed_round's value is not used then
        if (!good) badmask |= 1u << e;
        atomicAdd(reinterpret_cast<unsigned long long*>(&acc[R * lr + q]), (valid && good) ? (unsigned long long)fixed_round(sc) : 0ull);
      }
    }
    // rows that met an Inf / NaN (rare: one wave-uniform branch per trip instead of a masked LDS OR per entry)
    if (__builtin_expect(__any(valid && badmask != 0u), 0)) {
      if (valid) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((badmask >> e) & 1u) {
            const unsigned lr = w4[e] >> 16;
            atomicOr(&bad[lr >> 5], 1u << (lr & 31));
          }
      }
    }
  };
  // (The first D - 1 trips are requested HERE, right in front of the loop and after everything else of the prologue has
  // drained: the loop is then entered with exactly the pending loads its back edge carries, and the compiler's wait counts
  // stay exact in every phase; requested earlier, the merge of the two paths costs a full drain in the loop's first phase.)
#pragma unroll
  for (int d = 0; d < D - 1; ++d) {
    __builtin_amdgcn_sched_barrier(0);  // keep the trips' loads in trip order (the wait counts of the loop assume it)
    issue(d);
  }
  __builtin_amdgcn_sched_barrier(0);
  auto step = [&](auto ph) -> bool {
    constexpr int PH = decltype(ph)::value;
    const Plan p = pl[PH];
    if (p.q0 >= q_end) return false;  // uniform over the workgroup
    if (p.n_new > 0) store_piece(p.first_new, ctn[PH][0], xp[PH][0]);
    if (p.n_new > 1) store_piece(p.first_new + 1, ctn[PH][1], xp[PH][1]);
    __syncthreads();
    const int g = gq[PH];
    const bool valid = g < p.q1;
    const int buf = (p.a - t0 + (g >= p.e1 ? 1 : 0) + (g >= p.e2 ? 1 : 0)) & (kTlSlots - 1);
    const quad<T> vv = v[PH];
    const uint4 ii = ix[PH];
    issue((PH + D - 1) % D);
    consume(vv, ii, valid, buf);
    return true;
  };
  // (The waitcnt pass merges the pending loads of the prologue and of the back edge conservatively at the loop header: the FIRST
  // trip behind it drains the memory pipeline, one trip in D.  Two rounds of the ring per loop iteration halve that and change
  // nothing measurable — 0.548 against 0.550 ms on the banded config 3, profiles/r05_tl_ring_two_rounds_ab.txt: the other waves
  // of the workgroup cover the drain — so the loop keeps one round.)
  for (;;) {
    if (!step(std::integral_constant<int, 0>{})) break;
    if (!step(std::integral_constant<int, 1>{})) break;
    if constexpr (D > 2) {
      if (!step(std::integral_constant<int, 2>{})) break;
    }
    if constexpr (D > 3) {
      if (!step(std::integral_constant<int, 3>{})) break;
    }
  }
  __syncthreads();
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  auto value = [&](int i, const T&, int er) {  // er: the row's exponent (requested ahead, see the epilogue)
    if constexpr (ORDERED) {  // 2^er restores the row's scale (exact); a row whose absolute sum is not finite has no usable image
      acc_t<T> a;
      if constexpr (scalar_traits<T>::is_complex)
        a = er == 32767 ? zc{nan, nan} : zc{ldexp(accd[2 * i], er), ldexp(accd[2 * i + 1], er)};
      else
        a = er == 32767 ? nan : ldexp(accd[i], er);
      return a;
    }
    const bool unusable = er == 32767 || e_x == kPbXInf || ((bad[i >> 5] >> (i & 31)) & 1u);
    const int back = er - kx;  // 2^back restores the row's scale (empty rows: er = -1100, acc = 0)
    acc_t<T> a;
    if constexpr (scalar_traits<T>::is_complex)
      a = unusable ? zc{nan, nan} : zc{ldexp((double)acc[2 * i], back), ldexp((double)acc[2 * i + 1], back)};
    else
      a = unusable ? nan : ldexp((double)acc[i], back);
    return a;
  };
  pb_phase2_epilogue<T>(rb, row0, rows, xl, y, offset, dot_partials, red, xnorm2, value, [&](int i) { return (int)rexp[row0 + i]; });
}

namespace {
template <typename T> size_t tl_lds_bytes(int rb_rows) {
  return (size_t)rb_rows * sizeof(acc_t<T>) + (size_t)kTlSlots * kTlTileBytes + (size_t)((rb_rows + 31) / 32) * sizeof(unsigned) + 16;
}
template <typename T> void tl_opt_in_lds() {
  static std::atomic<unsigned long long> mask{0};
  once_per_device(mask, [] {
    pb_opt_in(&tl_spmv_kernel<T, kTlDepth, true, false>);
    pb_opt_in(&tl_spmv_kernel<T, kTlDepth, false, false>);
    pb_opt_in(&tl_spmv_kernel<T, kTlDepth, true, true>);
    pb_opt_in(&tl_spmv_kernel<T, kTlDepth, false, true>);
  });
}

// One launch over the row blocks [rb_first, rb_first + rb_count) of the image's order (op.tl.rbmap; identity without a map); x holds the
// global columns [col0, col_end), x_local the rank's own rows; the fixed-point class reads n_xmax maxima of |x| from op.tl.xmax.
template <typename T>
void tl_launch_rows(const ll_operator& op, int rb_first, int rb_count, const T* x, int64_t col0, int64_t col_end, const T* x_local, T* y,
                    double offset, double* dot_partials, hipStream_t s, const double* xnorm2, int n_xmax) {
  if (rb_count <= 0) return;
  constexpr int64_t V = (int64_t)(16 / sizeof(T));
  // 16-byte pieces of x: the fast form needs an aligned window of at least one piece that starts on a piece boundary
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && col0 % V == 0 && col_end - col0 >= V;
#define LL_TL_LAUNCH(AL, ORD)                                                                                                         \
  hipLaunchKernelGGL((tl_spmv_kernel<T, kTlDepth, AL, ORD>), dim3(rb_count), dim3(kPbThreads), tl_lds_bytes<T>(op.tl.rb_rows), s,      \
                     op.tl.rb_rows, op.n_local, col_end, op.tl.first.get(), op.tl.col.get(), op.tl.quad.get(), (const T*)op.tl.val.get(),              \
                     (const uint4*)op.tl.idx.get(), op.tl.rexp.get(), op.tl.xmax.get(), n_xmax, x, x_local, y, offset, dot_partials, xnorm2,       \
                     op.ctx->tune.tl_xcd_order ? 1 : 0, (const int32_t*)op.tl.rbmap.get(), rb_first, col0)
  if (aligned && op.tl.ordered) LL_TL_LAUNCH(true, true);
  else if (aligned) LL_TL_LAUNCH(true, false);
  else if (op.tl.ordered) LL_TL_LAUNCH(false, true);
  else LL_TL_LAUNCH(false, false);
#undef LL_TL_LAUNCH
  LL_HIP(hipGetLastError());
}
}  // namespace

// x = the WHOLE vector (single GPU; sharded: the gathered vector, x + row_begin the rank's own rows): max |x|, then every row block.
template <typename T>
int launch_spmv_tiled(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                      const double* xnorm2) {
  if (op.tl.nrb <= 0) return 0;
  tl_opt_in_lds<T>();
  const int xgrid = (int)std::max<int64_t>(1, std::min<int64_t>(kTlXmaxParts, (op.n + 255) / 256));
  if (!op.tl.ordered)  // (the component-wise form has no fixed-point grid to scale: no max|x| pre-pass)
    hipLaunchKernelGGL((tl_xmax_kernel<T>), dim3(xgrid), dim3(256), 0, s, (long long)op.n, x, op.tl.xmax.get(),
                       (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? 1 : 0);
  tl_launch_rows<T>(op, 0, op.tl.nrb, x, 0, op.n, x + op.row_begin, y, offset, dot_partials, s, xnorm2, xgrid);
  return op.tl.nrb;
}

// Sharded contexts (engine.cpp, Engine::gather_x): the maximum of |x| over the rank's own shard, one double at
// op.tl.xmax[tl_xmax_local_slot()] — the ranks' maxima are then all-gathered into op.tl.xmax[0, nranks), the table the kernel
// folds (a maximum does not depend on how the vector is cut, so every partition scales its fixed-point grid exactly like one GPU).
template <typename T> void launch_tl_xmax_local(const ll_operator& op, const T* x_own, hipStream_t s) {
  if (op.tl.nrb <= 0 || op.tl.ordered) return;
  double* parts = op.tl.xmax.get() + kTlXmaxParts;
  const int g = (int)std::max<int64_t>(1, std::min<int64_t>(kTlXmaxParts, (op.n_local + 255) / 256));
  hipLaunchKernelGGL((tl_xmax_kernel<T>), dim3(g), dim3(256), 0, s, (long long)op.n_local, x_own, parts,
                     (reinterpret_cast<uintptr_t>(x_own) & 15) == 0 ? 1 : 0);
  hipLaunchKernelGGL((tl_xmax_kernel<double>), dim3(1), dim3(256), 0, s, (long long)g, (const double*)parts, parts + kTlXmaxParts, 1);
  LL_HIP(hipGetLastError());
}
int tl_xmax_local_slot() { return 2 * kTlXmaxParts; }

// pass 0: the row blocks whose tiles are all own-column tiles (x = the rank's shard, global columns [col0, col_end));
// pass 1: the others (x = the gathered vector, col0 = 0).  n_xmax maxima (one per rank) wait in op.tl.xmax.
template <typename T>
int launch_spmv_tiled_pass(const ll_operator& op, int pass, const T* x, int64_t col0, int64_t col_end, const T* x_local, T* y,
                           double offset, double* dot_partials, hipStream_t s, const double* xnorm2, int n_xmax) {
  if (op.tl.nrb <= 0) return 0;
  tl_opt_in_lds<T>();
  const int first = pass == 0 ? 0 : op.tl.n_interior;
  const int count = pass == 0 ? op.tl.n_interior : op.tl.nrb - op.tl.n_interior;
  tl_launch_rows<T>(op, first, count, x, col0, col_end, x_local, y, offset, dot_partials, s, xnorm2, n_xmax);
  return op.tl.nrb;
}

template <typename T> int launch_x_max(int64_t n, const T* x, double* parts, hipStream_t s) {
  const int g = (int)std::max<int64_t>(1, std::min<int64_t>(kTlXmaxParts, (n + 255) / 256));
  hipLaunchKernelGGL((tl_xmax_kernel<T>), dim3(g), dim3(256), 0, s, (long long)n, x, parts,
                     (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? 1 : 0);
  LL_HIP(hipGetLastError());
  return g;
}

#define LL_INST_TL(T)                                                                                               \
  template int launch_spmv_tiled<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const double*);  \
  template void launch_tl_xmax_local<T>(const ll_operator&, const T*, hipStream_t);                                 \
  template int launch_spmv_tiled_pass<T>(const ll_operator&, int, const T*, int64_t, int64_t, const T*, T*, double, \
                                         double*, hipStream_t, const double*, int);                                 \
  template int launch_x_max<T>(int64_t, const T*, double*, hipStream_t);
LL_FOR_EACH_SCALAR(LL_INST_TL)

}  // namespace ll
