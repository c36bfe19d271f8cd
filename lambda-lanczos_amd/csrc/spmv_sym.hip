// SpMV of a symmetric / Hermitian matrix stored as ONE triangle (ll_op_create_csr_sym_*, LL_SPMV_SYM):
//   A = T + T^T - diag(T)  (real types),   A = T + T^H - diag(T)  (complex types; the diagonal is used as stored).
//
// One workgroup per ROW block I (rb_rows rows) owns y_I as 64-bit fixed-point accumulators in LDS, like pb_phase2_fixed and
// the tiled kernel.  Its stream holds every stored entry (k, j) with an end in I: the direct product a_kj x_j goes to row k when
// k lies in I, the mirrored product conj(a_kj) x_k to row j when j lies in I and j != k.  An entry whose two ends lie in
// different blocks is in both blocks' streams (built once on the host, sym_build).  The x window [row0 - halo, row0 + rb_rows +
// halo) is staged in LDS once and every product of the stream reads x from there: no product buffer, no global atomics.  halo is
// the half-bandwidth of all but at most 1/16 of the entries (sym_halo_for); the rest — e.g. the corners of a periodic band —
// are FAR entries of a short second list with one product each and x read from memory.  HBM sees the triangle (plus the
// entries read twice), x about (rb_rows + 2 halo) / rb_rows times, y once.
//
// Sums: the fixed-point class of pb_phase2_fixed.  Every product is rounded to the grid of its DESTINATION row,
// q_i = 2^(er_i + e_x + 1 - 62), where sum_j |a_ij| < 2^er_i over the FULL row of A (computed when the operator is created,
// on the expanded matrix in increasing column order: pb_rowexp_kernel, spmv_image_build.hip) and max|x| < 2^e_x (tl_xmax_kernel pre-pass, spmv_tiled.hip).  The
// mirrored product is the same multiply the full-storage kernels apply to the stored a_jk = conj(a_kj) (negating an imaginary
// part is exact), so the integers added are the ones pb_phase2_fixed adds on the expanded matrix and y is the same bits.
// The epilogue (offset x_i, the dot partials, the scaled input) is pb_phase2_epilogue itself.
#include <algorithm>
#include <atomic>
#include <vector>

#include "dev_helpers.hpp"
#include "fixed_round.hpp"
#include "ll_internal.hpp"
#include "spmv_shared.hpp"

namespace ll {

namespace {
constexpr int kSymBadRow = 32767;                // grid exponent of a row whose result is NaN
constexpr int kSymLdsCap = 160 * 1024 - 2048;    // dynamic LDS of one workgroup (the static part and slack stay free)
constexpr int kSymMinRows = 256;
constexpr int kSymMaxWindow = 65534;             // window indices are 16-bit; 0xffff marks padding
constexpr uint32_t kSymPad = 0xffffffffu;

__host__ __device__ inline size_t sym_align16(size_t b) { return (b + 15) & ~(size_t)15; }
template <typename T> size_t sym_lds_bytes(int rb_rows, int halo) {
  return sym_align16((size_t)rb_rows * sizeof(acc_t<T>)) + sym_align16((size_t)(rb_rows + 2 * halo) * sizeof(T)) +
         sym_align16((size_t)rb_rows * sizeof(int16_t)) + (size_t)((rb_rows + 31) / 32) * sizeof(unsigned);
}
}  // namespace

template <typename T> __device__ __forceinline__ T sym_conj(const T& a) {
  if constexpr (scalar_traits<T>::is_complex) return T{a.re, -a.im};
  else return a;
}

template <typename T>
__global__ __launch_bounds__(kPbThreads) void sym_spmv_kernel(int rb_rows, int halo, int64_t n,
                                                              const int64_t* __restrict__ qptr,  // [nrb + 1]
                                                              const T* __restrict__ val, const uint4* __restrict__ idx,
                                                              const int16_t* __restrict__ rexp,
                                                              const double* __restrict__ xmax_parts, int n_xmax,
                                                              const T* __restrict__ x, T* __restrict__ y, double offset,
                                                              double* __restrict__ dot_partials,
                                                              const double* __restrict__ xnorm2,
                                                              const int64_t* __restrict__ fptr, const T* __restrict__ fval,
                                                              const uint32_t* __restrict__ fdst, const int32_t* __restrict__ fsrc,
                                                              const T* __restrict__ diag) {
  constexpr int R = scalar_traits<T>::reals;
  const int win = rb_rows + 2 * halo;
  extern __shared__ double lds_raw[];
  char* base = reinterpret_cast<char*>(lds_raw);
  long long* acc = reinterpret_cast<long long*>(base);                                      // [rb_rows * R]
  base += sym_align16((size_t)rb_rows * sizeof(acc_t<T>));
  T* xw = reinterpret_cast<T*>(base);                                                       // [win]: x[row0 - halo + l]
  base += sym_align16((size_t)win * sizeof(T));
  int16_t* ex = reinterpret_cast<int16_t*>(base);                                           // [rb_rows]: grid exponent k_i
  base += sym_align16((size_t)rb_rows * sizeof(int16_t));
  unsigned* bad = reinterpret_cast<unsigned*>(base);                                        // rows that met Inf / NaN
  __shared__ double red[kPbWaves + 1];
  const int tid = threadIdx.x;
  const int rb = blockIdx.x;
  const int64_t row0 = (int64_t)rb * rb_rows;
  const int rows = (int)min((int64_t)rb_rows, n - row0);
  const int64_t wbase = row0 - halo;
  const double xs_fac = xnorm2 ? 1.0 / sqrt(*xnorm2) : 1.0;  // unnormalised input (see pb_phase1)
  const long long q0 = qptr[rb], q1 = qptr[rb + 1];

  // ---- scale of the fixed-point grid (as in the tiled kernel), accumulators, the x window
  double m = 0.0;
  for (int i = tid; i < n_xmax; i += kPbThreads) m = fmax(m, xmax_parts[i]);
  const double t = pb_block_max(m, red) * xs_fac;
  int e_x = -2000;  // x == 0: any scale does
  if (t > 0.0 && isfinite(t)) (void)frexp(t, &e_x);
  else if (!(t == 0.0)) e_x = kPbXInf;
  for (int i = tid; i < rb_rows * R; i += kPbThreads) acc[i] = 0;
  for (int i = tid; i < (rb_rows + 31) / 32; i += kPbThreads) bad[i] = 0u;
  for (int i = tid; i < rb_rows; i += kPbThreads) {
    int k = 0;
    if (i < rows) {
      const int er = rexp[row0 + i];
      k = (er == 32767 || e_x == kPbXInf) ? kSymBadRow : max(-1000, min(1000, 62 - (er + e_x + 1)));  // pb_phase2_fixed's k
    }
    ex[i] = (int16_t)k;
  }
  // (all loads of a round are requested before the first LDS store: a load -> store loop is a chain of memory latencies)
  constexpr int SU = 8;
  for (int l0 = 0; l0 < win; l0 += SU * kPbThreads) {
    T v[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int64_t g = wbase + l0 + u * kPbThreads + tid;
      v[u] = x[g < 0 ? 0 : (g < n ? g : n - 1)];
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int l = l0 + u * kPbThreads + tid;
      const int64_t g = wbase + l;
      if (l < win) xw[l] = (g >= 0 && g < n) ? rmul(xs_fac, v[u]) : zero<T>();
    }
  }
  __syncthreads();

  // ---- the stream: (4 values, 4 packed window indices) per lane and quad, two quads per lane requested before either is used
  auto add_row = [&](int r, const T& p) {
    const int k = ex[r];
    if (k == kSymBadRow) return;
    double pr[R];
    if constexpr (scalar_traits<T>::is_complex) {
      pr[0] = (double)p.re;
      pr[1] = (double)p.im;
    } else {
      pr[0] = (double)p;
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double sc = ldexp(pr[q], k);  // = pr * 2^k exactly as pb_phase2_fixed's multiply by pow2(k)
      if (!(fabs(sc) < 9.0e18)) atomicOr(&bad[r >> 5], 1u << (r & 31));
      else atomicAdd(reinterpret_cast<unsigned long long*>(&acc[R * r + q]), (unsigned long long)fixed_round(sc));
    }
  };
  auto consume = [&](const quad<T>& v, const uint4& w) {
    const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int lo = (int)(ws[e] & 0xffffu), hi = (int)(ws[e] >> 16);  // window index of the entry's row k / column j
      const int kr = lo - halo, jr = hi - halo;                        // local rows (padding: both beyond the block)
      if ((unsigned)kr < (unsigned)rows) add_row(kr, mul(v.e[e], xw[hi]));
      if ((unsigned)jr < (unsigned)rows && lo != hi) add_row(jr, mul(sym_conj(v.e[e]), xw[lo]));
    }
  };
  // the diagonal (its first entry per row; the same integers as if it travelled in the stream)
  for (int i = tid; i < rows; i += kPbThreads) add_row(i, mul(diag[row0 + i], xw[halo + i]));
  for (long long q = q0 + tid; q < q1; q += 2 * kPbThreads) {
    const long long qb = q + kPbThreads;
    const long long qc = qb < q1 ? qb : q;
    const quad<T> v0 = load_quad<T>(val + 4 * q);
    const uint4 w0 = idx[q];
    const quad<T> v1 = load_quad<T>(val + 4 * qc);
    const uint4 w1 = idx[qc];
    consume(v0, w0);
    if (qb < q1) consume(v1, w1);
  }
  // the far entries: one product each, the source element of x from memory (scaled like the staged window)
  const long long f1 = fptr[rb + 1];
  for (long long e = fptr[rb] + tid; e < f1; e += kPbThreads) {
    const T a = fval[e];
    const uint32_t d = fdst[e];
    const T xs = rmul(xs_fac, x[fsrc[e]]);
    add_row((int)(d & 0x7fffffffu), mul((d >> 31) ? sym_conj(a) : a, xs));
  }
  __syncthreads();
  auto value = [&](int i, const T&, int) {
    const int k = ex[i];
    const bool unusable = k == kSymBadRow || ((bad[i >> 5] >> (i & 31)) & 1u);
    const double back = unusable ? __longlong_as_double(0x7ff8000000000000ll) : pow2(-k);  // NaN for unusable rows
    acc_t<T> a;
    if constexpr (scalar_traits<T>::is_complex) a = zc{(double)acc[2 * i] * back, (double)acc[2 * i + 1] * back};
    else a = (double)acc[i] * back;
    return a;
  };
  pb_phase2_epilogue<T>(rb, row0, rows, x, y, offset, dot_partials, red, xnorm2, value, [&](int) { return 0; });
}

namespace {
template <typename T> void sym_opt_in_lds() {
  static std::atomic<unsigned long long> mask{0};
  int dev = 0;
  LL_HIP(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (mask.load(std::memory_order_acquire) & bit) return;
  LL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&sym_spmv_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             kSymLdsCap));
  mask.fetch_or(bit, std::memory_order_release);
}
}  // namespace

// The window's halo h: the smallest h such that at most 1/16 of the entries lie further than h from the diagonal (-1: no such
// h within the 16-bit window indices).
int64_t sym_halo_for(const int64_t* rp, const int32_t* ci, int64_t n) {
  constexpr int64_t kMax = kSymMaxWindow / 2;
  std::vector<int64_t> hist((size_t)kMax + 2, 0);  // entries per distance |i - j|, everything beyond kMax in the last bin
  for (int64_t i = 0; i < n; ++i)
    for (int64_t p = rp[i]; p < rp[i + 1]; ++p) {
      const int64_t d = ci[p] > i ? ci[p] - i : i - ci[p];
      ++hist[(size_t)std::min(d, kMax + 1)];
    }
  const int64_t allowed = rp[n] / 16;
  int64_t beyond = hist[(size_t)kMax + 1];  // entries with a distance > h, for h = kMax, kMax - 1, ...
  if (beyond > allowed) return -1;
  int64_t h = kMax;
  while (h > 0 && beyond + hist[(size_t)h] <= allowed) beyond += hist[(size_t)h--];
  return h;
}

// Eligibility: the largest power-of-two row block (256 ... 16384 rows, no larger than n needs) whose accumulators, grid exponents
// and x window fit the LDS and which is at least as tall as the halo (otherwise most entries would be read twice); and a halo
// of at most 2048, or of at most n / 4, or one row block that holds the whole matrix (a band wider than 2048 and than a quarter
// of the matrix has no locality left: the full-storage kernels serve it).  Every half-bandwidth <= 2048 is eligible for all
// four types (float: 8192-row blocks, double and complex float: 4096, complex double: 2048); a random matrix is not (a small
// one, n = 5000: halo 3750 > 2048 and > n / 4).
template <typename T> int sym_rows_for(int64_t n, int64_t halo) {
  if (halo < 0 || halo > kSymMaxWindow / 2) return 0;
  int64_t need = kSymMinRows;
  while (need < n && need < 16384) need *= 2;
  for (int64_t r = need; r >= kSymMinRows; r /= 2)
    if (r >= halo && r + 2 * halo <= kSymMaxWindow && sym_lds_bytes<T>((int)r, (int)halo) <= (size_t)kSymLdsCap)
      return (r >= n || halo <= 2048 || 4 * halo <= n) ? (int)r : 0;
  return 0;
}

template <typename T> void sym_build(const ll_operator& op, SymImage& im, const int64_t* rp, const int32_t* ci, const T* va) {
  ll_context* ctx = op.ctx;
  const int64_t n = op.n, R = im.rb_rows, H = im.halo;
  LL_REQUIRE(R > 0 && R + 2 * H <= kSymMaxWindow, "internal: one-triangle image geometry");
  const int64_t nrb = (n + R - 1) / R;
  LL_REQUIRE(nrb < (int64_t)0x7fffffff, "too many row blocks");
  // Entry (i, j), i = its row, in block b: a WINDOW entry when its other end lies in b's x window (both products of an entry with
  // both ends in b come from one window entry), otherwise a FAR entry of b (one product, x from memory).
  auto in_win = [&](int64_t b, int64_t g) { return g >= b * R - H && g < b * R + R + H; };
  std::vector<T> hd((size_t)n);  // the first diagonal entry of every row (zero: none); the entry leaves the streams
  std::vector<int64_t> dpos((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t p = rp[i]; p < rp[i + 1]; ++p)
      if (ci[p] == i) {
        hd[(size_t)i] = va[p];
        dpos[(size_t)i] = p;
        break;
      }
  std::vector<int64_t> qptr((size_t)nrb + 1, 0), fptr((size_t)nrb + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t bi = i / R;
    for (int64_t p = rp[i]; p < rp[i + 1]; ++p) {
      if (p == dpos[(size_t)i]) continue;
      const int64_t j = ci[p], bj = j / R;
      ++(in_win(bi, j) ? qptr : fptr)[(size_t)bi + 1];
      if (bj != bi) ++(in_win(bj, i) ? qptr : fptr)[(size_t)bj + 1];
    }
  }
  std::vector<int64_t> pos((size_t)nrb), fpos((size_t)nrb);
  for (int64_t b = 0; b < nrb; ++b) {
    pos[(size_t)b] = 4 * qptr[(size_t)b];
    qptr[(size_t)b + 1] = qptr[(size_t)b] + (qptr[(size_t)b + 1] + 3) / 4;
    fpos[(size_t)b] = fptr[(size_t)b];
    fptr[(size_t)b + 1] += fptr[(size_t)b];
  }
  const size_t entries = (size_t)(4 * qptr[(size_t)nrb]), far = (size_t)fptr[(size_t)nrb];
  std::vector<T> hv(std::max<size_t>(entries, 4));  // value-initialised: zero (padding)
  std::vector<uint32_t> hi(std::max<size_t>(entries, 4), kSymPad);
  std::vector<T> fv(std::max<size_t>(far, 1));
  std::vector<uint32_t> fd(std::max<size_t>(far, 1));
  std::vector<int32_t> fs(std::max<size_t>(far, 1));
  auto put = [&](int64_t b, int64_t i, int64_t j, const T& v) {
    const int64_t wb = b * R - H;  // window base of block b
    const size_t q = (size_t)pos[(size_t)b]++;
    hv[q] = v;
    hi[q] = (uint32_t)(i - wb) | ((uint32_t)(j - wb) << 16);
  };
  auto put_far = [&](int64_t b, int64_t dst, int64_t src, bool mirrored, const T& v) {
    const size_t q = (size_t)fpos[(size_t)b]++;
    fv[q] = v;
    fd[q] = (uint32_t)(dst - b * R) | (mirrored ? 0x80000000u : 0u);
    fs[q] = (int32_t)src;
  };
  for (int64_t i = 0; i < n; ++i) {
    const int64_t bi = i / R;
    for (int64_t p = rp[i]; p < rp[i + 1]; ++p) {
      if (p == dpos[(size_t)i]) continue;
      const int64_t j = ci[p], bj = j / R;
      if (in_win(bi, j)) put(bi, i, j, va[p]);
      else put_far(bi, i, j, false, va[p]);
      if (bj != bi) {
        if (in_win(bj, i)) put(bj, i, j, va[p]);
        else put_far(bj, j, i, true, va[p]);
      }
    }
  }
  auto up = [&](auto& dst, const auto& v, const char* what) {
    using E = typename std::decay_t<decltype(v)>::value_type;
    dst = ctx->dev_alloc<E>(v.size(), what);
    LL_HIP(hipMemcpy(dst.get(), v.data(), v.size() * sizeof(E), hipMemcpyHostToDevice));
  };
  up(im.qptr, qptr, "one-triangle image: row block offsets");
  up(im.val, hv, "one-triangle image: values");
  up(im.idx, hi, "one-triangle image: indices");
  up(im.fptr, fptr, "one-triangle image: far entry offsets");
  up(im.fval, fv, "one-triangle image: far values");
  up(im.fdst, fd, "one-triangle image: far destinations");
  up(im.fsrc, fs, "one-triangle image: far sources");
  up(im.diag, hd, "one-triangle image: diagonal");
  im.rexp = ctx->dev_alloc<int16_t>((size_t)std::max<int64_t>(n, 8), "one-triangle image: row exponents");
  im.xmax = ctx->dev_alloc<double>((size_t)kXmaxParts, "one-triangle image: maxima of |x|");
  im.nrb = (int)nrb;
}

template <typename T>
int launch_spmv_sym(const ll_operator& op, const T* x, T* y, double offset, double* dot_partials, hipStream_t s,
                    const double* xnorm2) {
  if (op.sym.nrb <= 0) return 0;
  sym_opt_in_lds<T>();
  const int nx = launch_x_max<T>(op.n, x, op.sym.xmax.get(), s);
  // (the kernel that publishes an iteration's scalars may complete that iteration's event itself: ll_context::stop_next)
  hipEvent_t stop = take_stop(op.ctx);
  LL_LAUNCH_STOP(stop, (sym_spmv_kernel<T>), dim3(op.sym.nrb), dim3(kPbThreads), sym_lds_bytes<T>(op.sym.rb_rows, op.sym.halo), s,
                 op.sym.rb_rows, op.sym.halo, op.n, (const int64_t*)op.sym.qptr.get(), (const T*)op.sym.val.get(),
                 (const uint4*)op.sym.idx.get(), (const int16_t*)op.sym.rexp.get(), (const double*)op.sym.xmax.get(), nx, x, y, offset,
                 dot_partials, xnorm2, (const int64_t*)op.sym.fptr.get(), (const T*)op.sym.fval.get(), (const uint32_t*)op.sym.fdst.get(),
                 (const int32_t*)op.sym.fsrc.get(), (const T*)op.sym.diag.get());
  LL_HIP(hipGetLastError());
  return op.sym.nrb;
}

#define LL_INST_SYM(T)                                                                                               \
  template int sym_rows_for<T>(int64_t, int64_t);                                                                   \
  template void sym_build<T>(const ll_operator&, SymImage&, const int64_t*, const int32_t*, const T*);              \
  template int launch_spmv_sym<T>(const ll_operator&, const T*, T*, double, double*, hipStream_t, const double*);
LL_FOR_EACH_SCALAR(LL_INST_SYM)

}  // namespace ll
