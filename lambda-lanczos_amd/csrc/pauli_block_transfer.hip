// A sum of Pauli strings between two momentum blocks of a ring, for gfx950 (ll_pauli_block_transfer, lanczos_hip.h): with B_s, B_t
// the isometries of the source block (momentum m_s) and the target block (m_t),
//   out = B_t^H (sum_j coef_j P_j) B_s c
// without a vector of the full space.  The strings need not commute with the translation: the plan
// (pauli_block_transfer_plan.hpp) replaces them by their momentum-q component Pbar_q, q = m_t - m_s, whose strings (X', z') with
// merged complex weights come as term tables like a Hamiltonian's, and Pbar_q maps block m_s wholly into block m_t:
//   out(a) = sum_{(X', z')} weight w_a(X', z') sqrt(R_a / R_b) e^(-2 pi i m_s l / L) c_b,      a ^ X' = T^l b
// with a, R_a from the TARGET's tables and b, l, R_b, the in-block test (m_s R_b = 0 mod L; in a sector: the partner keeps
// n_down set bits) and the phase table from the SOURCE's.
//
// The kernel is pauli_basis_kernel's geometry (pauli_basis.hpp): a workgroup takes blocks of 2^b target indices in a grid-stride
// loop (b: the tuning key of the target's own apply), a lane carries kPauliLaneStates of them through the group loop; the term
// tables are plain __restrict__ parameters (wave-uniform loads on the scalar path); per group the weights as pauli_basis_kernel
// forms them, then the Partner's add_group: one double fma per group in ascending mask order, one rounding to T.  It cannot be
// pauli_basis_kernel itself — that kernel reads x[i] at the OUTPUT's index —, and the X = 0 shortcut of the full-space policy
// does not carry over: the partner is a itself, but its number in the source basis has to be searched and the source block may
// exclude it.  The two Partner policies below hold both blocks' tables and call the ONE locate / pauli_bucket_search.
// Epilogue: |out(a)|^2 of the rounded value, summed per workgroup in a fixed tree (block_sum), one partial per workgroup, folded
// over the workgroups in a fixed order by reduce_cols_kernel.  The same bits run to run, for every alignment and wherever c and
// out live; the partial sums depend on the block size and the grid alone.
//
// Bytes: (sizeof(T) + 5) D_t (out, reps, orbit lengths of the target) plus per group what the source policy's apply gathers
// (pauli_momentum.hip, pauli_momentum_full.hip), the X = 0 group included.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 3.8 holds the table; no kernel uses scratch.
#include <cstring>

#include "dev_helpers.hpp"
#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_block_transfer_plan.hpp"
#include "pauli_measure.hpp"
#include "pauli_momentum_full_partner.hpp"
#include "pauli_momentum_partner.hpp"
#include "pauli_shared.hpp"

namespace ll {

namespace {
// Momentum blocks of ONE S_z sector: both share the sector's rank tables; src supplies the orbit table, its orbit lengths, the
// short-orbit test and the phases, the target the lane's states and lengths.
struct TransferMomentumPartner {
  const uint32_t* __restrict__ states;  // the target's reps
  const uint8_t* __restrict__ orbit_len;  // the target's
  PauliMomentumPartner src;
  __device__ __forceinline__ unsigned length(unsigned i) const { return (unsigned)orbit_len[i]; }
  __device__ __forceinline__ unsigned dead_length() const { return (unsigned)src.n_sites; }
  template <typename T, typename A, int E>
  __device__ __forceinline__ void add_group(unsigned X, const unsigned (&s)[E], const unsigned (&ra)[E], const bool (&live)[E],
                                            const A (&w)[E], const T* __restrict__ c, A (&acc)[E]) const {
    const unsigned px = __popc(X), himask = (1u << src.h) - 1;
    const unsigned L = (unsigned)src.n_sites, smask = (L >= 32u ? 0u : (1u << L)) - 1u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e] && 2 * __popc(s[e] & X) == px) {  // the partner has n_down set bits too
        const unsigned p = s[e] ^ X;
        const unsigned o = src.orbit[src.lo_rank[p & himask] + src.hi_rank[p >> src.h]];
        if (o != kPauliOrbitExcluded) {  // the partner's orbit is in the source block
          const unsigned j = o >> kPauliOrbitShiftBits, l = o & ((1u << kPauliOrbitShiftBits) - 1);
          bool is_short = false;
          for (int q = 0; q < src.nshort; ++q) is_short = is_short || pauli_rotl(p, (unsigned)src.short_shift[q], L, smask) == p;
          const unsigned rb = is_short ? (unsigned)src.orbit_len[j] : L;
          A wg = w[e];
          if (rb != ra[e]) wg = momentum_scale(wg, src.ratio[ra[e] * 32u + rb]);
          if (src.momentum != 0) wg = momentum_phase(wg, src.phase[2 * l], src.phase[2 * l + 1]);
          pauli_fma(acc[e], wg, c[j]);
        }
      }
    }
  }
};
// Momentum blocks of the full space: src supplies locate, the in-block mask, the searched basis and the phases
struct TransferMomentumFullPartner {
  const uint32_t* __restrict__ states;  // the target's reps
  const uint8_t* __restrict__ orbit_len;  // the target's
  PauliMomentumFullPartner src;
  unsigned src_dim;
  __device__ __forceinline__ unsigned length(unsigned i) const { return (unsigned)orbit_len[i]; }
  __device__ __forceinline__ unsigned dead_length() const { return 1u; }
  template <typename T, typename A, int E>
  __device__ __forceinline__ void add_group(unsigned X, const unsigned (&s)[E], const unsigned (&ra)[E], const bool (&live)[E],
                                            const A (&w)[E], const T* __restrict__ c, A (&acc)[E]) const {
    const unsigned m = (unsigned)src.momentum;
    unsigned rep[E], first[E], rb[E];
    src.locate(s, X, rep, first, rb);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (live[e] && ((src.in_block >> rb[e]) & 1u) != 0u) {  // the partner's orbit is in the source block: its reps[] holds b
        const unsigned j = pauli_bucket_search(src.states, src.start, src.prefix_shift, src.search_trips, rep[e], src_dim);
        const unsigned l = first[e] == 0u ? 0u : rb[e] - first[e];
        A wg = w[e];
        if (rb[e] != ra[e]) wg = momentum_scale(wg, src.ratio[ra[e] * 32u + rb[e]]);
        if (m != 0u) wg = momentum_phase(wg, src.phase[2 * l], src.phase[2 * l + 1]);
        pauli_fma(acc[e], wg, c[j]);
      }
    }
  }
};
}  // namespace

// dim: the target's; c holds the source's values (every index read comes from the source's tables: below the source's dim)
template <typename T, typename Partner>
__global__ __launch_bounds__(kBlock) void pauli_block_transfer_kernel(int b, unsigned nblocks, unsigned dim, int ngroups,
                                                                      const uint32_t* __restrict__ gx, const int32_t* __restrict__ gptr,
                                                                      const uint32_t* __restrict__ tz, const double* __restrict__ tc,
                                                                      Partner pt, const T* __restrict__ c, T* __restrict__ out,
                                                                      double* __restrict__ norm_partials) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  __shared__ double red[5];
  double norm_acc = 0.0;
  const unsigned bn = 1u << b;
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(dim / 2^b): base < dim < 2^27 (pauli_basis_kernel)
    const unsigned end = min(bn, dim - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned s[E], ra[E];
      bool live[E];
      A acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;
        live[e] = lo < end;
        s[e] = live[e] ? pt.states[base + lo] : 0u;
        ra[e] = live[e] ? pt.length(base + lo) : pt.dead_length();
        acc[e] = zero<A>();
      }
      for (int g = 0; g < ngroups; ++g) {
        const unsigned X = gx[g];
        A w[E];
#pragma unroll
        for (int e = 0; e < E; ++e) w[e] = zero<A>();
        for (int k = gptr[g], k1 = gptr[g + 1]; k < k1; ++k) {
          const unsigned z = tz[k];
          const A wk = PauliWeight<A>::load(tc, k, 0u);
#pragma unroll
          for (int e = 0; e < E; ++e) PauliWeight<A>::add(w[e], wk, __popc((s[e] ^ X) & z) & 1u);
        }
        pt.add_group(X, s, ra, live, w, c, acc);
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (live[e]) {
          const T v = narrow<T>(acc[e]);
          norm_acc += re_cmul(v, v);
          out[base + c0 + e * kBlock + threadIdx.x] = v;
        }
      }
    }
  }
  const double tot = block_sum(norm_acc, red);
  if (threadIdx.x == 0) norm_partials[blockIdx.x] = tot;
}

namespace {
struct TransferTables {
  int ngroups;
  const uint32_t* gx;
  const int32_t* gptr;
  const uint32_t* tz;
  const double* tc;
};
// returns the grid = the partials written
template <typename T, typename Partner>
int launch_transfer(int b, int64_t dim, const TransferTables& tb, const Partner& pt, const T* c, T* out, double* partials,
                    hipStream_t s) {
  const unsigned nblocks = (unsigned)((dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  hipLaunchKernelGGL((pauli_block_transfer_kernel<T, Partner>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, (unsigned)dim, tb.ngroups,
                     tb.gx, tb.gptr, tb.tz, tb.tc, pt, c, out, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T>
int launch_transfer_kind(const ll_operator& source, const ll_operator& target, const TransferTables& tb, const T* c, T* out,
                         double* partials, hipStream_t s) {
  if (target.kind == ll_operator::PAULI_MOMENTUM) {
    const PauliMomentumImage& ti = target.pauli_momentum;
    return launch_transfer(pauli_block_bits(target, &Tuning::pauli_momentum_block_bits, kPauliMomentumBlockBits), ti.dim, tb,
                           TransferMomentumPartner{ti.reps.get(), ti.orbit_len.get(), pauli_momentum_partner(source.pauli_momentum)}, c,
                           out, partials, s);
  }
  const PauliBlockImage& ti = target.pauli_block;  // PAULI_MOMENTUM_FULL: the caller admits the two kinds only
  return launch_transfer(pauli_block_bits(target, &Tuning::pauli_momentum_full_block_bits, kPauliMomentumFullBlockBits), ti.dim, tb,
                         TransferMomentumFullPartner{ti.basis.reps.get(), ti.basis.orbit_len.get(),
                                                     pauli_momentum_full_partner(source.pauli_block), (unsigned)source.pauli_block.dim},
                         c, out, partials, s);
}

PauliTransferSide transfer_side(const ll_operator& op) {
  PauliTransferSide sd;
  sd.elem_bytes = op.elem_bytes;
  sd.is_complex = op.is_complex;
  if (op.kind == ll_operator::PAULI_MOMENTUM || op.kind == ll_operator::PAULI_MOMENTUM_FULL || op.kind == ll_operator::PAULI_SYMMETRIC) {
    const PauliBlockView bv = pauli_block_view(op);
    sd.kind = op.kind == ll_operator::PAULI_MOMENTUM        ? kPauliTransferMomentum
              : op.kind == ll_operator::PAULI_MOMENTUM_FULL ? kPauliTransferMomentumFull
                                                            : kPauliTransferSymmetric;
    sd.n_sites = bv.n_sites;
    sd.n_down = bv.n_down;
    sd.momentum = bv.momentum;
  }
  return sd;
}

template <typename T>
void pauli_block_transfer_run(ll_context* ctx, const ll_operator* source, const ll_operator* target, const PauliBlockTransferPlan& plan,
                              const void* c, void* out, double* norm2_out) {
  const int64_t n_out = target->n_local;
  if (plan.nstrings() == 0) {  // exactly +0.0, no launch
    if (is_device_ptr(out)) {
      LL_HIP(hipSetDevice(ctx->device));
      LL_HIP(hipMemsetAsync(out, 0, (size_t)n_out * sizeof(T), ctx->stream));
      LL_HIP(hipStreamSynchronize(ctx->stream));
    } else {
      std::memset(out, 0, (size_t)n_out * sizeof(T));
    }
    if (norm2_out) *norm2_out = 0.0;
    return;
  }
  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<T> staged_in, staged_out;
  const T* const x = stage_in(ctx, staged_in, c, source->n_local);
  T* const y = stage_out(ctx, staged_out, out, n_out);
  DevBuf<int32_t> dgptr;
  DevBuf<uint32_t> dgx, dtz;
  DevBuf<double> dtc, sum;
  stage_table(ctx, dgptr, plan.gptr);
  stage_table(ctx, dgx, plan.gx);
  stage_table(ctx, dtz, plan.tz);
  stage_table(ctx, dtc, plan.tc);
  sum.alloc(ctx, 1);
  ctx->ensure_partials((size_t)kMaxGrid);
  double* const partials = ctx->partials.get();
  const TransferTables tb{(int)plan.ngroups(), dgx.p, dgptr.p, dtz.p, dtc.p};
  const int grid = launch_transfer_kind<T>(*source, *target, tb, x, y, partials, s);
  launch_reduce_cols(partials, grid, 1, sum.p, nullptr, s);
  stage_out_finish(ctx, staged_out, out, n_out);
  double norm2 = 0.0;
  LL_HIP(hipMemcpyAsync(&norm2, sum.p, sizeof(double), hipMemcpyDeviceToHost, s));
  LL_HIP(hipStreamSynchronize(s));  // the tables, the staged buffers and a pageable host buffer are no longer in use
  if (norm2_out) *norm2_out = norm2;
}
}  // namespace

// what capi.cpp calls: every check (nothing touches the device before they pass), the plan, then the operators' storage type
void pauli_block_transfer(ll_context* ctx, const ll_operator* source, const ll_operator* target, int64_t n_terms,
                          const ll_pauli_term* terms, const void* c, void* out, double* norm2_out) {
  LL_REQUIRE(ctx != nullptr && source != nullptr && target != nullptr && c != nullptr && out != nullptr,
             "ll_pauli_block_transfer: null argument");
  LL_REQUIRE(n_terms >= 0, "n_terms is negative");
  LL_REQUIRE(terms != nullptr || n_terms == 0, "ll_pauli_block_transfer: null argument (terms)");
  pauli_measure_prologue(ctx, "block transfers", {{source, "the source operator"}, {target, "the target operator"}});
  const PauliTransferSide ss = transfer_side(*source), ts = transfer_side(*target);
  if (const char* fault = pauli_block_transfer_fault(ss, ts))
    LL_REQUIRE(false, std::string(fault) + " (source: " + operator_kind_name(source->kind) + ", n_sites " + std::to_string(ss.n_sites) +
                          ", n_down " + std::to_string(ss.n_down) + "; target: " + operator_kind_name(target->kind) + ", n_sites " +
                          std::to_string(ts.n_sites) + ", n_down " + std::to_string(ts.n_down) + ")");
  for (int64_t j = 0; j < n_terms; ++j) {
    check_pauli_string("term", j, terms[j], ss.n_sites);
    LL_REQUIRE(source->is_complex || (__builtin_popcountll(terms[j].x_mask & terms[j].z_mask) & 1) == 0,
               "term " + std::to_string(j) + ": an odd number of Y factors makes the matrix complex; use a complex storage type");
  }
  const size_t eb = (size_t)source->elem_bytes;
  const uintptr_t a0 = (uintptr_t)c, a1 = a0 + (size_t)source->n_local * eb;
  const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)target->n_local * eb;
  LL_REQUIRE(a1 <= b0 || b1 <= a0, "input and output overlap");
  // a real storage type: both blocks have 2 m = 0 (mod n_sites) (creation), so 2 q = 0 and every weight of the plan is +-real
  const PauliBlockTransferPlan plan = pauli_block_transfer_plan(ss.n_sites, pauli_block_transfer_q(ss, ts), source->is_complex,
                                                                ss.kind == kPauliTransferMomentum, n_terms, terms);
  for_storage_type(*source, [&](auto t) { pauli_block_transfer_run<decltype(t)>(ctx, source, target, plan, c, out, norm2_out); });
}

}  // namespace ll
