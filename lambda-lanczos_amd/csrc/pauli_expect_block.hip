// Expectation values of Pauli strings on a state of a ring's (or a torus's) symmetry block, for gfx950 (ll_pauli_expect_block, lanczos_hip.h):
// the state is given by its coefficients c on the block's representatives, Psi = B c with B the block's isometry, and
//   out = coef * Re <Psi| P |Psi> = coef * sum_a Re[ conj(c_a) (Pbar c)(a) ],      Pbar = (1 / |G|) sum_{h in G} h P h^-1
// (nothing is divided by <c|c>): Psi transforms by a one-dimensional character of the block's group G, so P may be replaced by
// its group average, which commutes with G and is therefore an operator the block kernels apply.  The plan
// (pauli_expect_block_plan.hpp) enumerates the images, merges them and writes, per observable that is not identically zero (a
// slot), term tables like a Hamiltonian's; batches of at most kPauliExpectBlockBatch slots, one launch = one batch = one sweep
// over c.  No n-sized workspace: (Pbar c)(a) lives in registers.
//
// The kernel is pauli_basis_kernel's block loop (pauli_basis.hpp: 2^b indices per workgroup block, b from the tuning key of the
// operator's own apply) with the Partner policy of the operator's kind, unchanged: a lane loads kPauliLaneStates states, their
// orbit lengths and c once per chunk, then works through the slots of the batch in a wave-uniform run-time loop (not unrolled:
// add_group of the symmetric policy is a long body).  Per slot: tmp = 0; for every group of the slot the weights as
// pauli_basis_kernel forms them and pt.add_group(...); then sum_e Re(conj(c_e) tmp_e) in double, folded over the wave at once
// and added by lane 0 to the wave's own LDS cell of the slot (32 slots x 4 waves of doubles: a run-time slot index never meets
// a register array, so nothing goes to scratch).  At the end the four wave cells of a slot are added in a fixed tree: one
// partial per workgroup and slot, folded over the workgroups in a fixed order by reduce_cols_kernel.  The host multiplies by
// the caller's coefficient.  The order of every sum depends on the block size and the grid alone — not on the alignment of c,
// not on where it lives, not on the slot's number or its batch: the same bits run to run.
//
// Bytes per sweep: (sizeof(T) + 5) D (c, reps, orbit lengths) when every gather is found in cache, plus per slot and group with
// X != 0 what the policy's own apply gathers (pauli_momentum.hip, pauli_momentum_full.hip, pauli_symmetric.hip, pauli_torus.hip).  The searched
// policies are bound by the rotation search's integer work and the bucket search's dependent loads, once per slot, group and
// state — slots with equal x masks repeat it (open).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 3.5 holds the table; no kernel uses scratch.
#include <cmath>

#include "dev_helpers.hpp"
#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_expect_block_plan.hpp"
#include "pauli_measure.hpp"
#include "pauli_momentum_full_partner.hpp"
#include "pauli_momentum_partner.hpp"
#include "pauli_shared.hpp"
#include "pauli_symmetric_partner.hpp"
#include "pauli_torus_partner.hpp"

namespace ll {

namespace {
constexpr int kPauliExpectBlockBatch = 32;  // slots per sweep: the LDS cells of a workgroup are 32 x 4 doubles
constexpr int kWaves = kBlock / 64;
static_assert(kWaves == 4 && kPauliExpectBlockBatch * kWaves <= kBlock, "one thread zeroes one cell; the final tree adds four");

// Re[conj(c) v], c widened to the accumulator's type
__device__ __forceinline__ double expect_block_term(double c, double v) { return c * v; }
__device__ __forceinline__ double expect_block_term(float c, double v) { return (double)c * v; }
__device__ __forceinline__ double expect_block_term(zc c, zc v) { return re_cmul(c, v); }
__device__ __forceinline__ double expect_block_term(cf c, zc v) { return re_cmul(to_acc(c), v); }
}  // namespace

// sg[k] .. sg[k + 1]: the groups of slot k of the batch in gx / gptr; gptr, tz, tc as PauliTermImage, over all slots of the call
template <typename T, typename Partner>
__global__ __launch_bounds__(kBlock) void pauli_expect_block_kernel(int b, unsigned nblocks, unsigned dim, int count,
                                                                    const int32_t* __restrict__ sg, const uint32_t* __restrict__ gx,
                                                                    const int32_t* __restrict__ gptr, const uint32_t* __restrict__ tz,
                                                                    const double* __restrict__ tc, Partner pt,
                                                                    const T* __restrict__ x, double* __restrict__ partials) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  __shared__ double cell[kPauliExpectBlockBatch * kWaves];  // [slot][wave]: written by lane 0 of that wave alone
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kPauliExpectBlockBatch * kWaves) cell[threadIdx.x] = 0.0;
  __syncthreads();
  const unsigned bn = 1u << b;
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(dim / 2^b): base < dim < 2^27 (pauli_basis_kernel)
    const unsigned end = min(bn, dim - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned s[E], ra[E];
      bool live[E];
      T xi[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;
        live[e] = lo < end;
        s[e] = live[e] ? pt.states[base + lo] : 0u;
        ra[e] = live[e] ? pt.length(base + lo) : pt.dead_length();
        xi[e] = live[e] ? x[base + lo] : zero<T>();
      }
      for (int k = 0; k < count; ++k) {  // wave-uniform, as everything read from the tables
        A tmp[E];
#pragma unroll
        for (int e = 0; e < E; ++e) tmp[e] = zero<A>();
        for (int g = sg[k], g1 = sg[k + 1]; g < g1; ++g) {
          const unsigned X = gx[g];
          A w[E];
#pragma unroll
          for (int e = 0; e < E; ++e) w[e] = zero<A>();
          for (int t = gptr[g], t1 = gptr[g + 1]; t < t1; ++t) {
            const unsigned z = tz[t];
            const A c = PauliWeight<A>::load(tc, t, 0u);
#pragma unroll
            for (int e = 0; e < E; ++e) PauliWeight<A>::add(w[e], c, __popc((s[e] ^ X) & z) & 1u);
          }
          pt.add_group(X, s, ra, live, w, xi, x, dim, tmp);
        }
        double part = 0.0;  // a dead state carries c = 0 and tmp = 0
#pragma unroll
        for (int e = 0; e < E; ++e) part += expect_block_term(xi[e], tmp[e]);
        part = wave_sum(part);
        if (lane == 0) cell[k * kWaves + wave] += part;
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < count) {
    const double* const c = cell + threadIdx.x * kWaves;
    partials[(size_t)blockIdx.x * count + threadIdx.x] = (c[0] + c[1]) + (c[2] + c[3]);
  }
}

namespace {
struct ExpectBlockTables {
  const int32_t* sg;
  const uint32_t* gx;
  const int32_t* gptr;
  const uint32_t* tz;
  const double* tc;
};
// one batch: returns the grid = the rows of partials written
template <typename T, typename Partner>
int launch_pauli_expect_block(int b, int64_t dim, int count, const ExpectBlockTables& tb, const Partner& pt, const T* x,
                              double* partials, hipStream_t s) {
  const unsigned nblocks = (unsigned)((dim + ((int64_t)1 << b) - 1) >> b);
  const int grid = (int)std::min<unsigned>(nblocks, (unsigned)kMaxGrid);
  hipLaunchKernelGGL((pauli_expect_block_kernel<T, Partner>), dim3(grid), dim3(kBlock), 0, s, b, nblocks, (unsigned)dim, count, tb.sg,
                     tb.gx, tb.gptr, tb.tz, tb.tc, pt, x, partials);
  LL_HIP(hipGetLastError());
  return grid;
}
template <typename T>
int launch_pauli_expect_block_op(const ll_operator& op, int count, const ExpectBlockTables& tb, const T* x, double* partials,
                                 hipStream_t s) {
  switch (op.kind) {
    case ll_operator::PAULI_MOMENTUM:
      return launch_pauli_expect_block(pauli_block_bits(op, &Tuning::pauli_momentum_block_bits, kPauliMomentumBlockBits),
                                       op.pauli_momentum.dim, count, tb, pauli_momentum_partner(op.pauli_momentum), x, partials, s);
    case ll_operator::PAULI_MOMENTUM_FULL:
      return launch_pauli_expect_block(pauli_block_bits(op, &Tuning::pauli_momentum_full_block_bits, kPauliMomentumFullBlockBits),
                                       op.pauli_block.dim, count, tb, pauli_momentum_full_partner(op.pauli_block), x, partials, s);
    case ll_operator::PAULI_TORUS:
      return launch_pauli_expect_block(pauli_block_bits(op, &Tuning::pauli_torus_block_bits, kPauliTorusBlockBits),
                                       op.pauli_block.dim, count, tb, pauli_torus_partner(op.pauli_block), x, partials, s);
    default:  // PAULI_SYMMETRIC: pauli_expect_block admits the four kinds only
      return launch_pauli_expect_block(pauli_block_bits(op, &Tuning::pauli_symmetric_block_bits, kPauliSymmetricBlockBits),
                                       op.pauli_block.dim, count, tb, pauli_symmetric_partner(op.pauli_block), x, partials, s);
  }
}
}  // namespace

template <typename T>
void pauli_expect_block_run(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs, const void* psi,
                            double* out, int64_t* sweeps_out) {
  constexpr int B = kPauliExpectBlockBatch;
  const PauliBlockView bv = pauli_block_view(*op);
  PauliBlockGroup grp;
  grp.n_sites = bv.n_sites;
  grp.reflection = bv.parity != 0;
  grp.flip = bv.inversion != 0;
  if (op->kind == ll_operator::PAULI_TORUS) {
    grp.lx = op->pauli_block.lx;
    grp.ly = op->pauli_block.ly;
  }
  check_observables(bv.n_sites, n_obs, obs);
  const PauliExpectBlockPlan plan = pauli_expect_block_plan(grp, scalar_traits<T>::is_complex, bv.n_down >= 0, n_obs, obs, B);
  for (int64_t j = 0; j < n_obs; ++j) out[j] = 0.0;  // what the identically zero observables keep: +0.0
  const int64_t nslots = plan.nslots();
  if (sweeps_out) *sweeps_out = plan.nbatches();
  if (nslots == 0) return;  // nothing has touched the device

  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf<T> staged;
  const T* const x = stage_in(ctx, staged, psi, op->n_local);
  // the slots' tables, one after the other: sg[slot] = its first group, gptr[] counts the strings from the call's first
  std::vector<int32_t> sg, gptr;
  std::vector<uint32_t> gx, tz;
  std::vector<double> tc;
  for (const PauliExpectBlockSlot& sl : plan.slots) {
    sg.push_back((int32_t)gx.size());
    const int32_t t0 = (int32_t)tz.size();
    for (int64_t g = 0; g < sl.ngroups(); ++g) gptr.push_back(t0 + sl.gptr[(size_t)g]);
    gx.insert(gx.end(), sl.gx.begin(), sl.gx.end());
    tz.insert(tz.end(), sl.tz.begin(), sl.tz.end());
    tc.insert(tc.end(), sl.tc.begin(), sl.tc.end());
  }
  sg.push_back((int32_t)gx.size());
  gptr.push_back((int32_t)tz.size());
  DevBuf<int32_t> dsg, dgptr;
  DevBuf<uint32_t> dgx, dtz;
  DevBuf<double> dtc;
  stage_table(ctx, dsg, sg);
  stage_table(ctx, dgptr, gptr);
  stage_table(ctx, dgx, gx);
  stage_table(ctx, dtz, tz);
  stage_table(ctx, dtc, tc);
  const std::vector<double> sums = pauli_measure_sweeps(ctx, plan, (size_t)kMaxGrid * B, [&](int64_t k, double* partials) {
    const ExpectBlockTables tb{dsg.p + plan.batch_begin(k), dgx.p, dgptr.p, dtz.p, dtc.p};
    return launch_pauli_expect_block_op<T>(*op, (int)plan.batch_count(k), tb, x, partials, s);
  });
  for (int64_t i = 0; i < nslots; ++i) out[plan.slots[(size_t)i].obs] = plan.slots[(size_t)i].coef * sums[(size_t)i];
}

// what capi.cpp calls: the checks that do not depend on the storage type, then the operator's type
void pauli_expect_block(ll_context* ctx, const ll_operator* op, int64_t n_obs, const ll_pauli_term* obs, const void* psi, double* out,
                        int64_t* sweeps_out) {
  LL_REQUIRE(ctx != nullptr && op != nullptr, "null argument");
  LL_REQUIRE(n_obs >= 0, "n_obs is negative");
  LL_REQUIRE(n_obs == 0 || (obs != nullptr && psi != nullptr && out != nullptr), "null argument");
  pauli_measure_prologue(ctx, "expectation values", {{op, "the operator"}});
  if (op->kind == ll_operator::PAULI || op->kind == ll_operator::PAULI_SECTOR)
    LL_REQUIRE(false, std::string("the operator is ") + operator_kind_name(op->kind) +
                          ": its basis is not a symmetry block; measure with ll_pauli_expect");
  LL_REQUIRE(op->kind == ll_operator::PAULI_MOMENTUM || op->kind == ll_operator::PAULI_MOMENTUM_FULL ||
                 op->kind == ll_operator::PAULI_SYMMETRIC || op->kind == ll_operator::PAULI_TORUS,
             std::string("the operator is ") + operator_kind_name(op->kind) +
                 ": expectation values on a symmetry block need a momentum, full-momentum or momentum / reflection / "
                 "spin-inversion block of a sum of Pauli strings");  // (the text callers match on; a torus block is admitted too)
  if (sweeps_out) *sweeps_out = 0;
  if (n_obs == 0) return;
  for_storage_type(*op, [&](auto t) { pauli_expect_block_run<decltype(t)>(ctx, op, n_obs, obs, psi, out, sweeps_out); });
}

}  // namespace ll
