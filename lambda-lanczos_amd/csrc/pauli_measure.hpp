// The host side that the measuring entry points on the Pauli-sum operators share (pauli_expect.hip, pauli_expect_block.hip,
// pauli_rdm.hip, pauli_block_embed.hip, pauli_block_transfer.hip): the checks they begin with, a host vector staged on the device, the sweeps over the
// batches of a plan with their fold, and one view of the three kinds of symmetry block.  The kernels, their launch wrappers and
// the per-kind switches stay in the .hip files; the storage-type dispatch is for_storage_type (ll_internal.hpp).
#pragma once

#include <initializer_list>

#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_expect_plan.hpp"

namespace ll {

// After an entry point's own null checks: every operator belongs to the context, and the context is not sharded.
// name: "the operator", "the block operator"; feature: "expectation values", the subject of "... are not built for sharded contexts".
struct NamedOperator {
  const ll_operator* op;
  const char* name;
};
inline void pauli_measure_prologue(const ll_context* ctx, const char* feature, std::initializer_list<NamedOperator> ops) {
  for (const NamedOperator& o : ops) LL_REQUIRE(o.op->ctx == ctx, std::string(o.name) + " belongs to another context");
  LL_REQUIRE(ctx->comm == nullptr, std::string(feature) + " are not built for sharded contexts (a context with a communicator)");
}
inline void check_observables(int n_sites, int64_t n_obs, const ll_pauli_term* obs) {
  for (int64_t j = 0; j < n_obs; ++j) check_pauli_string("observable", j, obs[j], n_sites);
}

// The device pointer of an input of n values that may be host memory: a host vector is copied into `staged`, which the caller
// keeps until it has synchronised the stream (a pageable source is read until then).
template <typename T> const T* stage_in(ll_context* ctx, DevBuf<T>& staged, const void* src, int64_t n) {
  if (is_device_ptr(src)) return (const T*)src;
  staged.alloc(ctx, (size_t)n);
  LL_HIP(hipMemcpyAsync(staged.p, src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return staged.p;
}
// The same for an output: the device buffer to write now; stage_out_finish enqueues the copy to a host `dst` behind the kernels.
template <typename T> T* stage_out(ll_context* ctx, DevBuf<T>& staged, void* dst, int64_t n) {
  if (is_device_ptr(dst)) return (T*)dst;
  staged.alloc(ctx, (size_t)n);
  return staged.p;
}
template <typename T> void stage_out_finish(ll_context* ctx, const DevBuf<T>& staged, void* dst, int64_t n) {
  if (staged.p) LL_HIP(hipMemcpyAsync(dst, staged.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
}

// A host table of a call on the device, enqueued on the stream (the caller keeps `src` until it has synchronised)
template <typename V> void stage_table(ll_context* ctx, DevBuf<V>& dst, const std::vector<V>& src) {
  dst.alloc(ctx, std::max<size_t>(src.size(), 1));
  if (!src.empty()) LL_HIP(hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(V), hipMemcpyHostToDevice, ctx->stream));
}

// One sweep per batch: launch(k, partials) enqueues batch k — bt.batch_count(k) columns of partials, one row per workgroup — and
// returns its grid; reduce_cols_kernel folds the rows in a fixed order into the batch's slots.  Returns the bt.nslots() folded
// sums, after the call's one copy back and one synchronisation: the tables and a pageable psi are no longer read.
// partials_doubles: the most a launch writes.
template <typename Launch>
std::vector<double> pauli_measure_sweeps(ll_context* ctx, const PauliBatches& bt, size_t partials_doubles, Launch&& launch) {
  hipStream_t s = ctx->stream;
  DevBuf<double> sums;
  sums.alloc(ctx, (size_t)bt.nslots());
  ctx->ensure_partials(partials_doubles);
  double* const partials = ctx->partials.get();
  for (int64_t k = 0; k < bt.nbatches(); ++k) {
    const int grid = launch(k, partials);
    launch_reduce_cols(partials, grid, (int)bt.batch_count(k), sums.p + bt.batch_begin(k), nullptr, s);
  }
  std::vector<double> host((size_t)bt.nslots());
  LL_HIP(hipMemcpyAsync(host.data(), sums.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  LL_HIP(hipStreamSynchronize(s));
  return host;
}

// What the measuring code reads of a symmetry block, whichever of the two images holds it (PAULI_MOMENTUM: PauliMomentumImage,
// no reflection, no inversion; PAULI_MOMENTUM_FULL and PAULI_SYMMETRIC: PauliBlockImage, n_down = -1 on the full space)
struct PauliBlockView {
  int n_sites, n_down, momentum, parity, inversion;
  const double* phase;
  const uint32_t* reps;
  const uint8_t* orbit_len;
  int64_t dim;
};
inline PauliBlockView pauli_block_view(const ll_operator& op) {
  if (op.kind == ll_operator::PAULI_MOMENTUM) {
    const PauliMomentumImage& im = op.pauli_momentum;
    return {im.n_sites, im.n_down, im.momentum, 0, 0, im.phase.get(), im.reps.get(), im.orbit_len.get(), im.dim};
  }
  const PauliBlockImage& im = op.pauli_block;
  return {im.n_sites,     im.n_down, im.momentum, im.parity, im.inversion, im.phase.get(), im.basis.reps.get(), im.basis.orbit_len.get(),
          im.dim};
}

}  // namespace ll
