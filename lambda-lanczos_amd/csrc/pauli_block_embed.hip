// A state between a ring's symmetry block and the full space or an S_z sector, for gfx950 (ll_pauli_block_expand,
// ll_pauli_block_project, lanczos_hip.h): with B the block's isometry (pauli_block_embed_plan.hpp),
//   expand    psi[t] = val(t) c[col(t)],    val(t) = chi(g) / sqrt(R_b) for t = g b, +0.0 where the block excludes the orbit of t
//   project   c[a] = sum_{t in the orbit of a} conj(val(t)) psi[t] = (sqrt(R_a) / |G|) sum_{g in G} conj(chi(g)) psi[g a]
// over the basis of a target operator: all 2^n_sites states, or the states of one S_z sector in ascending order.
//
// Expand is a gather over the OUTPUT index, so every store is coalesced: a workgroup takes blocks of 2^b output indices in a
// grid-stride loop (b: the key pauli_block_expand_block_bits), a lane carries kPauliLaneStates of them — the state t is the index
// itself or target.states[index] — and a Locator of the block's kind answers (column, R, l, sign flip, in the block):
//   momentum block of a sector   orbit[rank(t)], the table of the operator's own apply (a sector target: rank(t) is the index)
//   momentum block, full space   PauliMomentumFullPartner::locate, then pauli_bucket_search; in the block iff m R = 0 (mod L)
//   symmetric block              PauliSymmetricPartner::locate, then pauli_bucket_search; in the block iff the entry found is b
// — the locate() of the applying kernels: one definition of who reached the minimum first and how many did.  A state outside a
// sector block's sector is not found (its representative has another popcount), or is masked by its popcount (momentum block).
// The value: wide(c[col]) * factor[R] (one rounding per component), times the phase where m != 0 (exact on the axes), a sign
// flip, one rounding to T.  Output indices reach 2^30 (unsigned arithmetic below 2^31 + 2^11, byte offsets through size_t).
//
// Project takes one representative per lane over blocks of 2^b representatives (b: the key pauli_block_project_block_bits), as
// the block kernels do, and walks the |G| elements in the one order (rho, zeta, j) -> T^j P^rho Z^zeta — wave-uniform bounds, the
// phase a scalar load —, gathers psi at the image (through the target's rank tables in a sector) and accumulates
// conj(chi(g)) psi in double; at the end factor[R_a] = sqrt(R_a) / |G|, one rounding to T.  No atomics, no search: the order of
// the sum is fixed by the enumeration alone.  Both kernels: the same bits run to run, for every block size, grid and alignment.
//
// Bytes: expand writes sizeof(T) N and reads c through a cached gather (the searched kinds also read about search_trips
// representatives per state, the momentum kind 4 N bytes of orbit table, a sector target 4 N bytes of states); project reads
// sizeof(T) N gathered (every state of an admitted orbit |G| / R times, the repeats from cache) and writes sizeof(T) D.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 3.7 holds the table; no kernel uses scratch.
#include "dev_helpers.hpp"
#include "engine.hpp"
#include "ll_internal.hpp"
#include "loop_support.hpp"
#include "pauli_block_embed_plan.hpp"
#include "pauli_measure.hpp"
#include "pauli_momentum_full_partner.hpp"
#include "pauli_shared.hpp"
#include "pauli_symmetric_partner.hpp"

namespace ll {

namespace {
// (column, R, l, flip, in the block) of E states; SectorTarget: idx[] is rank(t) in the sector
struct EmbedMomentumLocator {
  const uint32_t* __restrict__ orbit;
  const uint8_t* __restrict__ orbit_len;
  const uint32_t* __restrict__ lo_rank;
  const uint32_t* __restrict__ hi_rank;
  int h, n_down;
  template <bool SectorTarget, int E>
  __device__ __forceinline__ void find(const unsigned (&t)[E], const unsigned (&idx)[E], const bool (&live)[E], unsigned (&col)[E],
                                       unsigned (&R)[E], unsigned (&l)[E], unsigned (&flip)[E], bool (&in)[E]) const {
    const unsigned himask = (1u << h) - 1u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      in[e] = live[e] && (SectorTarget || (int)__popc(t[e]) == n_down);  // the rank tables hold the sector's states only
      col[e] = R[e] = l[e] = flip[e] = 0u;
      if (in[e]) {
        const unsigned o = orbit[SectorTarget ? idx[e] : lo_rank[t[e] & himask] + hi_rank[t[e] >> h]];
        in[e] = o != kPauliOrbitExcluded;
        if (in[e]) {
          col[e] = o >> kPauliOrbitShiftBits;
          l[e] = o & ((1u << kPauliOrbitShiftBits) - 1u);
          R[e] = (unsigned)orbit_len[col[e]];
        }
      }
    }
  }
};
struct EmbedMomentumFullLocator {
  PauliMomentumFullPartner pt;
  unsigned dim;
  template <bool SectorTarget, int E>
  __device__ __forceinline__ void find(const unsigned (&t)[E], const unsigned (&)[E], const bool (&live)[E], unsigned (&col)[E],
                                       unsigned (&R)[E], unsigned (&l)[E], unsigned (&flip)[E], bool (&in)[E]) const {
    unsigned rep[E], first[E];
    pt.locate(t, 0u, rep, first, R);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      in[e] = live[e] && ((pt.in_block >> R[e]) & 1u) != 0u;  // then reps[] holds the representative
      col[e] = flip[e] = 0u;
      l[e] = first[e] == 0u ? 0u : R[e] - first[e];  // t = T^(R - first) b
      if (in[e]) col[e] = pauli_bucket_search(pt.states, pt.start, pt.prefix_shift, pt.search_trips, rep[e], dim);
    }
  }
};
struct EmbedSymmetricLocator {
  PauliSymmetricPartner pt;
  unsigned dim;
  template <bool SectorTarget, int E>
  __device__ __forceinline__ void find(const unsigned (&t)[E], const unsigned (&)[E], const bool (&live)[E], unsigned (&col)[E],
                                       unsigned (&R)[E], unsigned (&l)[E], unsigned (&flip)[E], bool (&in)[E]) const {
    const unsigned L = (unsigned)pt.n_sites;
    unsigned rep[E], who[E], cnt[E];
    pt.locate(t, 0u, rep, who, cnt);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      in[e] = false;
      col[e] = R[e] = 0u;
      const unsigned first = who[e] & 31u;
      l[e] = first == 0u ? 0u : L - first;  // t = h^-1 b, h = T^first P^rho Z^zeta: the phase of T^(L - first)
      flip[e] = ((who[e] >> 5) & pt.neg_parity) ^ ((who[e] >> 6) & pt.neg_inversion);
      if (live[e]) {
        const unsigned j = pauli_bucket_search(pt.states, pt.start, pt.prefix_shift, pt.search_trips, rep[e], dim);
        in[e] = pt.states[j] == rep[e];  // b is in the basis (as the applying kernel decides it)
        col[e] = j;
        R[e] = (unsigned)pt.orbit_len[j];  // of b when it is in the basis; not used otherwise
      }
    }
  }
};

// conj(chi) v for chi = (c, sn) * (-1)^flip; m = 0: the phase is 1
__device__ __forceinline__ double project_term(double v, double c, double, unsigned m, unsigned flip) {
  return pauli_flip_sign(m != 0u ? v * c : v, flip);
}
__device__ __forceinline__ zc project_term(zc v, double c, double sn, unsigned m, unsigned flip) {
  return pauli_flip_sign(m != 0u ? zc{v.re * c + v.im * sn, v.im * c - v.re * sn} : v, flip);
}
__device__ __forceinline__ void project_add(double& acc, double v) { acc += v; }
__device__ __forceinline__ void project_add(zc& acc, zc v) {
  acc.re += v.re;
  acc.im += v.im;
}
}  // namespace

template <typename T, typename Locator, bool SectorTarget>
__global__ __launch_bounds__(kBlock) void pauli_block_expand_kernel(int b, unsigned nblocks, unsigned n,
                                                                    const uint32_t* __restrict__ tstates, Locator lc, unsigned m,
                                                                    const double* __restrict__ phase,
                                                                    const double* __restrict__ factor, const T* __restrict__ c,
                                                                    T* __restrict__ out) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  const unsigned bn = 1u << b;  // b <= 30
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(n / 2^b): base < n <= 2^30
    const unsigned end = min(bn, n - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned t[E], idx[E], col[E], R[E], l[E], flip[E];
      bool live[E], in[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;  // < 2^30 + 2^10
        live[e] = lo < end;
        idx[e] = live[e] ? base + lo : 0u;
        t[e] = SectorTarget ? (live[e] ? tstates[idx[e]] : 0u) : idx[e];
      }
      lc.template find<SectorTarget>(t, idx, live, col, R, l, flip, in);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (live[e]) {
          T v = zero<T>();  // +0.0: the block excludes the orbit of t, or t lies outside the block's sector
          if (in[e]) {
            A w = momentum_scale(to_acc(c[col[e]]), factor[R[e]]);
            if (m != 0u) w = momentum_phase(w, phase[2 * l[e]], phase[2 * l[e] + 1]);
            v = narrow<T>(pauli_flip_sign(w, flip[e]));
          }
          out[(size_t)idx[e]] = v;
        }
      }
    }
  }
}

// the group: T^j (always), P^rho iff use_p, Z^zeta iff use_z; neg_p / neg_z: the flag carries a factor -1
template <typename T, bool SectorTarget>
__global__ __launch_bounds__(kBlock) void pauli_block_project_kernel(int b, unsigned nblocks, unsigned dim,
                                                                     const uint32_t* __restrict__ reps,
                                                                     const uint8_t* __restrict__ orbit_len,
                                                                     const uint32_t* __restrict__ lo_rank,
                                                                     const uint32_t* __restrict__ hi_rank, int h, int n_sites,
                                                                     unsigned m, unsigned use_p, unsigned use_z, unsigned neg_p,
                                                                     unsigned neg_z, const double* __restrict__ phase,
                                                                     const double* __restrict__ factor, const T* __restrict__ psi,
                                                                     T* __restrict__ out) {
  typedef acc_t<T> A;
  constexpr int E = kPauliLaneStates;
  const unsigned L = (unsigned)n_sites, smask = (1u << L) - 1u, himask = (1u << h) - 1u;  // 1 <= L <= 30
  const unsigned bn = 1u << b;
  for (unsigned blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const unsigned base = blk << b;  // nblocks = ceil(dim / 2^b): base < dim < 2^27
    const unsigned end = min(bn, dim - base);
    for (unsigned c0 = 0; c0 < end; c0 += kBlock * E) {
      unsigned s[E], cur[E];
      bool live[E];
      A acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const unsigned lo = c0 + e * kBlock + threadIdx.x;
        live[e] = lo < end;
        s[e] = live[e] ? reps[base + lo] : 0u;
        acc[e] = zero<A>();
      }
      for (unsigned rho = 0; rho <= use_p; ++rho) {
        for (unsigned zeta = 0; zeta <= use_z; ++zeta) {
          const unsigned flip = (rho & neg_p) ^ (zeta & neg_z);
#pragma unroll
          for (int e = 0; e < E; ++e) cur[e] = (rho ? __brev(s[e]) >> (32u - L) : s[e]) ^ (zeta ? smask : 0u);
          for (unsigned j = 0; j < L; ++j) {  // cur = T^j P^rho Z^zeta s
            const double pc = phase[2 * j], ps = phase[2 * j + 1];
#pragma unroll
            for (int e = 0; e < E; ++e) {
              if (live[e]) {
                const unsigned i = SectorTarget ? lo_rank[cur[e] & himask] + hi_rank[cur[e] >> h] : cur[e];  // G keeps the sector
                project_add(acc[e], project_term(to_acc(psi[(size_t)i]), pc, ps, m, flip));
              }
              cur[e] = pauli_rotl(cur[e], 1u, L, smask);
            }
          }
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (live[e]) {
          const unsigned i = base + c0 + e * kBlock + threadIdx.x;
          out[i] = narrow<T>(momentum_scale(acc[e], factor[orbit_len[i]]));
        }
      }
    }
  }
}

namespace {
struct EmbedTables {
  unsigned m;
  const double* phase;
  const double* factor;
};
template <typename T, bool SectorTarget, typename Locator>
void launch_expand(const PauliEmbedLaunch& g, int64_t n, const uint32_t* tstates, const Locator& lc, const EmbedTables& tb, const T* c,
                   T* out, hipStream_t s) {
  hipLaunchKernelGGL((pauli_block_expand_kernel<T, Locator, SectorTarget>), dim3(g.grid), dim3(kBlock), 0, s, g.bits, (unsigned)g.units,
                     (unsigned)n, tstates, lc, tb.m, tb.phase, tb.factor, c, out);
  LL_HIP(hipGetLastError());
}
template <typename T, bool SectorTarget>
void launch_expand_kind(const ll_operator& block, const PauliEmbedLaunch& g, int64_t n, const uint32_t* tstates, const EmbedTables& tb,
                        const T* c, T* out, hipStream_t s) {
  switch (block.kind) {
    case ll_operator::PAULI_MOMENTUM: {
      const PauliMomentumImage& im = block.pauli_momentum;
      launch_expand<T, SectorTarget>(g, n, tstates,
                                     EmbedMomentumLocator{im.orbit.get(), im.orbit_len.get(), im.lo_rank.get(), im.hi_rank.get(), im.h,
                                                          im.n_down},
                                     tb, c, out, s);
      return;
    }
    case ll_operator::PAULI_MOMENTUM_FULL:
      launch_expand<T, SectorTarget>(g, n, tstates,
                                     EmbedMomentumFullLocator{pauli_momentum_full_partner(block.pauli_block), (unsigned)block.pauli_block.dim},
                                     tb, c, out, s);
      return;
    default:  // PAULI_SYMMETRIC: the caller admits the three kinds only
      launch_expand<T, SectorTarget>(g, n, tstates,
                                     EmbedSymmetricLocator{pauli_symmetric_partner(block.pauli_block), (unsigned)block.pauli_block.dim},
                                     tb, c, out, s);
  }
}

PauliEmbedSide embed_side(const ll_operator& op) {
  PauliEmbedSide sd;
  sd.elem_bytes = op.elem_bytes;
  sd.is_complex = op.is_complex;
  switch (op.kind) {
    case ll_operator::PAULI:
      sd.role = kPauliEmbedTargetFull;
      sd.n_sites = op.pauli.n_sites;
      break;
    case ll_operator::PAULI_SECTOR:
      sd.role = kPauliEmbedTargetSector;
      sd.n_sites = op.pauli_sector.n_sites;
      sd.n_down = op.pauli_sector.n_down;
      break;
    case ll_operator::PAULI_MOMENTUM:
    case ll_operator::PAULI_MOMENTUM_FULL:
    case ll_operator::PAULI_SYMMETRIC: {
      const PauliBlockView bv = pauli_block_view(op);
      sd.role = op.kind == ll_operator::PAULI_MOMENTUM    ? kPauliEmbedBlockMomentum
                : op.kind == ll_operator::PAULI_SYMMETRIC ? kPauliEmbedBlockSymmetric
                                                          : kPauliEmbedBlockMomentumFull;
      sd.n_sites = bv.n_sites;
      sd.n_down = bv.n_down;
      break;
    }
    default: break;
  }
  return sd;
}

template <typename T>
void pauli_block_embed_run(ll_context* ctx, const ll_operator* block, const ll_operator* target, bool expand, const void* in, void* out) {
  LL_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const PauliBlockView bv = pauli_block_view(*block);
  const bool sector_target = target->kind == ll_operator::PAULI_SECTOR;
  const int64_t dim = block->n_local, n = target->n_local;
  const int64_t n_in = expand ? dim : n, n_out = expand ? n : dim;
  const unsigned m = (unsigned)bv.momentum;

  DevBuf<T> staged_in, staged_out;
  const T* const x = stage_in(ctx, staged_in, in, n_in);
  T* const y = stage_out(ctx, staged_out, out, n_out);
  const std::vector<double> fac = expand ? pauli_block_expand_factors()
                                         : pauli_block_project_factors(pauli_block_group_size(bv.n_sites, bv.parity != 0, bv.inversion != 0));
  DevBuf<double> dfac;
  dfac.alloc(ctx, fac.size());
  LL_HIP(hipMemcpyAsync(dfac.p, fac.data(), fac.size() * sizeof(double), hipMemcpyHostToDevice, s));
  const EmbedTables tb{m, bv.phase, dfac.p};
  if (expand) {
    const PauliEmbedLaunch g = pauli_block_embed_launch(n, ctx->tune.pauli_block_expand_block_bits, kPauliBlockExpandBlockBits, kMaxGrid);
    if (sector_target) launch_expand_kind<T, true>(*block, g, n, target->pauli_sector.states.get(), tb, x, y, s);
    else launch_expand_kind<T, false>(*block, g, n, nullptr, tb, x, y, s);
  } else {
    const PauliEmbedLaunch g = pauli_block_embed_launch(dim, ctx->tune.pauli_block_project_block_bits, kPauliBlockProjectBlockBits, kMaxGrid);
    const PauliSectorImage& ts = target->pauli_sector;
    const unsigned use_p = bv.parity != 0 ? 1u : 0u, use_z = bv.inversion != 0 ? 1u : 0u;
    const unsigned neg_p = bv.parity < 0 ? 1u : 0u, neg_z = bv.inversion < 0 ? 1u : 0u;
    if (sector_target)
      hipLaunchKernelGGL((pauli_block_project_kernel<T, true>), dim3(g.grid), dim3(kBlock), 0, s, g.bits, (unsigned)g.units, (unsigned)dim,
                         bv.reps, bv.orbit_len, ts.lo_rank.get(), ts.hi_rank.get(), ts.h, bv.n_sites, m, use_p, use_z, neg_p, neg_z,
                         bv.phase, tb.factor, x, y);
    else
      hipLaunchKernelGGL((pauli_block_project_kernel<T, false>), dim3(g.grid), dim3(kBlock), 0, s, g.bits, (unsigned)g.units, (unsigned)dim,
                         bv.reps, bv.orbit_len, (const uint32_t*)nullptr, (const uint32_t*)nullptr, 0, bv.n_sites, m, use_p, use_z, neg_p,
                         neg_z, bv.phase, tb.factor, x, y);
    LL_HIP(hipGetLastError());
  }
  stage_out_finish(ctx, staged_out, out, n_out);
  LL_HIP(hipStreamSynchronize(s));  // the factor table, the staged buffers and a pageable host buffer are no longer in use
}
}  // namespace

// what capi.cpp calls: every check (nothing touches the device before they pass), then the operators' storage type
void pauli_block_embed(ll_context* ctx, const ll_operator* block, const ll_operator* target, bool expand, const void* in, void* out) {
  const char* const who = expand ? "ll_pauli_block_expand" : "ll_pauli_block_project";
  LL_REQUIRE(ctx != nullptr && block != nullptr && target != nullptr && in != nullptr && out != nullptr, std::string(who) + ": null argument");
  pauli_measure_prologue(ctx, "block embeddings", {{block, "the block operator"}, {target, "the target operator"}});
  const PauliEmbedSide bs = embed_side(*block), ts = embed_side(*target);
  LL_REQUIRE(pauli_embed_is_block(bs.role),
             std::string("the block operator is ") + operator_kind_name(block->kind) +
                 ": it must be a momentum, full-momentum or momentum / reflection / spin-inversion block of a sum of Pauli strings");
  LL_REQUIRE(pauli_embed_is_target(ts.role),
             std::string("the target operator is ") + operator_kind_name(target->kind) +
                 ": it must be a full-space or S_z-sector sum of Pauli strings, which names the basis of the expanded state");
  if (const char* fault = pauli_block_embed_fault(bs, ts))
    LL_REQUIRE(false, std::string(fault) + " (block: " + operator_kind_name(block->kind) + ", n_sites " + std::to_string(bs.n_sites) +
                          ", n_down " + std::to_string(bs.n_down) + "; target: " + operator_kind_name(target->kind) + ", n_sites " +
                          std::to_string(ts.n_sites) + ", n_down " + std::to_string(ts.n_down) + ")");
  const size_t eb = (size_t)block->elem_bytes;
  const uintptr_t a0 = (uintptr_t)in, a1 = a0 + (size_t)(expand ? block->n_local : target->n_local) * eb;
  const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)(expand ? target->n_local : block->n_local) * eb;
  LL_REQUIRE(a1 <= b0 || b1 <= a0, "input and output overlap");
  for_storage_type(*block, [&](auto t) { pauli_block_embed_run<decltype(t)>(ctx, block, target, expand, in, out); });
}

}  // namespace ll

