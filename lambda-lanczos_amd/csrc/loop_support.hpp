// Run-scoped resources of the whole-loop drivers: buffers from the context's slab cache, the ring of read-back slots, phase timing.
#pragma once

#include "ll_internal.hpp"

#include <algorithm>
#include <utility>

namespace ll {

// A run-scoped device buffer.  Like the Krylov slabs it comes from, and goes back to, the context's slab cache: a
// hipMalloc / hipFree pair per run() costs hundreds of microseconds (hipFree synchronises the device) — most of a run on
// the small problems the reference is used for.
template <typename T> struct DevBuf {
  T* p = nullptr;
  ll_context* owner = nullptr;
  size_t bytes = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p && owner) owner->cache_put((void*)p, bytes);
    p = nullptr;
  }
  void alloc(ll_context* ctx, size_t count) {
    release();
    owner = ctx;
    bytes = std::max<size_t>(count * sizeof(T), 16);
    for (size_t i = 0; i < ctx->slab_cache.size(); ++i)
      if (ctx->slab_cache[i].second == bytes) {
        p = (T*)ctx->slab_cache[i].first;
        ctx->slab_cache.erase(ctx->slab_cache.begin() + (long)i);
        break;
      }
    if (!p) ctx->dev_malloc((void**)&p, bytes, "work vectors");
    ctx->test_fill_if_set(p, bytes / sizeof(T));
  }
};

// The host's read-back area (ctx->pinned, pinned and device-mapped): iteration k publishes its four scalars (alpha, beta^2, c0, c1)
// into ring slot k % kRingSlots; the gate values of the pair and block forms follow the slots, one per slot.  Sixteen slots: a
// block of eight iterations is enqueued while the eight of the block before it are still being collected.
constexpr int kRingSlots = 16, kSlotScalars = 4, kGateAt = kRingSlots * kSlotScalars;
constexpr size_t kPinnedScalars = 96;  // (kGateAt + kRingSlots used)

struct EventRing {
  hipEvent_t ev[kRingSlots];
  EventRing() {
    for (auto& e : ev) LL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~EventRing() {
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
};

struct PhaseTimer {  // optional per-phase device timing (HIP events on the context's stream)
  // Marks come in triples — start, after the operator, end of the iteration (or pair) — and are recorded into a RING of events
  // that the context keeps between runs: a triple is read back (its events completed long ago: the host runs a group or two ahead
  // of the device) when its slot comes round again.  (One fresh event per mark — 900 for config 3's run to convergence, 10 000 for
  // config 2's — cost the first profiled run of a process up to 0.5 s of host time in hipEventCreate on some boxes.)
  static constexpr size_t kTriples = 128;
  bool on;
  hipStream_t s;
  std::vector<hipEvent_t>& evs;
  size_t n = 0;  // marks so far
  double acc_op = 0.0, acc_rest = 0.0;
  PhaseTimer(ll_context* ctx, hipStream_t st) : on(ctx->profiling), s(st), evs(ctx->timer_events) {}
  void read(size_t first) {
    float a = 0, b = 0;
    if (hipEventSynchronize(evs[first + 2]) != hipSuccess) return;
    if (hipEventElapsedTime(&a, evs[first], evs[first + 1]) == hipSuccess) acc_op += a * 1e-3;
    if (hipEventElapsedTime(&b, evs[first + 1], evs[first + 2]) == hipSuccess) acc_rest += b * 1e-3;
  }
  void mark() {
    if (!on) return;
    const size_t slot = n % (3 * kTriples);
    if (slot % 3 == 0 && n >= 3 * kTriples) read(slot);  // the triple that used these events
    if (slot >= evs.size()) {
      hipEvent_t e;
      LL_HIP(hipEventCreate(&e));
      evs.push_back(e);
    }
    LL_HIP(hipEventRecord(evs[slot], s));
    ++n;
  }
  void collect(double& t_op, double& t_rest) {
    if (!on) return;
    // complete triples still in the ring: the last min(n / 3, kTriples) ones, minus those already read when their slot was reused
    const size_t triples = n / 3, done = n >= 3 * kTriples ? (n - 3 * kTriples) / 3 + ((n % 3) ? 1 : 0) : 0;
    for (size_t t = done; t < triples; ++t) read((t % kTriples) * 3);
    t_op += acc_op;
    t_rest += acc_rest;
    acc_op = acc_rest = 0.0;
    n = 0;
  }
};

// ll_context::stop_next for one operator application: set on entry, cleared on every exit — a throwing apply included, so that no later
// launch on the context is handed an event of a ring that has gone away (~EventRing)
struct StopNext {
  ll_context* ctx;
  StopNext(ll_context* c, hipEvent_t ev) : ctx(c) { ctx->stop_next = ev; }
  ~StopNext() { ctx->stop_next = nullptr; }
  bool taken() const { return ctx->stop_next == nullptr; }  // the launcher hung the event on its kernel
};

// The next `count` doubles of a buffer that is carved into regions (LoopState::PairBuf, LoopState::LagBuf)
inline double* carve(double*& at, size_t count) { return std::exchange(at, at + count); }
}  // namespace ll
