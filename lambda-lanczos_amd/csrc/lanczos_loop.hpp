// Host drivers: the device-resident Krylov loop of LambdaLanczos<T>::run (LL:216-366) and Exponentiator<T>::run
// (EX:87-173).  Everything n-sized stays in HBM; per iteration the host receives four doubles (alpha_k, beta_k^2
// and two diagnostics) through pinned, device-mapped memory and runs the k x k tridiagonal step (a11/a12) while
// the device already executes iteration k+1 (lag-1 speculation: a speculative iteration only writes basis slots
// the results never read, so stopping one iteration "late" on the device is harmless).
// This header is the loop machinery both drivers share (lanczos_run.cpp, expo_run.cpp; the basis-free drivers — recurrence.hpp,
// two_pass_run.cpp, expo_two_pass_multi_run.cpp — take the argument checks, the default start vector and the speculation policy at
// its end).  Run-scoped resources: loop_support.hpp; the host algebra of the raw-basis forms: raw_basis.hpp.
#pragma once

#include "engine.hpp"
#include "loop_support.hpp"
#include "raw_basis.hpp"
#include "ritz_tracker.hpp"
#include "trace.hpp"

#include <algorithm>
#include <cmath>
#include <limits>
#include <random>
#include <string>
#include <variant>

namespace ll {

// Environment switches used below come from ctx->tune (read once per context, ll_internal.hpp):
//   dgks_threshold  DGKS "twice is enough": a second Gram-Schmidt pass is due when the first one removed more than this
//                   fraction of ||w||^2 (LL_DGKS_THRESHOLD; a value > 1 forces the second pass in every iteration: tests).
//   tridiag_lag     sharded contexts consume the helper thread's verdicts a fixed number of iterations late
//                   (StepWorker::consume); each stop costs that many speculative iterations, a slow host step is hidden
//                   for that many (LL_TRIDIAG_LAG; negative: the single-process opportunistic policy — unsafe with more
//                   than one rank, kept to demonstrate the hang).

// One Lanczos iteration as the device sees it, shared by the eigen-solver and the Exponentiator loops:
//   y = A u_{k-1} + offset u_{k-1}, alpha (a1-a3)  ->  three-term update + Gram-Schmidt against `runs` + norm (a4-a7)
//   ->  normalisation + publish of the iteration's four scalars (a8).
// The last step is DEFERRED where the operator kernel can normalise its input on the fly (Engine::can_defer_scale): the
// iteration then ends with w_k unnormalised in a work buffer and the partial sums of ||w_k||^2; the NEXT iteration's
// operator kernel folds them, works with u_k = w_k / ||w_k||, writes u_k into the basis slot and publishes — one launch
// and one read of w per iteration less (three launches become two in the Exponentiator loop, five become four in the
// eigen-solver's).  flush() does the same work with the stand-alone kernel when no next iteration follows.
template <typename T> struct LoopState {
  Engine<T>& E;
  Basis<T>& U;
  EventRing& ring;
  PhaseTimer& timer;
  int64_t nl;
  hipStream_t s;
  bool fuse_launches = true, defer = false;
  bool dgks = false;      // CGS with the DGKS test against the basis (configure): the host takes the second-pass decision (collect)
  DevBuf<T> work[2];      // defer: w_k lives in work[k & 1]
  // What is pending between two enqueues — at most ONE of the three, hence one value:
  struct None {};
  struct DeferredIter {  // iteration k ended without its normalisation / publish: they ride in the next operator kernel
    typename Engine<T>::PartialsPending sums;
    double* host;
    const double* alpha;
    int slot;
    int64_t k;
    // what the kernel that normalises w_k into u_out folds and publishes (the next operator kernel, or flush's launch_scale_publish);
    // in ScaleIn's field order: partials, nparts, c1_out, alpha, c0, host, u_out (a field added there must be added here)
    static_assert(sizeof(ScaleIn<T>) == 7 * sizeof(void*), "ScaleIn has changed: revisit scale_in");
    ScaleIn<T> scale_in(T* u_out) const { return ScaleIn<T>{sums.partials, sums.nparts, sums.c1, alpha, sums.c0, host, u_out}; }
  };
  struct LaggedIter {  // iteration k ended with the raw w_k: its late update rides in the next sweep (see below)
    int64_t k;
    const double* c1;
  };
  struct PairIter {  // two raw vectors r[0] -> u_P, r[1] -> u_{P+1} (pair form, see below)
    int64_t P = 0;                              // Lanczos vectors complete in the basis
    const T* r[2] = {nullptr, nullptr};
    const double* g[2] = {nullptr, nullptr};    // reals * K measured coefficients each; g[1] is followed by gam = <u_P, r[1]> (reals)
    const double* rho2[2] = {nullptr, nullptr}; // squared norms of the orthogonal parts
    int set = 0;                                // which pair of buffers holds r[0] / r[1]: 0 = work, 1 = pwork
    int rec = 0;                                // records pb.rec[2 * rec], pb.rec[2 * rec + 1] hold g[0] / g[1]
  };
  struct BlockIter {  // a_0 .. a_k in their basis slots, raw from a_{blk_k0} on (block form, see below)
    int64_t k = 0;
  };
  std::variant<None, DeferredIter, LaggedIter, PairIter, BlockIter> pending;
  template <typename Kind> const Kind* pending_as() const { return std::get_if<Kind>(&pending); }
  NormRefs refs_prev{nullptr, nullptr, nullptr, 0};
  double t_enqueue = 0.0, t_wait = 0.0;
  int64_t n_second_passes = 0;  // DGKS second passes taken on the host (collect)
  // Lagged block Gram-Schmidt (kernels.hip, lagged_kernel; gs_small.hip on short vectors): ONE sweep over the basis per iteration.  The iteration ends
  // with the raw w_k in work[k & 1], its coefficients g_k = U^H w_k in lb.g[k & 1] and ||w_k||^2 - |g_k|^2 in *LaggedIter::c1; the
  // next iteration's operator kernel takes w_k / beta_k as its input and the next sweep writes the corrected u_k.
  bool lagged = false;
  int64_t n_lagged = 0;     // iterations enqueued in the lagged form (statistics)
  bool lag_ok = false;      // this pass: every iteration so far went through enqueue_lagged (the device copy of T is complete)
  static constexpr int kLaggedMaxLocked = 512;
  // The regions of ctx->h.get() (bind_buffers).  Per parity of k: g (coefficients) and, kTOff further, t (lagged_fold_kernel); then
  // the device copy of alpha / beta and the locked eigenvalues.
  static constexpr size_t kTOff = (size_t)kLaggedMaxCols + 8, kHHalf = 2 * kTOff + 2 * (size_t)Engine<T>::R + 8;
  struct LagBuf {
    double* g[2] = {nullptr, nullptr};  // at 0 and kHHalf
    double* hist_alpha = nullptr;       // at 2 * kHHalf, kTOff entries
    double* hist_beta = nullptr;        // kTOff entries
    double* lambda = nullptr;           // kLaggedMaxLocked entries
    static constexpr size_t kDoubles = 2 * kHHalf + 2 * kTOff + (size_t)kLaggedMaxLocked;
  } lb;
  double lag_beta2_min = 0.0;  // passes with locked vectors: smallest beta^2 the one-sweep form accepts (begin_pass)
  int64_t n_locked = 0;       // locked eigenvectors at the front of every run list (restart passes)
  const T* locked = nullptr;
  int64_t ld = 0;
  int64_t small_bytes = 0;

  // Pair form (gs_pair.hip, gs_small.hip; tools/pair_gs_model.py): TWO iterations per sweep over the basis.  State between
  // sweeps (PairIter): u_0 .. u_{P-1} complete in the basis; two raw vectors pending, r[0] -> u_P and r[1] -> u_{P+1}, with their
  // measured coefficients (g[0]; g[1] followed by <u_P, r[1]>) and the squared norms of their orthogonal parts (rho2[0], rho2[1]).
  int64_t max_k_hint = 0;     // the loop's max_iteration (sizes the sweeps' partial sums up front, begin_pass)
  bool pair_enabled = false;
  bool pair_allowed = true;   // this pass: a coefficient above kGate switches the form off for the rest of the pass
  int64_t n_pair = 0;         // iterations enqueued in the pair form (statistics; includes speculative ones that were dropped)
  int64_t n_gate_trips = 0;   // passes that left the pair form through the coefficient gate
  DevBuf<T> pwork[2];         // with work[0..1]: the four raw vectors of a pair
  DevBuf<T> psplit;           // hand-over vector of a split sweep (more stored vectors than one launch sums columns for)
  static constexpr size_t kPresizeCols = 4096;  // columns the sweeps' partial sums are sized for at pass start
  DevBuf<double> pbuf;        // coefficient records, predictions, scalars (its own allocation: ctx->h.get() may move)
  static constexpr size_t kPairRec = (size_t)kLaggedMaxCols + 32;
  struct PairBuf {            // the regions of pbuf, in this order (enable_pair)
    double* rec[4] = {nullptr, nullptr, nullptr, nullptr};  // coefficient records, kPairRec each
    double* zero = nullptr;   // a record of zeros
    double *p3 = nullptr, *p4 = nullptr;  // predictions, a record each
    double* fold = nullptr;   // fold scratch, a record
    double* cols = nullptr;   // folded columns (two per stored vector: twice a record)
    double* scal = nullptr;   // 64 scalars: [0] = 1 (rho1^2 of a vector that is already complete); [8 + 2 i], [9 + 2 i]: rho^2 pair i
                              // (alternating); [16 ..]: |r3|^2, <r1, r3>
    static constexpr size_t kDoubles = 10 * kPairRec + 64;
  } pb;
  bool slot_pair[kRingSlots] = {};                    // the scalars of this ring slot came from a pair or block fold (its gate is valid)
  static_assert(kRingSlots == 16 && kScalNorms >= kScalAlpha + kRingSlots && kScalScratch >= kScalNorms + 3 * kRingSlots,
                "the rings of the device scalar area follow kRingSlots");
  int ev_of_slot[kRingSlots] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};  // the event that covers a ring slot's scalars (the slots of a pair or block share one)
  // Block form (gs_block.hip; tools/block_gs_model.py): UP TO EIGHT iterations per sweep over a basis that is never rewritten.  The
  // slots U.vec(j), j >= blk_k0, hold the RAW three-term vectors a_j; bb.rho2[j] and row j of the packed triangle bb.cpk (at
  // R j (j - 1) / 2) hold rho_j^2 and the measured coefficients C_j[l] = <u_l, a_j>, and the orthonormal u_j = (a_j - sum_l C_j[l] u_l)
  // / rho_j exist only implicitly: the Ritz GEMV takes transformed coefficients (ritz_basis), and leaving the form completes the raw
  // vectors in place with one multi-axpy each (block_flush: an O(P^2) pass over the basis — a gate trip, a DGKS repair or the
  // pair_max_stored hook, none of which an ordinary pass meets).  That cost and the R K^2 / 2 coefficients are why the form is
  // bounded by kBlockMaxVecs vectors and only taken by passes whose max_iteration stays within the bound (configure); the others
  // keep the pair form.
  bool block_enabled = false;
  bool block_allowed = true;   // this pass: a gate trip switches the form off for the rest of the pass
  int64_t blk_k0 = 0;          // first raw vector of the pass (the vectors in front of it are complete: rho = 1, zero rows)
  int64_t n_block = 0;         // iterations enqueued in the block form (statistics)
  int64_t n_block_flushed = 0; // raw vectors completed by block_flush (statistics: multi-axpys over the basis)
  int64_t n_block8 = 0;        // ... of n_block: iterations enqueued eight to a sweep (statistics)
  int blk_quiet = 0;           // this pass: collected block iterations in a row whose gate value stayed <= kBlock8Tau (the guard of
                               // the blocks of eight, ll_internal.hpp; collect counts, enqueue_block_f64 asks for kBlock8Quiet)
  DevBuf<double> bbuf;
  DevBuf<T> bsplit[2];         // hand-over vectors of a split block sweep
  struct BlockBuf {            // the regions of bbuf (enable_block)
    double* rho2 = nullptr;    // cap entries
    double* cpk = nullptr;     // packed rows 0 .. cap - 1
    double* dk = nullptr;      // predict scratch, a record
    double* p = nullptr;       // predictions, kBlockMaxM records
    double *prA = nullptr, *prB = nullptr;    // compensation coefficients, a record each
    double *raw0 = nullptr, *raw1 = nullptr;  // fold scratch, a record each
    double* cols = nullptr;    // folded columns: kBlockMaxM records and the Gram tail
    double* nsq = nullptr;     // |b_s|^2 (and <x_prev, b_s>) of the block's three-term updates, 4 doubles apart
    int64_t cap = 0;           // vectors the records are sized for
    size_t rec = 0;            // doubles per record
  } bb;
  static size_t block_row_at(int64_t j) { return ll::block_row_at(Engine<T>::R, j); }
  void enable_block() {
    constexpr size_t R = (size_t)Engine<T>::R;
    block_enabled = true;
    bb.cap = std::min<int64_t>(max_k_hint, (int64_t)kBlockMaxVecs) + 8;
    bb.rec = R * (size_t)(bb.cap + 8);
    const size_t tri = block_row_at(bb.cap) + R * (size_t)bb.cap;
    constexpr size_t kTail = R * (size_t)(kBlockMaxM * (kBlockMaxM - 1) / 2) + (size_t)kBlockMaxM;  // Gram triangle and norms
    bbuf.alloc(E.ctx, (size_t)bb.cap + tri + (5 + 2 * (size_t)kBlockMaxM) * bb.rec + kTail + 4 * (size_t)kBlockMaxM + 32);
    double* b = bbuf.p;
    bb.rho2 = carve(b, (size_t)bb.cap);
    bb.cpk = carve(b, tri);
    bb.dk = carve(b, bb.rec);
    bb.p = carve(b, (size_t)kBlockMaxM * bb.rec);
    bb.prA = carve(b, bb.rec);
    bb.prB = carve(b, bb.rec);
    bb.raw0 = carve(b, bb.rec);
    bb.raw1 = carve(b, bb.rec);
    bb.cols = carve(b, (size_t)kBlockMaxM * bb.rec + kTail);
    bb.nsq = carve(b, 4 * (size_t)kBlockMaxM);
  }
  // the gate of the pair form: what is neglected is the SQUARE of a relative coefficient, which must stay below the rounding of the
  // storage type (float vectors carry coefficients of ~1e-6 by rounding alone)
  static constexpr double kGate = sizeof(typename scalar_traits<T>::real) == 4 ? 2e-4 : kPairGate;
  // Pointer table of the software-pipelined sweep (gs_pair.hip, pair_sweep_pipe_kernel): entry c = stored column c of this pass —
  // the locked eigenvectors, then u_0, u_1, ... — written on the device, slab by slab (launch_fill_ptrs), when a pass starts and
  // whenever the basis has grown by a slab.
  DevBuf<const T*> vtab;
  static constexpr size_t kVtabCap = (size_t)kLaggedMaxCols + (size_t)kLaggedMaxLocked + 64;
  size_t vtab_chunks = 0;     // slabs of U whose slots are in the table
  void vtab_begin_pass() {
    if (!vtab.p) return;
    launch_fill_ptrs<T>(vtab.p, 0, (int)std::min<int64_t>(n_locked, (int64_t)kVtabCap), locked, ld, s);
    vtab_chunks = 0;
  }
  const T* const* vtab_sync() {
    if (!vtab.p) return nullptr;
    for (; vtab_chunks < U.chunks.size(); ++vtab_chunks) {
      const int64_t start = n_locked + (int64_t)vtab_chunks * U.chunk_vecs;
      const int64_t count = std::min<int64_t>(U.chunk_vecs, (int64_t)kVtabCap - start);
      launch_fill_ptrs<T>(vtab.p, (int)start, (int)count, U.chunks[vtab_chunks], ld, s);
    }
    return vtab.p;
  }

  LoopState(Engine<T>& e, Basis<T>& u, EventRing& r, PhaseTimer& t, int64_t n_local, hipStream_t st)
      : E(e), U(u), ring(r), timer(t), nl(n_local), s(st) {}
  // Which forms this run may take.  orth_dgks: Gram-Schmidt against the basis in the CGS form with the DGKS test, which the one-sweep
  // forms and the host's second-pass decision (collect) need; defer_ok: the deferred normalisation without it (a loop without
  // Gram-Schmidt: the Exponentiator without full_orthogonalize).
  void configure(int64_t ld_, int64_t max_iteration, bool orth_dgks, bool defer_ok) {
    const Tuning& tune = E.ctx->tune;
    ld = ld_;
    max_k_hint = max_iteration;
    small_bytes = tune.blas_small_bytes;
    dgks = orth_dgks;
    // Two launches per iteration less on single-GPU runs: alpha is folded by the multi-dot that needs it, and the fold of
    // the post-pass norm + the publish step ride in the normalisation kernel.  LL_FUSE_LAUNCHES=0: separate kernels (A/B).
    fuse_launches = tune.fuse_launches;
    defer = E.can_defer_scale() && fuse_launches && (orth_dgks || defer_ok);
    lagged = E.can_scale_input() && fuse_launches && tune.lagged_gs && orth_dgks;
    if (defer || lagged)
      for (auto& w : work) w.alloc(E.ctx, (size_t)ld);
    if (lagged) bind_buffers();
    // two iterations per sweep (device operators, streaming vectors; enqueue_pair decides per iteration)
    if (lagged && tune.pair_gs && vec_bytes() >= pair_min_bytes()) enable_pair();
    // up to eight per sweep over a raw basis: where the pipelined pair sweep runs (pointer table, streaming vectors: enqueue_block
    // decides), double precision, one rank, and only for passes that cannot outgrow the form's bound
    if (pair_enabled && tune.block_gs && vtab.p && sizeof(typename scalar_traits<T>::real) == 8 && E.ctx->comm == nullptr &&
        max_iteration >= 1 && max_iteration <= (int64_t)kBlockMaxVecs)
      enable_block();
  }
  // the vector length the forms are chosen by (sharded: the shard stride, the same on every rank)
  int64_t vec_bytes() const { return (E.ctx->comm != nullptr ? E.op->n_shard : nl) * (int64_t)sizeof(T); }
  // from this length on the BLAS kernels take the streaming geometry
  int64_t stream_bytes() const { return std::min<int64_t>(small_bytes, (int64_t)1 << 20); }
  // The shortest vector of a one-sweep form: form_min by default, the lagged_min_bytes key if set; the streaming geometry at most.
  int64_t min_bytes(int64_t form_min) const {
    const int64_t tuned = E.ctx->tune.lagged_min_bytes;
    return std::min<int64_t>(stream_bytes(), tuned >= 0 ? tuned : form_min);
  }
  // Below the streaming geometry, down to 320 KiB, the one-sweep kernel of the small-vector geometry (lagged_small_kernel): four
  // launches per iteration against the three of the two small-vector sweeps, but one pass over the basis: Laplacian, window 100:
  // n = 5.0e4 20.8 -> 25.8 k it/s, 1.0e5 18.3 -> 21.0 k; n = 3.0e4 26.3 -> 25.3 k and n = 1e4 26.4 -> 19.1 k would lose
  // (profiles/r03_small_vector_kernel_gaps.txt).
  int64_t lagged_min_bytes() const { return min_bytes((int64_t)320 << 10); }
  // Below the streaming geometry the pair sweep runs in the small-vector geometry (pair_small_kernel: four waves per 1 KiB strip split
  // the stored vectors), one launch, as many columns as 64 KiB of LDS hold (Laplacian, window 100, it/s with / without the pair form:
  // n = 5.0e4 (401 KB) 25.8 k / 26.3 k, n = 1.0e5 (800 KB) 24.3 k / 20.9 k: seven launches per pair against four per iteration, half
  // the basis traffic — the pair form takes over from 512 KiB).
  int64_t pair_min_bytes() const { return min_bytes((int64_t)512 << 10); }
  double* pinned_slot(int slot) const { return E.ctx->pinned.get() + kSlotScalars * slot; }
  double* pinned_gate(int slot) const { return E.ctx->pinned.get() + kGateAt + slot; }
  void enable_pair() {
    pair_enabled = true;
    for (auto& w : pwork)
      if (!w.p) w.alloc(E.ctx, (size_t)ld);
    pbuf.alloc(E.ctx, PairBuf::kDoubles);
    if (E.ctx->tune.sweep_pipeline > 0) vtab.alloc(E.ctx, kVtabCap);
    double* b = pbuf.p;
    for (auto& r : pb.rec) r = carve(b, kPairRec);
    pb.zero = carve(b, kPairRec);
    pb.p3 = carve(b, kPairRec);
    pb.p4 = carve(b, kPairRec);
    pb.fold = carve(b, kPairRec);
    pb.cols = carve(b, 2 * kPairRec);
    pb.scal = carve(b, 64);
    LL_HIP(hipMemsetAsync(pb.zero, 0, kPairRec * sizeof(double), s));
    launch_set_scalar(pb.scal + 0, 1.0, s);
  }
  // partial sums of the sweeps: sized at pass start for up to kPresizeCols columns (begin_pass); beyond that in powers of two —
  // every growth is a hipFree, i.e. a device synchronisation
  void want_partial_cols(size_t cols) {
    if (cols > kPresizeCols) {
      size_t p2 = kPresizeCols;
      while (p2 < cols) p2 *= 2;
      cols = p2;
    }
    E.ctx->ensure_partials((size_t)kMaxGrid * cols);
  }
  // Everything up front: growing ctx->h.get() in the middle of a pass would free the pending coefficients (layout: LagBuf).
  // Called again at the start of every pass: a two-sweep iteration with more than ~7000 coefficient
  // columns (Engine::orth) may have grown, i.e. moved, ctx->h.get() since.
  void bind_buffers() {
    E.ctx->ensure_h(LagBuf::kDoubles);
    double* b = E.ctx->h.get();
    for (auto& g : lb.g) g = carve(b, kHHalf);
    lb.hist_alpha = carve(b, kTOff);
    lb.hist_beta = carve(b, kTOff);
    lb.lambda = carve(b, (size_t)kLaggedMaxLocked);
  }
  // a new Lanczos pass: k restarts at 1.  The compensation of the lagged form needs the image under the operator of every
  // vector it orthogonalises against: the recurrence for the Lanczos vectors, lambda_i z_i for a locked EIGENvector
  // (lambda_shifted: eigenvalues of the operator the loop applies, i.e. including eigenvalue_offset).  A caller's
  // arbitrary orthogonalizeTo vectors (run_iteration) have no such relation: lambda_shifted = nullptr keeps the
  // two-sweep form for that pass.
  // What the compensation neglects for a locked column is c_z r with r = A z - lambda z and c_z ~ ||r|| / beta, i.e. the
  // SQUARE of the locked vector's residual: it is measured here (one operator application per locked vector and pass) and
  // the pass takes the one-sweep form only if every ||r_i|| <= 3e-8 max|lambda| (effect on the recurrence ~ 1e-15 max|lambda|
  // at a typical beta).  Ritz vectors of clustered or degenerate eigenvalues, or of a pass cut off by max_iteration, do not meet
  // that and keep the two-sweep form.  All numbers are all-reduced: the same decision on every rank.
  // norm_scale: a rank-independent estimate of the OPERATOR's size (the previous passes' ||T||_inf, lanczos_run: at least
  // ||A + offset||_2 restricted to the Krylov space, at most 3 x ||A + offset||_2 — so "3e-8 scale" below means at most
  // 9e-8 ||A + offset||_2 and the neglected term at most ~1e-14 ||A + offset||_2 at a typical beta): the gate is
  // relative to the OPERATOR's size, not to max|lambda + offset|, which collapses when a locked eigenvalue sits near -offset.
  // refs0: the norm of the start vector u_0 (the first three-term update reads it as beta_0^2).
  void begin_pass(const NormRefs& refs0, const T* locked_vecs, int64_t n_lock, const double* lambda_shifted = nullptr,
                  double offset = 0.0, double norm_scale = 0.0) {
    refs_prev = refs0;
    pending = None{};
    locked = locked_vecs;
    n_locked = n_lock;
    pair_allowed = true;
    block_allowed = true;
    blk_k0 = 0;
    blk_quiet = 0;
    for (auto& b : slot_pair) b = false;
    // (lambda_shifted == nullptr with locked vectors — a caller's orthogonalizeTo list, run_iteration LL:216-220,259: their Rayleigh
    // quotients theta_i = <z_i, (A + offset) z_i> are MEASURED below and take the eigenvalues' place; the residual gate then decides
    // whether the list consists of eigenvectors to the accuracy the one-sweep forms need)
    lag_ok = lagged && n_lock <= kLaggedMaxLocked;
    lag_beta2_min = 0.0;
    if (lag_ok) vtab_begin_pass();
    if (lagged) {
      bind_buffers();
      // The partial sums of the sweeps — one column per coefficient, kMaxGrid rows — are sized HERE for the longest basis this pass can
      // reach (max_k_hint: max_iteration; the column limits of the one-sweep forms bound it): growing them in the loop means a
      // hipFree, i.e. a device synchronisation, plus a hipMalloc a dozen times in a run's first call on a context (geometric growth
      // up to 600 columns for config 3's 301 iterations) — 0.5-0.7 s of the 1.15-1.37 s that call took on some boxes of round 5,
      // against 0.62 s for the second call.
      constexpr size_t R = (size_t)Engine<T>::R;
      const size_t reach = (size_t)std::max<int64_t>(0, std::min<int64_t>(max_k_hint, (int64_t)kLaggedMaxCols)) + (size_t)n_lock + 2;
      const size_t cols = std::min<size_t>(kPresizeCols, (block_enabled ? (size_t)E.ctx->tune.block_gs_max : 2) * R * reach + 6 * R + 4);  // (longer runs: powers of two, enqueue_pair)
      E.ctx->ensure_partials((size_t)kMaxGrid * cols);
    }
    if (!lag_ok || n_lock == 0) return;
    const bool measure_theta = lambda_shifted == nullptr;
    if (!measure_theta) {
      LL_HIP(hipMemcpyAsync(lb.lambda, lambda_shifted, (size_t)n_lock * sizeof(double), hipMemcpyHostToDevice, s));
      LL_HIP(hipStreamSynchronize(s));  // (pageable source: the caller's array may go away)
    }
    const BasisSegs<T> none = no_segs<T>(ld);
    E.ctx->ensure_partials(kMaxGrid);
    double* r2_dev = lb.g[0];  // free until the first iteration of the pass: ||A z_i - lambda_i z_i||^2, i < n_lock
    for (int64_t i = 0; i < n_lock; ++i) {
      const T* z = locked + i * ld;
      T* y = work[0].p;
      E.apply(z, y, offset, measure_theta ? lb.lambda + i : nullptr, true);  // (theta_i = Re <z_i, y>: the fused dot of the operator kernel)
      const ThreeTerm<T> tt{nullptr, z, lb.lambda + i, NormRefs{nullptr, nullptr, nullptr, 0}};  // y <- y - lambda_i z, ||y||^2
      const int grid = launch_mdot<T>(nl, y, none, tt, nullptr, E.ctx->partials.get(), small_bytes, s);
      launch_reduce_cols(E.ctx->partials.get(), grid, 1, r2_dev + i, nullptr, s);
    }
    E.all_reduce(r2_dev, (size_t)n_lock);  // one collective and one fetch for all locked vectors
    std::vector<double> r2((size_t)n_lock), theta;
    E.fetch(r2_dev, r2.data(), (size_t)n_lock);
    if (measure_theta) {
      theta.resize((size_t)n_lock);
      E.fetch(lb.lambda, theta.data(), (size_t)n_lock);
      lambda_shifted = theta.data();
    }
    double scale = norm_scale, worst = 0.0;
    for (int64_t i = 0; i < n_lock; ++i) {
      worst = std::max(worst, std::sqrt(std::max(r2[(size_t)i], 0.0)));
      scale = std::max(scale, std::fabs(lambda_shifted[i]));
    }
    if (!(worst <= 3e-8 * scale)) {
      lag_ok = false;
      return;
    }
    // c_z ~ ||r|| / beta: the neglected term is <= ||r||^2 / beta; below this beta^2 it would exceed 1e-13 scale and the
    // loop leaves the one-sweep form for the rest of the pass (collect)
    const double bmin = worst * worst / (1e-13 * scale);
    lag_beta2_min = bmin * bmin;
  }
  RunList<T> basis_runs(int64_t count) {  // locked vectors, then u_0 .. u_{count-1}
    RunList<T> runs;
    runs.ld = ld;
    runs.add(locked, n_locked);
    runs.add_basis(U, count);
    return runs;
  }
  // the event of ring slot `slot` covers that slot's scalars: recorded here unless the launcher hung it on its kernel (taken)
  void slot_event(int slot, bool taken = false) {
    ev_of_slot[slot] = slot;
    if (!taken) LL_HIP(hipEventRecord(ring.ev[slot], s));
  }
  // iteration k's three-term update w -= alpha u_{k-1} + beta u_{k-2}; where apply left alpha's partial sums (da), the multi-dot folds them
  ThreeTerm<T> three_term(int64_t k, int slot, const typename Engine<T>::DeferredAlpha& da) {
    ThreeTerm<T> tt{k > 1 ? U.vec(k - 2) : nullptr, U.vec(k - 1), E.S(kScalAlpha + slot), refs_prev};
    if (da.nparts > 0) {
      tt.alpha_partials = da.partials;
      tt.alpha_nparts = da.nparts;
      tt.alpha_out = E.S(kScalAlpha + slot);
    }
    return tt;
  }
  // dst -= [locked, u_0 .. u_{j-1}] c with the device coefficients c (reals per stored vector): one multi-axpy per launch group
  void subtract_basis(T* dst, int64_t j, const double* c) {
    const RunList<T> runs = basis_runs(j);
    int off = 0;
    for (auto& grp : runs.groups(max_vecs_per_launch<T>())) {
      launch_maxpy<T>(nl, dst, grp, c + Engine<T>::R * off, nullptr, E.ctx->partials.get(), small_bytes, s);
      off += grp.total();
    }
  }
  // u_j = (raw - [locked, u_0 .. u_{j-1}] g) / rho in its basis slot, with the two-sweep kernels: a raw vector completed with its
  // measured coefficients g (reals per stored vector) and the squared norm *rho2 of its orthogonal part
  void complete_raw(int64_t j, const T* raw, const double* g, const double* rho2) {
    T* dst = U.vec(j);
    if (dst != raw) LL_HIP(hipMemcpyAsync(dst, raw, (size_t)nl * sizeof(T), hipMemcpyDeviceToDevice, s));
    subtract_basis(dst, j, g);
    const NormRefs nr{rho2, rho2, rho2, 0};
    launch_scale<T>(nl, dst, 0.0, &nr, s);
  }
  // u_k = (w - U g) / beta with the two-sweep kernels: the pending late update, applied now (the vector is needed
  // complete: a second Gram-Schmidt pass on it, or the loop leaves the lagged form)
  void flush_lag() {
    const LaggedIter* lg = pending_as<LaggedIter>();
    if (!lg) return;
    complete_raw(lg->k, work[lg->k & 1].p, lb.g[lg->k & 1], lg->c1);
    pending = None{};
  }
  // u_j must be complete in its basis slot (second Gram-Schmidt pass on it)
  void make_final(int64_t j) {
    if (const PairIter* pr = pending_as<PairIter>()) {
      if (j >= pr->P) pair_flush(j + 1);
    } else if (pending_as<BlockIter>()) {
      block_flush(j);
    } else if (const LaggedIter* lg = pending_as<LaggedIter>()) {
      if (lg->k == j) flush_lag();
    }
  }
  // Leave the pair form: complete the two pending vectors with their measured coefficients (two-sweep kernels).  Afterwards
  // u_0 .. u_{P+1} are complete, nothing is pending, and iteration P + 2 can be enqueued from a clean state.
  // count: only the vectors u_j with j < count are needed (end of a pass: the Ritz vectors use u_0 .. u_{m-1}; a repair of u_j:
  // nothing behind u_j survives it) — a pending vector beyond that is dropped instead of completed.
  void pair_flush(int64_t count) {
    const PairIter* pr = pending_as<PairIter>();
    if (!pr) return;
    // (g[1]: R * P coefficients against the basis, then <u_P, r[1]>: one contiguous list)
    for (int v = 0; v < 2 && pr->P + v < count; ++v) complete_raw(pr->P + v, pr->r[v], pr->g[v], pr->rho2[v]);
    const double* rho2 = pr->rho2[1];
    pending = None{};
    refs_prev = NormRefs{rho2, rho2, rho2, 0};  // beta^2 of the last completed vector, for the next three-term update
  }
  // Leave whichever of the two forms is pending: the raw vectors among u_0 .. u_{count-1} are completed, those behind are dropped
  void flush_raw(int64_t count = std::numeric_limits<int64_t>::max()) {
    if (pending_as<BlockIter>()) block_flush(count - 1);
    else pair_flush(count);
  }
  BlockRows fetch_block_rows(int64_t end) {
    BlockRows br;
    br.R = Engine<T>::R;
    br.k0 = blk_k0;
    br.end = std::max(end, blk_k0);
    const size_t cnt = (size_t)(br.end - br.k0);
    if (cnt == 0) return br;
    br.rows.resize(block_row_at(br.end) - block_row_at(br.k0) + 1);
    br.rho.resize(cnt);
    if (br.rows.size() > 1) E.fetch(bb.cpk + block_row_at(br.k0), br.rows.data(), br.rows.size() - 1);
    E.fetch(bb.rho2 + br.k0, br.rho.data(), cnt);
    for (auto& r : br.rho) r = std::sqrt(r);
    return br;
  }
  // Leave the block form: the raw vectors a_k0 .. a_last are completed and normalised IN PLACE, from the highest index down —
  //   u_j = (a_j - sum_{l<j} (C_j[l] / rho_l) a_l) / rho_j    (first order in C)
  // uses only raw vectors of lower index, which the descending order has not touched yet.  Whatever lies behind a_last (later vectors
  // of a block that a gate, a repair or a stop cut) is dropped.  One multi-axpy over the basis per raw vector.
  void block_flush(int64_t last) {
    const BlockIter* bi = pending_as<BlockIter>();
    if (!bi) return;
    last = std::min(last, bi->k);
    if (last >= blk_k0) {
      BlockRows br = fetch_block_rows(last + 1);
      block_rows_over_raw(br, last);
      if (br.rows.size() > 1) {
        LL_HIP(hipMemcpyAsync(bb.cpk + block_row_at(br.k0), br.rows.data(), (br.rows.size() - 1) * sizeof(double), hipMemcpyHostToDevice, s));
        LL_HIP(hipStreamSynchronize(s));  // (pageable source)
      }
      for (int64_t j = last; j >= br.k0; --j) {
        T* dst = U.vec(j);
        subtract_basis(dst, j, bb.cpk + block_row_at(j));
        launch_scale<T>(nl, dst, 1.0 / br.rho[(size_t)(j - br.k0)], nullptr, s);
        ++n_block_flushed;
      }
    }
    const double* r2 = bb.rho2 + std::max<int64_t>(last, 0);
    pending = None{};
    refs_prev = NormRefs{r2, r2, r2, 0};  // beta^2 of the last completed vector, for the next three-term update
  }
  // End of a pass with raw vectors pending: of the u_0 .. u_{count-1} the Ritz vectors need, u_P (and u_{P+1}) of a pair, or a_k0 .. of a
  // block, exist only as raw vectors with their measured coefficients.  Instead of completing them (flush_raw: the whole basis read once
  // per pending vector — 1.4 ms of a 131 ms step on config 3), ritz_basis folds the late update into the GEMV's COEFFICIENTS (raw_basis.hpp).
  struct Tail {
    PairIter pair;
    int nvec = 0;  // pending vectors the result needs (0: none, no tail; 1: u_P; 2: u_P and u_{P+1})
    bool block = false;  // the basis is raw: the GEMV's coefficients are transformed with `rows`
    BlockRows rows;
  };
  Tail take_tail(int64_t count) {
    Tail t;
    if (const BlockIter* bi = pending_as<BlockIter>()) {
      t.block = true;
      t.rows = fetch_block_rows(std::min<int64_t>(count, bi->k + 1));
      pending = None{};
      return t;
    }
    if (const PairIter* pr = pending_as<PairIter>()) {
      t.pair = *pr;
      t.nvec = (int)std::max<int64_t>(0, std::min<int64_t>(2, count - pr->P));
      pending = None{};
    }
    return t;
  }
  // The end of a pass, the one entry of both drivers: what is raw among u_0 .. u_{count-1} goes into the returned tail, or is completed
  // first (flush_raw): with ritz_tail = 0 (A/B), and a pair where the caller takes no pair tail (the Exponentiator calls its GEMV with m columns).
  Tail end_pass(int64_t count, bool pair_tail_ok) {
    if (!E.ctx->tune.ritz_tail || !(pair_tail_ok || pending_as<BlockIter>())) flush_raw(count);
    return take_tail(count);
  }
  // The GEMV of the Ritz vectors x_w = sum_{k<m} s_wk u_k (coeff: nw rows of m): returns the basis runs the GEMV reads and rewrites
  // coeff to match them, one row of runs.total() per vector.  Without a pair tail those are u_0 .. u_{m-1} (raw from a_k0 on with a
  // block tail); with one, the stored columns of the last sweep (locked vectors first, then u_0 .. u_{P-1}), then r1 (and r2).
  RunList<T> ritz_basis(const Tail& tail, int64_t m, int64_t nw, std::vector<T>& coeff) {
    RunList<T> basis;
    basis.ld = ld;
    if (tail.block || tail.nvec == 0) {
      if (tail.block) block_coeff_over_raw(tail.rows, m, nw, coeff.data());
      basis.add_basis(U, m);
      return basis;
    }
    constexpr int R = Engine<T>::R;
    const int64_t Pt = tail.pair.P, K = n_locked + Pt;
    std::vector<double> g1h((size_t)R * K + 1), g2h((size_t)R * (K + 1) + 1), rho(2, 1.0);
    if (K > 0) E.fetch(tail.pair.g[0], g1h.data(), (size_t)R * K);
    E.fetch(tail.pair.g[1], g2h.data(), (size_t)R * (K + 1));
    E.fetch(tail.pair.rho2[0], &rho[0], 1);
    E.fetch(tail.pair.rho2[1], &rho[1], 1);
    coeff = pair_coeff_over_raw(R, g1h, g2h, std::sqrt(rho[0]), std::sqrt(rho[1]), n_locked, Pt, tail.nvec, m, nw, coeff);
    basis = basis_runs(Pt);
    basis.add(tail.pair.r[0], 1);
    if (tail.nvec == 2) basis.add(tail.pair.r[1], 1);
    return basis;
  }
  // Iterations kk .. kk + m - 1 in the block form: m = 8 in real double where the guard admits it (blk_quiet; key block_gs_max = 4: never), else 4,
  // and 4, 2 or 1 where fewer remain before max_iteration.  Entered from the
  // one-sweep state (iteration kk - 1 pending with its measured coefficients, u_0 .. u_{kk-2} complete) or continued from a block.
  // Returns m; 0: not taken.
  int64_t enqueue_block(int64_t kk, double offset) {
    if constexpr (sizeof(typename scalar_traits<T>::real) == 8) return enqueue_block_f64(kk, offset);
    else return 0;  // (single precision keeps the pair form: the block kernels, and enqueue_block_f64, exist for double and complex double)
  }
  int64_t enqueue_block_f64(int64_t kk, double offset) {
    constexpr int R = Engine<T>::R;
    const Tuning& tune = E.ctx->tune;
    if (!block_enabled || !block_allowed || !pair_allowed || !lag_ok || n_locked != 0) return 0;
    const BlockIter* const bi = pending_as<BlockIter>();
    const LaggedIter* const lg = pending_as<LaggedIter>();
    int64_t k;  // index of the last stored vector
    if (bi) {
      if (bi->k + 1 != kk) return 0;
      k = bi->k;
    } else if (lg && lg->k == kk - 1 && kk >= 3) {
      k = kk - 1;
    } else {
      return 0;
    }
    const int64_t remaining = max_k_hint - (kk - 1);  // never beyond the loop's max_iteration
    if (remaining < 1) return 0;
    // (complex double keeps blocks of four: its sweep of eight needs 264 registers, one wave per SIMD, and no rate of it has been measured)
    const bool eight = !scalar_traits<T>::is_complex && tune.block_gs_max >= 8 && remaining >= 8 && blk_quiet >= kBlock8Quiet;
    const int m = eight ? 8 : (remaining >= 4 ? 4 : (remaining >= 2 ? 2 : 1));
    // the streaming geometry of the pipelined pair sweep (launch_pair_sweep), within the records
    const int64_t strips16k = (nl * (int64_t)sizeof(T) + 16383) / 16384;
    const bool streaming = tune.sweep_pipeline >= 2 || strips16k > 2 * kCUs + kCUs / 4;
    if (!streaming || vec_bytes() < stream_bytes() || k + m + 1 > bb.cap || (size_t)(k + m + 1) > kVtabCap) return 0;
    if (tune.pair_max_stored > 0 && k + 1 > tune.pair_max_stored) return 0;  // (test hook: the hand-over to the one-sweep form)
    const int W = (int)(k + 1);
    const int ncols = m * R * W + R * m * (m - 1) / 2 + m;
    int per_launch = block_sweep_max_vecs<T>(m);
    if (tune.pair_split_vecs > 0) per_launch = std::min(per_launch, std::max(1, tune.pair_split_vecs));
    if (W > per_launch)
      for (auto& b : bsplit)
        if (!b.p) b.alloc(E.ctx, (size_t)ld);
    const double te0 = now_s();
    want_partial_cols((size_t)std::max(ncols, 1 + R));
    if (!bi) {  // a_k moves from its work buffer into its basis slot; the records start here
      LL_HIP(hipMemcpyAsync(U.vec(k), work[k & 1].p, (size_t)nl * sizeof(T), hipMemcpyDeviceToDevice, s));
      launch_block_enter((int)k, R, lb.g[k & 1], lg->c1, bb.rho2, bb.cpk, s);
      blk_k0 = k;
    }
    BlockVecs<T> bv{};
    for (int i = 0; i < m; ++i) bv.b[i] = U.vec(k + 1 + i);  // (may add a slab: the pointer table is brought up to date after it)
    bv.part[0] = bsplit[0].p;
    bv.part[1] = bsplit[1].p;
    const T* const* vt = vtab_sync();
    BlockScalars sc{};
    BlockHost host{};
    int slots[kBlockMaxM] = {};
    for (int i = 0; i < kBlockMaxM; ++i) {
      const int ii = std::min(i, m - 1);
      slots[i] = (int)((kk + ii) % kRingSlots);
      sc.e[i] = E.S(kScalAlpha + slots[i]);
      sc.nsq[i] = bb.nsq + 4 * ii;
      host.slot[i] = pinned_slot(slots[i]);
      host.gate[i] = pinned_gate(slots[i]);
    }
    // ---- m x (operator on the previous vector / its norm, raw three-term update, |b|^2)
    for (int i = 0; i < m; ++i) {
      const T* x = i == 0 ? U.vec(k) : bv.b[i - 1];
      const T* xp = i == 0 ? U.vec(k - 1) : (i == 1 ? U.vec(k) : bv.b[i - 2]);
      const double* xn2 = i == 0 ? bb.rho2 + k : bb.nsq + 4 * (i - 1);
      const double* pn2 = i == 0 ? bb.rho2 + k - 1 : (i == 1 ? bb.rho2 + k : bb.nsq + 4 * (i - 2));
      double* e = E.S(kScalAlpha + slots[i]);
      timer.mark();
      typename Engine<T>::DeferredAlpha da;
      E.apply(x, bv.b[i], offset, e, true, fuse_launches ? &da : nullptr, nullptr, xn2);
      timer.mark();
      const int g3 = launch_pair_three_term<T>(nl, bv.b[i], x, xp, e, da.nparts > 0 ? da.partials : nullptr, da.nparts, xn2, pn2,
                                               E.ctx->partials.get(), false, s);
      launch_reduce_cols(E.ctx->partials.get(), g3, 1 + R, bb.nsq + 4 * i, nullptr, s);
      if (i + 1 < m) timer.mark();
    }
    // ---- one sweep for all of them
    launch_block_predict((int)k, m, R, sc, bb.rho2, bb.cpk, lb.hist_alpha, lb.hist_beta, bb.dk, bb.p, (int)bb.rec, bb.prA, bb.prB, s);
    const int grid = launch_block_sweep<T>(nl, vt, W, m, bv, bb.prA, bb.prB, E.ctx->partials.get(), tune.lagged_pieces, per_launch, s);
    launch_reduce_cols(E.ctx->partials.get(), grid, ncols, bb.cols, nullptr, s);
    const int ev = slots[m - 1];  // ONE event for the block: its scalars are published by the same fold kernel
    launch_block_fold(bb.cols, (int)k, m, R, sc, bb.p, (int)bb.rec, bb.rho2, bb.cpk, lb.hist_alpha, lb.hist_beta, bb.raw0, bb.raw1, host, s,
                      tune.event_in_launch ? ring.ev[ev] : nullptr);
    if (!tune.event_in_launch) LL_HIP(hipEventRecord(ring.ev[ev], s));
    timer.mark();
    for (int i = 0; i < m; ++i) {
      ev_of_slot[slots[i]] = ev;
      slot_pair[slots[i]] = true;
    }
    pending = BlockIter{k + m};
    n_block += m;
    if (m == 8) n_block8 += m;
    if (m >= 2) n_pair += m;  // (iterations that shared a sweep with a neighbour)
    n_lagged += m;
    t_enqueue += now_s() - te0;
    return m;
  }
  // Iterations k and k + 1 in the pair form.  Entered from the one-sweep state (iteration k - 1 pending with its measured
  // coefficients: u_{k-2} plays the part of an already complete first vector, g1 = 0, rho1 = 1) or continued from a pair.
  bool enqueue_pair(int64_t k, double offset) {
    constexpr int R = Engine<T>::R;
    // (restart passes: lag_ok already says that the locked vectors are eigenvectors to the one-sweep form's gate, begin_pass)
    if (!pair_enabled || !pair_allowed || !lag_ok) return false;
    // never beyond the loop's max_iteration: iteration k + 1 would be an operator application the caller did not ask for, and with
    // max_iteration == n its input is the normalised remainder of a vanishing vector; the last odd iteration runs in the one-sweep form
    if (max_k_hint > 0 && k + 1 > max_k_hint) return false;
    const int64_t Lk = n_locked;
    PairIter in;
    if (const PairIter* pr = pending_as<PairIter>()) {
      if (pr->P + 2 != k) return false;
      in = *pr;
    } else if (const LaggedIter* lg = pending_as<LaggedIter>(); lg && lg->k == k - 1 && k >= 3) {
      // g[1]: L + k - 1 = K + 1 coefficients: against the locked vectors and u_0 .. u_{P-1}, then <u_P, r2>; the outputs go to pwork
      // and to the records 0 / 1
      in = PairIter{k - 2, {U.vec(k - 2), work[(k - 1) & 1].p}, {pb.zero, lb.g[(k - 1) & 1]}, {pb.scal + 0, lg->c1}, 0, 1};
    } else {
      return false;
    }
    const int64_t P = in.P;
    const T *const r1 = in.r[0], *const r2 = in.r[1];
    const double *const g1 = in.g[0], *const g2 = in.g[1], *const rho1sq = in.rho2[0], *const rho2sq = in.rho2[1];
    const int out_set = in.set ^ 1, out_rec = in.rec ^ 1;
    const int64_t K = Lk + P;  // stored columns of the sweep
    const int ncols = 2 * R * (int)K + 5 * R + 1;
    // the coefficient records hold reals * (K + 2) (+ reals) numbers, the recorded tridiagonal kLaggedMaxCols + 8 entries; the
    // sweep's 2 reals K + 5 reals + 1 columns are summed in as many launches as one workgroup's LDS asks for (pair_sweep_max_vecs);
    // below the streaming geometry, down to pair_min_bytes, in the small-vector geometry
    const bool small_geometry = vec_bytes() < stream_bytes();
    if ((int64_t)R * (K + 8) > kLaggedMaxCols || vec_bytes() < pair_min_bytes()) return false;
    if (small_geometry && (!pair_small_fits<T>((int)K) || K > max_vecs_per_launch<T>() || basis_runs(P).runs.size() > (size_t)kMaxSegs)) return false;
    if (E.ctx->tune.pair_max_stored > 0 && K > E.ctx->tune.pair_max_stored) return false;  // (test hook: the hand-over to the one-sweep form)
    const RunList<T> stored = basis_runs(P);
    int per_launch = pair_sweep_max_vecs<T>();
    if (E.ctx->tune.pair_split_vecs > 0) per_launch = std::min(per_launch, std::max(1, E.ctx->tune.pair_split_vecs));
    const std::vector<BasisSegs<T>> groups = stored.groups(per_launch);
    if (!small_geometry && groups.size() > 1 && !psplit.p) psplit.alloc(E.ctx, (size_t)ld);
    const double te0 = now_s();
    T* r3 = out_set ? pwork[0].p : work[0].p;
    T* r4 = out_set ? pwork[1].p : work[1].p;
    double* rec3 = pb.rec[2 * out_rec];
    double* rec4 = pb.rec[2 * out_rec + 1];
    double* nxt = pb.scal + 8 + 2 * out_rec;
    double* t3 = pb.scal + 16;  // |r3|^2, <r1, r3>
    const double* gam = g2 + R * K;
    const int sa = (int)(k % kRingSlots), sb = (int)((k + 1) % kRingSlots);
    double* e1 = E.S(kScalAlpha + sa);
    double* e2 = E.S(kScalAlpha + sb);
    want_partial_cols((size_t)std::max(ncols, 1 + R));
    // ---- iteration k: operator on r2 / rho2, three-term with raw vectors
    timer.mark();
    typename Engine<T>::DeferredAlpha da1, da2;
    E.apply(r2, r3, offset, e1, true, fuse_launches ? &da1 : nullptr, nullptr, rho2sq);
    timer.mark();
    // Where the second operator kernel reads x itself (CSR-stream, lattice, dense on one GPU) it folds the three-term kernel's
    // partial sums of |r3|^2 on the fly (ScaleIn, like the deferred normalisation of 3.3) and pair_predict_kernel folds <r1, r3>:
    // no fold launch in between.  The PB / tiled kernels and sharded contexts want the folded scalar (all-reduced).
    const bool fold_in_consumers = fuse_launches && E.can_defer_scale();
    int grid = launch_pair_three_term<T>(nl, r3, r2, r1, e1, da1.nparts > 0 ? da1.partials : nullptr, da1.nparts, rho2sq, rho1sq,
                                         E.ctx->partials.get(), fold_in_consumers, s);
    const int tt_grid = grid;
    if (!fold_in_consumers) {
      launch_reduce_cols(E.ctx->partials.get(), grid, 1 + R, t3, nullptr, s);
      if (E.ctx->comm != nullptr) E.all_reduce(t3, (size_t)(1 + R));  // |r3|^2 and <r1, r3> over the shards
    }
    timer.mark();
    // ---- iteration k + 1: operator on r3 / |r3|; its three-term update is formed inside the sweep
    timer.mark();
    if (fold_in_consumers) {
      ScaleIn<T> sc;
      sc.partials = E.ctx->partials.get();  // column 0: |r3|^2 per workgroup
      sc.nparts = tt_grid;
      sc.c1_out = t3;                   // the folded |r3|^2, for the predict / sweep / fold kernels
      E.apply(r3, r4, offset, e2, true, &da2, &sc, nullptr);
    } else {
      E.apply(r3, r4, offset, e2, true, fuse_launches ? &da2 : nullptr, nullptr, t3);
    }
    timer.mark();
    // ---- one sweep for both
    launch_pair_predict((int)P, (int)Lk, R, g1, g2, rho1sq, rho2sq, gam, t3, fold_in_consumers ? E.ctx->partials.get() : nullptr, tt_grid,
                        e1, e2, da2.nparts > 0 ? da2.partials : nullptr, da2.nparts, lb.hist_alpha, lb.hist_beta, lb.lambda, pb.p3, pb.p4, s);
    T* const uP = U.vec(P);
    T* const uQ = U.vec(P + 1);  // (may add a slab: the pointer table is brought up to date after it)
    if (small_geometry) {
      const BasisSegs<T> none = no_segs<T>(ld);
      const std::vector<BasisSegs<T>> one = stored.groups(max_vecs_per_launch<T>());  // a single group (checked above)
      LL_REQUIRE(launch_pair_sweep_small<T>(nl, one.empty() ? none : one[0], (int)K, r1, r2, r3, r4, uP, uQ, g1, g2, gam, pb.p4, rho1sq, rho2sq,
                                            e2, t3, E.ctx->partials.get(), &grid, s),
                 "internal: the small-geometry pair sweep refused a launch that was checked to fit");
    } else {
      grid = launch_pair_sweep<T>(nl, groups, (int)K, r1, r2, r3, r4, uP, uQ, psplit.p, g1, g2, gam, pb.p4, rho1sq, rho2sq, e2, t3,
                                  E.ctx->partials.get(), E.ctx->tune.lagged_pieces, s, vtab_sync(), E.ctx->tune.sweep_pipeline >= 2);
    }
    launch_reduce_cols(E.ctx->partials.get(), grid, ncols, pb.cols, nullptr, s);
    // sharded: ONE all-reduce carries both iterations' columns; every rank then folds the same numbers to the same bits
    if (E.ctx->comm != nullptr) E.all_reduce(pb.cols, (size_t)ncols);
    launch_pair_fold(pb.cols, (int)P, (int)Lk, R, lb.lambda, pb.p4, g2, gam, rho2sq, t3, e1, e2, rec3, rec4, nxt, lb.hist_alpha, lb.hist_beta, pb.fold,
                     pinned_slot(sa), pinned_slot(sb), pinned_gate(sa), pinned_gate(sb), s,
                     E.ctx->tune.event_in_launch ? ring.ev[sb] : nullptr);
    // ONE event for both iterations of the pair (their scalars are published by the same fold kernel): every event record is a marker
    // packet between two dependent kernels of a loop that is bound by exactly those gaps at small sizes
    if (!E.ctx->tune.event_in_launch) LL_HIP(hipEventRecord(ring.ev[sb], s));
    ev_of_slot[sa] = ev_of_slot[sb] = sb;
    timer.mark();
    slot_pair[sa] = slot_pair[sb] = true;
    pending = PairIter{P + 2, {r3, r4}, {rec3, rec4}, {nxt, nxt + 1}, out_set, out_rec};
    n_pair += 2;
    n_lagged += 2;  // (the pair form is a one-sweep form: ll_run_stats.lagged_iterations counts it, pair_iterations singles it out)
    t_enqueue += now_s() - te0;
    return true;
  }
  bool enqueue_lagged(int64_t k, double offset, int64_t nb_total) {
    constexpr int R = Engine<T>::R;
    if (!lag_ok) return false;
    const LaggedIter* const late = pending_as<LaggedIter>();  // iteration k - 1, if its update is pending
    const double* const prev_c1 = late ? late->c1 : nullptr;
    const RunList<T> in_memory = basis_runs(late ? k - 1 : k);  // u_{k-1} is not in memory while its update is pending
    const std::vector<BasisSegs<T>> groups = in_memory.groups(max_vecs_per_launch<T>());
    // (very short vectors keep the two-sweep form of the small-vector kernels, lagged_min_bytes).  The one sweep of the streaming
    // geometry overtakes the two small-vector sweeps from about 1 MiB per vector, well below the 4 MiB at which the streaming
    // two-sweep kernels do (Laplacian, window 100: n = 2.0e5 14.3 -> 15.4 k it/s, 3.6e5 10.9 -> 14.0 k, 5.0e5 8.5 -> 12.4 k;
    // n = 1.0e5 would lose 5 %; profiles/r03_small_vector_kernel_gaps.txt)
    if (nb_total != k + n_locked || R * nb_total > kLaggedMaxCols || groups.size() > 1 || vec_bytes() < lagged_min_bytes()) {
      lag_ok = false;  // for the rest of the pass: the two-sweep iterations do not record T on the device
      return false;
    }
    const double te0 = now_s();
    const int slot = (int)(k % kRingSlots);
    slot_pair[slot] = false;
    T* y = work[k & 1].p;
    const T* x = late ? work[(k - 1) & 1].p : U.vec(k - 1);
    timer.mark();
    typename Engine<T>::DeferredAlpha da;
    E.apply(x, y, offset, E.S(kScalAlpha + slot), true, fuse_launches ? &da : nullptr, nullptr, prev_c1);
    timer.mark();
    const ThreeTerm<T> tt = three_term(k, slot, da);
    const int ncols = R * (int)nb_total + 1;
    want_partial_cols((size_t)ncols);
    const BasisSegs<T> none = no_segs<T>(ld);
    int grid;
    if (late) {
      const Lagged<T> lg{work[(k - 1) & 1].p, U.vec(k - 1), lb.g[(k - 1) & 1], lb.g[(k - 1) & 1] + kTOff, prev_c1};
      grid = launch_lagged<T>(nl, y, groups.empty() ? none : groups[0], lg, tt, E.ctx->partials.get(), E.ctx->tune.lagged_pieces,
                              stream_bytes(), s);
      ++n_lagged;
    } else {
      grid = launch_mdot<T>(nl, y, groups.empty() ? none : groups[0], tt, nullptr, E.ctx->partials.get(), small_bytes, s);
    }
    double* c = E.S(kScalNorms + 3 * slot);
    double* hb = lb.g[k & 1];
    const double* c0 = c;
    if (E.ctx->comm == nullptr) {
      launch_reduce_cols(E.ctx->partials.get(), grid, ncols, hb, c, s);  // coefficients -> hb, ||w||^2 -> c[0]
    } else {  // one all-reduce for the coefficients and ||w||^2; every rank then folds the same numbers to the same bits
      launch_reduce_cols(E.ctx->partials.get(), grid, ncols, hb, nullptr, s);
      E.all_reduce(hb, (size_t)ncols);
      c0 = hb + R * nb_total;
    }
    const double* pg = late ? lb.g[(k - 1) & 1] : nullptr;
    launch_lagged_fold(hb, (int)nb_total, (int)n_locked, R, hb + kTOff, c0, c, c + 1, E.S(kScalAlpha + slot), pg,
                       pg ? pg + kTOff : nullptr, prev_c1, lb.hist_alpha, lb.hist_beta, lb.lambda, pinned_slot(slot), s,
                       E.ctx->tune.event_in_launch ? ring.ev[slot] : nullptr);
    slot_event(slot, E.ctx->tune.event_in_launch);
    timer.mark();
    pending = LaggedIter{k, c + 1};
    refs_prev = NormRefs{c, c + 1, c + 1, 0};
    t_enqueue += now_s() - te0;
    return true;
  }
  void enqueue(int64_t k, double offset, const RunList<T>& runs, int mode) {
    flush_raw();  // (a pending pair or block is completed first: the forms below start from complete vectors)
    if (mode == LL_ORTH_CGS_DGKS && !pending_as<DeferredIter>() && enqueue_lagged(k, offset, runs.total())) return;
    flush_lag();  // (leaving the lagged form: u_{k-1} must be complete)
    lag_ok = false;
    const double te0 = now_s();
    const int slot = (int)(k % kRingSlots);
    slot_pair[slot] = false;
    const DeferredIter* const prev = pending_as<DeferredIter>();  // iteration k - 1, if its normalisation is pending
    // (then u_{k-1} is still w_{k-1} in its work buffer: this operator kernel normalises it on the fly)
    const T* x = prev ? work[(k - 1) & 1].p : U.vec(k - 1);
    T* y = defer ? work[k & 1].p : U.vec(k);
    const ScaleIn<T> sc = prev ? prev->scale_in(U.vec(k - 1)) : ScaleIn<T>{};
    timer.mark();
    typename Engine<T>::DeferredAlpha da;
    // the operator kernel that publishes iteration k-1's scalars completes that iteration's event itself where its launcher can
    // (LL_LAUNCH_STOP: no marker packet between it and the sweep's first kernel); otherwise the event is recorded behind it
    const bool ev_in_launch = prev && E.ctx->tune.event_in_launch;
    bool ev_taken = false;
    {
      const StopNext stop(E.ctx, ev_in_launch ? ring.ev[prev->slot] : nullptr);
      E.apply(x, y, offset, E.S(kScalAlpha + slot), true, fuse_launches ? &da : nullptr, prev ? &sc : nullptr);  // P0-P3
      ev_taken = ev_in_launch && stop.taken();
    }
    if (prev) {
      slot_event(prev->slot, ev_taken);  // iteration k-1's scalars are on their way to the host
      pending = None{};
    }
    timer.mark();
    const ThreeTerm<T> tt = three_term(k, slot, da);  // P4
    typename Engine<T>::PassRequest req;
    req.host = pinned_slot(slot);
    req.alpha = E.S(kScalAlpha + slot);
    req.caller_normalises = fuse_launches;
    const typename Engine<T>::PassEnd end = E.orth_pass(y, runs, mode, tt, E.S(kScalNorms + 3 * slot), &req);  // P5-P7
    const auto* const sums = std::get_if<typename Engine<T>::PartialsPending>(&end.how);
    if (sums && defer) {  // P8 rides in the next operator kernel
      pending = DeferredIter{*sums, req.host, req.alpha, slot, k};
    } else if (sums) {  // norm fold + publish + normalisation in one launch (P8)
      launch_scale_publish<T>(nl, y, sums->partials, sums->nparts, sums->c1, req.alpha, sums->c0, req.host, s);
      slot_event(slot);
    } else if (const auto* dv = std::get_if<typename Engine<T>::DerivePending>(&end.how)) {  // sharded: derived norm + publish + normalisation in one launch
      launch_scale_derive<T>(nl, y, dv->c0_src, dv->h, dv->count, dv->c0_out, dv->c1, req.alpha, req.host, s);
      slot_event(slot);
    } else {  // folded: w is in its basis slot already
      LL_REQUIRE(!defer, "internal: deferred normalisation needs the fused norm fold");
      if (std::holds_alternative<typename Engine<T>::Folded>(end.how)) launch_publish(req.host, req.alpha, end.refs, s);
      slot_event(slot);
      launch_scale<T>(nl, y, 0.0, &end.refs, s);  // P8
    }
    timer.mark();
    refs_prev = end.refs;
    t_enqueue += now_s() - te0;
  }
  // the pending iteration is the last one: normalise it into its basis slot and publish its scalars now
  void flush() {
    const DeferredIter* const d = pending_as<DeferredIter>();
    if (!d) return;
    const ScaleIn<T> sc = d->scale_in(U.vec(d->k));
    launch_scale_publish<T>(nl, sc.u_out, sc.partials, sc.nparts, sc.c1_out, sc.alpha, sc.c0, sc.host, s, work[d->k & 1].p);
    slot_event(d->slot);
    pending = None{};
  }
  // Enqueue the next iteration(s) from k on: two at once where the pair form applies (one sweep over the basis for both), else
  // one, orthogonalised against the locked vectors and u_0 .. u_{k-1} (full) or against nothing.  Returns how many.
  int64_t enqueue_group(int64_t k, double offset, int mode, bool full) {
    if (dgks && !pending_as<DeferredIter>()) {
      if (const int64_t m = enqueue_block(k, offset)) return m;
      if (enqueue_pair(k, offset)) return 2;
    }
    RunList<T> runs;
    runs.ld = ld;
    if (full) runs = basis_runs(k);
    enqueue(k, offset, runs, mode);
    return 1;
  }
  // Everything enqueued after iteration j is dropped (u_j is final in its basis slot): the next enqueue is j + 1, and its three-term
  // update reads beta_j^2 from iteration j's norm triple.
  void restart_after(int64_t j) {
    pending = None{};
    double* cj = E.S(kScalNorms + 3 * (int)(j % kRingSlots));
    refs_prev = NormRefs{cj, cj + 1, cj + 1, 0};
  }
  // Host half of iteration j, part 1: wait for its four scalars and take the decisions that may change u_j — the DGKS second pass,
  // leaving the one-sweep form, the pair form's gate.  redone: u_j changed or the form changed under everything enqueued after it,
  // which the caller enqueues again from j + 1.
  struct Scalars {
    double alpha, beta2, c0, c1;
    bool redone;
  };
  Scalars collect(int64_t j) {
    const int slot = (int)(j % kRingSlots);
    const double tw0 = now_s();
    LL_HIP(hipEventSynchronize(ring.ev[ev_of_slot[slot]]));
    t_wait += now_s() - tw0;
    const volatile double* hp = pinned_slot(slot);
    Scalars r{hp[0], hp[1], hp[2], hp[3], false};
    // the guard of the blocks of eight: how many block iterations in a row, up to this one, published a quiet gate value
    blk_quiet = block_enabled && slot_pair[slot] && *pinned_gate(slot) <= kBlock8Tau ? std::min(blk_quiet + 1, (int)kBlock8Quiet) : 0;
    double* const beta2_dev = E.S(kScalNorms + 3 * slot) + 1;  // what the next three-term update reads as beta_j^2
    if (dgks && r.c1 < E.ctx->tune.dgks_threshold * r.c0) {
      // DGKS "twice is enough", decided here from the published norms: the first pass removed more than half of
      // ||w||^2, so Gram-Schmidt is repeated on u_j (already scaled to unit norm on the device) and beta_j shrinks
      // by the norm that survives.  Rare (near breakdown / deflation); costs one pipeline drain.
      if (r.c1 > 0.0 && std::isfinite(r.c1)) {
        const RunList<T> again = basis_runs(j);
        make_final(j);
        r.beta2 = r.c1 * E.second_pass(U.vec(j), again);
        ++n_second_passes;
        launch_set_scalar(beta2_dev, r.beta2, s);
        if (lag_ok) launch_set_scalar(lb.hist_beta + j - 1, std::sqrt(r.beta2), s);  // the device copy of T
        restart_after(j);
        r.redone = true;
      } else {
        r.beta2 = 0.0;  // w vanished exactly: breakdown (H3)
      }
    }
    if (!r.redone && lag_ok && n_locked > 0 && r.beta2 < lag_beta2_min) {
      // beta_j too small for the first-order treatment of the locked columns (begin_pass): u_j is completed with the two-sweep
      // kernels (unless the speculative sweep already has) and the pass continues in the two-sweep form
      make_final(j);
      lag_ok = false;
      restart_after(j);
      r.redone = true;
    }
    if (!r.redone && slot_pair[slot] && !(*pinned_gate(slot) <= kGate)) {
      // A coefficient of this iteration's raw vector grew beyond what the pair form tracks to first order (beta -> eps: an
      // exhausted Krylov space, breakdown).  The iteration itself stands — its coefficients were MEASURED, its alpha / beta
      // are exact — but whatever took the vector as an operator input (the second iteration of its pair, the next pair) is
      // second-order inaccurate: u_j is completed with its measured coefficients, everything after it is enqueued again, and
      // the rest of the pass runs in the one-sweep form (exact for coefficients of any size).
      pair_allowed = false;
      block_allowed = false;
      ++n_gate_trips;
      make_final(j);
      launch_set_scalar(beta2_dev, r.beta2, s);
      restart_after(j);
      r.redone = true;
    }
    return r;
  }
};

// Callback operators run WITHOUT speculation: the user's mv_mul must be called exactly as often as the reference calls it (LL:243:
// once per executed iteration) and never on the 1/sqrt(~0)-scaled vector that follows a breakdown; a host callback synchronises the
// stream anyway, so there is nothing to overlap.
inline bool speculates(const ll_operator* op) { return !(op->kind == ll_operator::HOST_CB || op->kind == ll_operator::DEV_CB); }
// Part 2 of the host half (Ritz values, breakdown, convergence; the Exponentiator's exp(a T_j) e_1) runs on a helper thread, in
// iteration order, wherever the loop speculates; LL_TRIDIAG_THREAD=0 computes the verdicts inline (lag 1, the round-1 behaviour).
inline bool threaded_verdicts(const ll_context* ctx, const ll_operator* op) { return speculates(op) && ctx->tune.tridiag_thread; }

// One Lanczos pass of iterations 1 .. max_iteration on the host side, shared by the eigen-solver and the Exponentiator: enqueue,
// collect the scalars (alpha and beta land in alpha / beta, then on_collect(j, scalars) runs), hand T_j to the worker's tracker and
// absorb its verdicts into `last`.  Returns whether a stop verdict ended the pass.
template <typename T, typename Tracker, typename OnCollect>
bool run_pass(LoopState<T>& LS, StepWorker<Tracker>& worker, int64_t max_iteration, double offset, int mode, bool full,
              std::vector<double>& alpha, std::vector<double>& beta, typename Tracker::Out& last, double& t_tridiag,
              OnCollect&& on_collect) {
  const ll_context* ctx = LS.E.ctx;
  // This thread keeps enqueuing and looks at the verdicts as they arrive, at most kMaxLag iterations late.  A verdict that arrives
  // late only means a few speculative iterations more on the device (they write basis slots the results never read).  The lag is
  // only ever used when the helper is slower than the device — in practice the O(m^2) QR confirmations of LL_TRIDIAG_AUTO near
  // convergence at large m (190 ms at m = 3300 against 9 ms per device iteration at n = 1e6) — so the bound is generous; while the
  // helper keeps up the verdicts are one iteration late.
  const size_t kMaxLag = worker.threaded() ? 24 : 0;
  const int64_t lockstep_lag = worker.threaded() && ctx->comm != nullptr ? std::max(-1, ctx->tune.tridiag_lag) : -1;  // see StepWorker::consume
  bool stopped = false;
  auto absorb = [&](typename Tracker::Out& o) {
    t_tridiag += o.seconds;
    last = std::move(o);
    return last.stop;
  };
  auto collect = [&](int64_t j) {
    const typename LoopState<T>::Scalars sc = LS.collect(j);
    alpha.push_back(sc.alpha);
    beta.push_back(std::sqrt(sc.beta2));
    on_collect(j, sc);
    worker.submit((int64_t)alpha.size(), alpha.data(), beta.data());
    return sc.redone;
  };
  typename Tracker::Out r;
  if (speculates(LS.E.op)) {
    // One group of iterations (one, or the two of a pair) is enqueued ahead of the group whose scalars are collected.
    int64_t enq = 0, col = 0;  // iterations enqueued / collected so far
    int64_t ahead_first = 1, ahead_last = 0;  // the group enqueued last, not yet collected (empty: first > last)
    while (!stopped && col < max_iteration) {
      const int64_t grp_first = ahead_first, grp_last = ahead_last;
      if (enq < max_iteration) {
        ahead_first = enq + 1;
        enq += LS.enqueue_group(enq + 1, offset, mode, full);
        ahead_last = enq;
      } else {
        LS.flush();  // nothing follows: the last iteration's normalisation / publish step happens now
        ahead_first = 1;
        ahead_last = 0;
      }
      for (int64_t j = grp_first; j <= std::min(grp_last, max_iteration) && !stopped; ++j) {
        const bool redo = collect(j);
        col = j;
        if (redo) {  // u_j changed under everything enqueued after it: enqueue again from j + 1
          enq = j;
          ahead_first = 1;
          ahead_last = 0;
        }
        stopped = worker.consume(j, lockstep_lag, kMaxLag, absorb);
        if (redo) break;
      }
    }
  } else {
    for (int64_t k = 1; k <= max_iteration && !stopped; ++k) {
      // (one iteration at a time: callback operators never take the one-sweep forms, so enqueue_group never enqueues a pair)
      LS.enqueue_group(k, offset, mode, full);
      collect(k);  // redone: u_k was repaired in place, nothing ran ahead
      while (!stopped && worker.wait_pop(r)) stopped = absorb(r);
    }
  }
  while (!stopped && worker.wait_pop(r)) stopped = absorb(r);  // the first stop verdict wins; else the last iteration's values
  return stopped;
}

// The argument checks of the whole-loop runs, and their float tolerance: ll_*_params_default() fills in the DOUBLE one
// (eps_factor * DBL_EPSILON: LL:150, EX:58 with real_t<T> = double); the reference scales it with the epsilon of real_t<T>, so a
// float run left at that default gets eps_factor * FLT_EPSILON instead of a tolerance float data can never meet (which would run
// to max_iteration = n).
template <typename T, typename Params> void check_run(ll_context* ctx, ll_operator* op, Params& P, double eps_factor) {
  if (sizeof(typename scalar_traits<T>::real) == 4 && P.eps == std::numeric_limits<double>::epsilon() * eps_factor)
    P.eps = (double)std::numeric_limits<float>::epsilon() * eps_factor;
  LL_REQUIRE(op && op->ctx == ctx, "operator belongs to another context");
  LL_REQUIRE(op->is_complex == scalar_traits<T>::is_complex && op->elem_bytes == (int)sizeof(T),
             "operator scalar type mismatch");
  LL_REQUIRE(P.matrix_size == op->n, "matrix_size differs from the operator dimension");
  LL_REQUIRE(P.max_iteration >= 1, "max_iteration must be >= 1");
}

// The default start vector (LL:70-104): std::random_device-seeded mt19937, uniform [-1,1]; complex: real part, then imaginary part
template <typename T> void random_start(T* v, int64_t n) {
  typedef typename scalar_traits<T>::real Real;
  std::random_device dev;
  std::mt19937 mt(dev());
  std::uniform_real_distribution<Real> r((Real)-1, (Real)1);
  Real* f = reinterpret_cast<Real*>(v);
  for (int64_t i = 0; i < n * scalar_traits<T>::reals; ++i) f[i] = r(mt);
}

// The ll_run_stats fields both runs fill (n_passes, seconds_setup and seconds_finish are the eigen-solver's own).
template <typename T>
void fill_stats(ll_run_stats* stats, LoopState<T>& loop, int64_t total_iterations, size_t last_alpha_len, double t_tridiag,
                double t_start) {
  ll_context* ctx = loop.E.ctx;
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->total_iterations = total_iterations;
    stats->seconds_host_tridiag = t_tridiag;
    stats->last_alpha_len = (int64_t)last_alpha_len;
    stats->seconds_host_enqueue = loop.t_enqueue;
    stats->seconds_host_wait = loop.t_wait;
    stats->second_passes = loop.n_second_passes;
    stats->lagged_iterations = loop.n_lagged;
    stats->pair_iterations = loop.n_pair;
    stats->pair_gate_trips = loop.n_gate_trips;
    stats->reserved[0] = loop.n_block;          // block_iterations
    stats->reserved[1] = loop.n_block_flushed;  // block_flushed_vectors
    stats->reserved[2] = loop.n_block8;         // block8_iterations
    loop.timer.collect(stats->seconds_spmv, stats->seconds_orth);
    ctx->drain_comm_events(&stats->seconds_comm_gather, &stats->seconds_comm_allreduce);
    stats->seconds_total = now_s() - t_start;
  }
  ctx->drain_comm_events(nullptr, nullptr);
}

}  // namespace ll
