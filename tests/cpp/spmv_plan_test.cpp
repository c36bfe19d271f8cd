// The host-side planning of the propagation-blocked and the 2-D tiled SpMV images (lambda-lanczos_amd/csrc/spmv_plan.hpp) against
// properties that follow from what the kernels READ: every property is checked by brute force over every column, every segment slot
// or every tile of small shapes, with no second implementation of the planner's arithmetic to agree with.  Built (plain, and with
// the address and undefined-behaviour sanitizers) and run by tests/test_spmv_plan_host.py.
#include <cstdio>
#include <random>
#include <set>

#include "spmv_plan.hpp"

using namespace ll;

static std::mt19937_64 rng(20261019);
static long long checks = 0, fails = 0;
#define REQUIRE(cond, ...)                          \
  do {                                              \
    ++checks;                                       \
    if (!(cond) && fails++ < 20) {                  \
      std::printf("FAIL line %d: ", __LINE__);      \
      std::printf(__VA_ARGS__);                     \
      std::printf("\n");                            \
    }                                               \
  } while (0)

// ================================================================= PB: the column plan
// What phase 1 reads: workgroup idx stages ncols[idx] elements from its source buffer at xoff[idx] — the rank's own shard for the
// table range [0, own_total), the gathered buffer (region c at P * start[c], rank s's piece at + s * len[c]) for the ranges
// [chunk_first[c], + chunk_count[c]) — and the build kernels send global column j to (pb_block_of, local).
static void test_column_plan(int64_t n, int P, int rank, int gather_chunks, int pb_block, int pb_col_block, int64_t col_cap,
                             size_t elem_bytes, size_t acc_bytes) {
  const int64_t S = (n + P - 1) / P;
  PlanShape sh;
  sh.n = n;
  sh.nranks = P;
  sh.rank = rank;
  sh.shard = P > 1 ? S : n;
  sh.row_begin = std::max(rank, 0) * S;
  sh.n_local = std::max<int64_t>(0, std::min<int64_t>(S, n - sh.row_begin));
  sh.elem_bytes = elem_bytes;
  sh.acc_bytes = acc_bytes;
  PlanTuning tune;
  tune.gather_chunks = gather_chunks;
  tune.pb_block = pb_block;
  tune.pb_col_block = pb_col_block;
  PlanLimits lim;
  lim.col_cap = col_cap;
  PbGeometry g;
  const bool ok = pb_plan_geometry(sh, tune, lim, &g);
#define CASE "n=%lld P=%d rank=%d chunks=%d block=%d colblock=%d cap=%lld elem=%d"
#define CASE_ARGS (long long)n, P, rank, gather_chunks, pb_block, pb_col_block, (long long)col_cap, (int)elem_bytes
  REQUIRE(ok, CASE ": no plan", CASE_ARGS);
  if (!ok) return;
  const PbColMap& m = g.map;
  const GatherPlan& gp = g.gather;
  const int64_t ncb = g.ncb;
  REQUIRE((int64_t)g.xoff.size() == ncb && (int64_t)g.ncols.size() == ncb, CASE ": table sizes", CASE_ARGS);
  REQUIRE(g.nrb >= 1 && g.rb_rows >= 1 && g.rb_rows * g.nrb >= sh.n_local, CASE ": row blocks", CASE_ARGS);
  // ---- the gather plan: chunks tile [0, S), starts on multiples of 256
  REQUIRE(gp.nchunks >= 1 && gp.nchunks <= kMaxGatherChunks && (P > 1 || gp.nchunks == 1), CASE ": nchunks %d", CASE_ARGS, gp.nchunks);
  int64_t covered = 0;
  for (int c = 0; c < gp.nchunks; ++c) {
    REQUIRE(gp.start[c] == covered && gp.start[c] % 256 == 0 && gp.len[c] > 0, CASE ": chunk %d start %lld len %lld", CASE_ARGS, c,
            (long long)gp.start[c], (long long)gp.len[c]);
    covered += gp.len[c];
  }
  REQUIRE(covered == sh.shard, CASE ": chunks cover %lld of %lld", CASE_ARGS, (long long)covered, (long long)sh.shard);
  // ---- the launch ranges: own blocks [0, own_total), then chunk by chunk up to ncb
  REQUIRE(g.own_total >= 0 && g.own_total <= ncb && (rank >= 0 || g.own_total == 0), CASE ": own_total", CASE_ARGS);
  int64_t next = g.own_total;
  for (int c = 0; c < gp.nchunks; ++c) {
    REQUIRE(g.chunk_first[c] == next && g.chunk_count[c] >= 0, CASE ": chunk range %d", CASE_ARGS, c);
    next += g.chunk_count[c];
  }
  REQUIRE(next == ncb, CASE ": ranges end at %lld, ncb %lld", CASE_ARGS, (long long)next, (long long)ncb);
  // ---- every table index is produced exactly once by the blocks (chunk, shard, block in chunk)
  std::vector<int> produced((size_t)ncb, 0);
  int64_t nblocks = 0;
  for (int c = 0; c < gp.nchunks; ++c)
    for (int s = 0; s < P; ++s)
      for (int64_t first = gp.start[c]; first < gp.start[c] + gp.len[c]; first += m.bl[c], ++nblocks) {
        int local = -1;
        const int idx = pb_block_of(m, (long long)s * sh.shard + first, &local);
        REQUIRE(idx >= 0 && idx < ncb && local == 0, CASE ": block at %lld of shard %d -> %d, local %d", CASE_ARGS, (long long)first, s, idx, local);
        if (idx >= 0 && idx < ncb) ++produced[(size_t)idx];
      }
  REQUIRE(nblocks == ncb, CASE ": %lld blocks, ncb %lld", CASE_ARGS, (long long)nblocks, (long long)ncb);
  for (int64_t i = 0; i < ncb; ++i) REQUIRE(produced[(size_t)i] == 1, CASE ": index %lld produced %d times", CASE_ARGS, (long long)i, produced[(size_t)i]);
  // ---- every global column
  int64_t sum_cols = 0;
  for (int64_t i = 0; i < ncb; ++i) {
    sum_cols += g.ncols[(size_t)i];
    REQUIRE(g.ncols[(size_t)i] >= 0 && g.ncols[(size_t)i] <= g.cb_cols, CASE ": ncols[%lld] = %d, cb_cols %d", CASE_ARGS, (long long)i,
            g.ncols[(size_t)i], g.cb_cols);
  }
  REQUIRE(sum_cols == n, CASE ": sum of ncols %lld", CASE_ARGS, (long long)sum_cols);
  REQUIRE((int64_t)g.cb_cols <= col_cap && (int64_t)g.cb_cols * (int64_t)elem_bytes + (2 * g.nrb + 1) * 8 + 16 <= lim.lds_cap,
          CASE ": cb_cols %d", CASE_ARGS, g.cb_cols);
  std::vector<int64_t> seen((size_t)ncb, 0), blk_shard((size_t)ncb, -1), blk_chunk((size_t)ncb, -1), blk_first((size_t)ncb, -1);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t s = j / sh.shard, l = j - s * sh.shard;  // shard and offset inside it
    int c = 0;
    while (c + 1 < gp.nchunks && gp.start[c + 1] <= l) ++c;  // the gather chunk that ships offset l
    int local = -1;
    const int idx = pb_block_of(m, j, &local);
    REQUIRE(idx >= 0 && idx < ncb, CASE ": column %lld -> block %d", CASE_ARGS, (long long)j, idx);
    if (idx < 0 || idx >= ncb) continue;
    REQUIRE(local >= 0 && local < g.ncols[(size_t)idx], CASE ": column %lld -> local %d of %d", CASE_ARGS, (long long)j, local, g.ncols[(size_t)idx]);
    const bool own = (int)s == rank;
    const int64_t pos = own ? l : (int64_t)P * gp.start[c] + s * gp.len[c] + (l - gp.start[c]);
    REQUIRE(g.xoff[(size_t)idx] + local == pos, CASE ": column %lld read at %lld, lies at %lld", CASE_ARGS, (long long)j,
            (long long)(g.xoff[(size_t)idx] + local), (long long)pos);
    REQUIRE(own == (idx < g.own_total), CASE ": column %lld own %d, block %d, own_total %d", CASE_ARGS, (long long)j, (int)own, idx, g.own_total);
    if (!own) REQUIRE(idx >= g.chunk_first[c] && idx < g.chunk_first[c] + g.chunk_count[c], CASE ": column %lld of chunk %d in block %d", CASE_ARGS,
                      (long long)j, c, idx);
    // no block straddles a chunk or a shard, and its columns are consecutive
    if (seen[(size_t)idx]++ == 0) {
      blk_shard[(size_t)idx] = s;
      blk_chunk[(size_t)idx] = c;
      blk_first[(size_t)idx] = j - local;
    }
    REQUIRE(blk_shard[(size_t)idx] == s && blk_chunk[(size_t)idx] == c && blk_first[(size_t)idx] == j - local,
            CASE ": block %d straddles at column %lld", CASE_ARGS, idx, (long long)j);
  }
  for (int64_t i = 0; i < ncb; ++i) REQUIRE(seen[(size_t)i] == g.ncols[(size_t)i], CASE ": block %lld holds %lld columns, ncols %d", CASE_ARGS,
                                            (long long)i, (long long)seen[(size_t)i], g.ncols[(size_t)i]);
#undef CASE
#undef CASE_ARGS
}

static void test_column_plans() {
  struct Override {
    int pb_block, pb_col_block;
  };
  for (const int64_t n : {1, 2, 5, 17, 255, 256, 257, 600, 1031, 2049})
    for (const int P : {1, 2, 3, 8})
      for (const int rank : std::set<int>{0, P - 1, -1})
        for (const int chunks : {0, 1, 3, 8})
          for (const Override o : {Override{0, 0}, Override{4, 0}, Override{5, 0}, Override{0, 7}})
            for (const int64_t cap : {65536, 13000, 48}) {
              test_column_plan(n, P, rank, chunks, o.pb_block, o.pb_col_block, cap, 8, 8);
              test_column_plan(n, P, rank, chunks, o.pb_block, o.pb_col_block, cap, 16, 16);
            }
}

// ================================================================= PB: shapes the planner turns down
static bool pb_plans(int64_t n, int64_t n_local, int row_block, int col_block) {
  PlanShape sh;
  sh.n = sh.shard = n;
  sh.n_local = n_local;
  PlanTuning tune;
  tune.pb_row_block = row_block;
  tune.pb_col_block = col_block;
  PbGeometry g;
  return pb_plan_geometry(sh, tune, PlanLimits(), &g);
}
static void test_rejections() {
  // phase 1 keeps 2 nrb + 1 table entries of 8 bytes next to its x slice: (2 nrb + 1) * 8 + 16 + 1024 bytes must fit kPbLdsCap
  const int64_t nrb_max = ((kPbLdsCap - 1024 - 16) / 8 - 1) / 2;
  REQUIRE(pb_plans(4 * nrb_max, 4 * nrb_max, 4, 0), "nrb = %lld must fit", (long long)nrb_max);
  REQUIRE(!pb_plans(4 * (nrb_max + 1), 4 * (nrb_max + 1), 4, 0), "nrb = %lld cannot fit", (long long)nrb_max + 1);
  // ncb * nrb beyond 24 Mi segments: 5000 row blocks x 5033 / 5034 column blocks
  REQUIRE(5000ll * 5033 <= (24ll << 20) && 5000ll * 5034 > (24ll << 20), "the pair brackets the limit");
  REQUIRE(pb_plans(4 * 5033, 4 * 5000, 4, 4), "5000 x 5033 segments are allowed");
  REQUIRE(!pb_plans(4 * 5034, 4 * 5000, 4, 4), "5000 x 5034 segments are too many");
  // the LDS histogram of the build kernels: ncb * 4 bytes within 60 KiB
  REQUIRE(pb_plans(4 * 15360, 16, 0, 4), "15360 column blocks: a 60 KiB histogram");
  REQUIRE(!pb_plans(4 * 15361, 16, 0, 4), "15361 column blocks: beyond 60 KiB");
  // the tiled image has the same two limits (tiles of 2048 doubles)
  auto tl_plans = [](int64_t n, int64_t n_local, int row_block) {
    PlanShape sh;
    sh.n = sh.shard = n;
    sh.n_local = n_local;
    PlanTuning tune;
    tune.pb_row_block = row_block;
    TlGeometry g;
    return tl_plan_geometry(sh, tune, PlanLimits(), &g);
  };
  REQUIRE(tl_plans(2048ll * 15360, 16, 0) && !tl_plans(2048ll * 15360 + 1, 16, 0), "tiled: histogram limit");
  REQUIRE(tl_plans(2048ll * 5033, 4 * 5000, 4) && !tl_plans(2048ll * 5034, 4 * 5000, 4), "tiled: count table limit");
}

// ================================================================= PB: the two segment orders
static std::vector<int32_t> random_counts(int ncb, int nrb) {
  std::vector<int32_t> cnt((size_t)ncb * nrb);
  for (auto& k : cnt) {
    const unsigned u = (unsigned)(rng() % 8);
    k = u < 3 ? 0 : (u < 6 ? (int32_t)(rng() % 20) : (int32_t)(rng() % 300));  // zeros, sizes around the pads, long segments
  }
  return cnt;
}
// What the kernels read: phase 1 streams the slots [segq[c][0], segq[c][nrb]) of column block c and writes segment (c, r) to
// segdest[c][r] + (slot - segq[c][r]); phase 2 streams [rptr[r], rptr[r + 1]).
static void test_segments(int ncb, int nrb, int64_t pad) {
  const std::vector<int32_t> cnt = random_counts(ncb, nrb);
  const PbSegments sg = pb_plan_segments(cnt, ncb, nrb, pad);
  REQUIRE((int64_t)sg.segq.size() == (int64_t)ncb * (nrb + 1) && (int64_t)sg.segdest.size() == (int64_t)ncb * nrb &&
              (int64_t)sg.rptr.size() == nrb + 1,
          "%d x %d pad %lld: table sizes", ncb, nrb, (long long)pad);
  auto padded = [&](int c, int r) { return ((int64_t)cnt[(size_t)c * nrb + r] + pad - 1) / pad * pad; };
  int64_t total = 0;
  for (int c = 0; c < ncb; ++c)
    for (int r = 0; r < nrb; ++r) total += padded(c, r);
  REQUIRE(sg.entries == total, "%d x %d pad %lld: entries %lld, padded sum %lld", ncb, nrb, (long long)pad, (long long)sg.entries, (long long)total);
  if (sg.entries != total) return;
  // slot by slot: who owns it in either order (-1: nobody yet)
  std::vector<int> owner_q((size_t)total, -1), owner_d((size_t)total, -1);
  for (int c = 0; c < ncb; ++c)
    for (int r = 0; r < nrb; ++r) {
      const int64_t q = sg.segq[(size_t)c * (nrb + 1) + r], d = sg.segdest[(size_t)c * nrb + r];
      REQUIRE(q >= 0 && q + padded(c, r) <= total && d >= 0 && d + padded(c, r) <= total, "%d x %d pad %lld: segment (%d, %d) out of range", ncb, nrb,
              (long long)pad, c, r);
      if (!(q >= 0 && q + padded(c, r) <= total && d >= 0 && d + padded(c, r) <= total)) return;
      for (int64_t i = 0; i < padded(c, r); ++i) {
        REQUIRE(owner_q[(size_t)(q + i)] == -1 && owner_d[(size_t)(d + i)] == -1, "%d x %d pad %lld: segment (%d, %d) overlaps", ncb, nrb,
                (long long)pad, c, r);
        owner_q[(size_t)(q + i)] = c * nrb + r;   // c-major rank of the segment
        owner_d[(size_t)(d + i)] = r * ncb + c;   // r-major rank of the segment
      }
    }
  // every slot is taken (disjoint + the sizes add up to the total) and the owners' ranks never decrease: contiguous, in order
  for (int64_t i = 0; i < total; ++i) {
    REQUIRE(owner_q[(size_t)i] >= 0 && owner_d[(size_t)i] >= 0, "%d x %d pad %lld: slot %lld is nobody's", ncb, nrb, (long long)pad, (long long)i);
    if (i > 0)
      REQUIRE(owner_q[(size_t)i] >= owner_q[(size_t)i - 1] && owner_d[(size_t)i] >= owner_d[(size_t)i - 1], "%d x %d pad %lld: order breaks at slot %lld",
              ncb, nrb, (long long)pad, (long long)i);
  }
  for (int c = 0; c < ncb; ++c) {  // the sentinel of column block c is where the next one starts; the last is the end of the image
    const int64_t end = c + 1 < ncb ? sg.segq[(size_t)(c + 1) * (nrb + 1)] : total;
    REQUIRE(sg.segq[(size_t)c * (nrb + 1) + nrb] == end, "%d x %d pad %lld: sentinel of column block %d", ncb, nrb, (long long)pad, c);
  }
  for (int r = 0; r < nrb; ++r) REQUIRE(sg.rptr[(size_t)r] == sg.segdest[(size_t)r], "%d x %d pad %lld: rptr[%d]", ncb, nrb, (long long)pad, r);
  REQUIRE(sg.rptr[(size_t)nrb] == total, "%d x %d pad %lld: rptr[nrb]", ncb, nrb, (long long)pad);
}

// ================================================================= PB: the arena of the four streams
static void test_arena() {
  const size_t two_mib = (size_t)2 << 20;
  for (const size_t cap : {(size_t)16, (size_t)17, ((size_t)1 << 20) + 3})
    for (const size_t elem : {(size_t)4, (size_t)8, (size_t)16}) {
      const PbArena a = pb_plan_arena(cap, elem);
      REQUIRE(a.o_val == 0 && a.o_col % two_mib == 0 && a.o_row % two_mib == 0 && a.o_prod % two_mib == 0, "cap %zu elem %zu: alignment", cap, elem);
      REQUIRE(a.o_val + cap * elem <= a.o_col && a.o_col + cap * 2 <= a.o_row && a.o_row + cap * 2 <= a.o_prod && a.o_prod + cap * elem == a.total,
              "cap %zu elem %zu: streams overlap", cap, elem);
      REQUIRE(a.o_val < a.o_col && a.o_col < a.o_row && a.o_row < a.o_prod && a.o_prod < a.total, "cap %zu elem %zu: order", cap, elem);
    }
}

// ================================================================= tiled: row blocks and the column map
static void test_tiled_geometry() {
  struct Sizes {
    size_t elem, acc;
  };
  for (const Sizes sz : {Sizes{8, 8}, Sizes{16, 16}, Sizes{4, 8}, Sizes{8, 16}})  // double, complex double, float, complex float
    for (const int64_t n : {1, 17, 2049, 70000, 3000000})
      for (const int row_block : {0, 5, 40}) {
        if (row_block > 0 && n > 70000) continue;  // (beyond the count-table limit: test_rejections)
        const size_t elem = sz.elem, acc = sz.acc;
        PlanShape sh;
        sh.n = sh.shard = sh.n_local = n;
        sh.elem_bytes = elem;
        sh.acc_bytes = acc;
        PlanTuning tune;
        tune.pb_row_block = row_block;
        {
          TlGeometry g;
          const bool ok = tl_plan_geometry(sh, tune, PlanLimits(), &g);
          REQUIRE(ok, "tiled n=%lld elem=%zu: no plan", (long long)n, elem);
          if (!ok) continue;
          const int C = kTlTileBytes / (int)elem;
          REQUIRE(g.tile_cols == C && g.ncb == (n + C - 1) / C, "tiled n=%lld elem=%zu: tiles", (long long)n, elem);
          REQUIRE(g.rb_rows % 2 == 0 && g.rb_rows >= 4 && g.nrb * g.rb_rows >= n && (g.nrb - 1) * g.rb_rows < n, "tiled n=%lld elem=%zu: rb_rows %lld",
                  (long long)n, elem, (long long)g.rb_rows);
          // the y slice, the x ring and the bad-row bits fit the LDS
          REQUIRE(g.rb_rows * (int64_t)acc + kTlSlots * kTlTileBytes + (g.rb_rows + 31) / 32 * 4 + 16 <= kPbLdsCap, "tiled n=%lld elem=%zu acc=%zu: LDS",
                  (long long)n, elem, acc);
          if (row_block > 0) REQUIRE(g.rb_rows == row_block + (row_block & 1), "tiled: forced row block %d -> %lld", row_block, (long long)g.rb_rows);
          for (const int64_t j : std::set<int64_t>{0, n / 2, n - 1, std::min<int64_t>(n - 1, C - 1), std::min<int64_t>(n - 1, C)}) {
            int local = -1;
            const int idx = pb_block_of(g.map, j, &local);
            REQUIRE(idx == j / C && local == j % C, "tiled n=%lld elem=%zu: column %lld -> (%d, %d)", (long long)n, elem, (long long)j, idx, local);
          }
        }
      }
}

// ================================================================= tiled: the tile list
// What the kernel reads: row block r walks the tiles [tfirst[r], tfirst[r + 1]) of tcol / tquad; the scatter kernel puts the entries
// of tile (c, r) at segq[c][r]; a sharded launch takes the row blocks rbmap[0, n_interior) with the rank's own shard for x.
static void test_tiles(int ncb, int nrb, bool walk_modulo, int P, int rank, bool all_empty) {
  std::vector<int32_t> cnt = random_counts(ncb, nrb);
  if (all_empty) std::fill(cnt.begin(), cnt.end(), 0);
  const int C = 8;
  TlGeometry g;
  g.nrb = nrb;
  g.ncb = ncb;
  g.tile_cols = C;
  g.rb_rows = 4;
  PlanShape sh;
  sh.n = (int64_t)ncb * C - 3;
  sh.nranks = P;
  sh.rank = rank;
  const int64_t S = (sh.n + P - 1) / P;
  sh.shard = P > 1 ? S : sh.n;
  sh.row_begin = rank * S;
  sh.n_local = std::max<int64_t>(0, std::min<int64_t>(S, sh.n - sh.row_begin));
  int64_t nnz = 0;
  for (const int32_t k : cnt) nnz += k;
  const TlTiles t = tl_plan_tiles(cnt, g, sh, nnz, walk_modulo);
#define CASE "tiles %d x %d walk %d P=%d rank=%d"
#define CASE_ARGS ncb, nrb, (int)walk_modulo, P, rank
  // ---- the walk is a permutation of the column tiles; ascending: the identity
  std::vector<int> hit((size_t)ncb, 0);
  REQUIRE((int)t.order.size() == ncb, CASE ": order holds %zu tiles", CASE_ARGS, t.order.size());
  for (const int32_t c : t.order) {
    REQUIRE(c >= 0 && c < ncb, CASE ": order holds %d", CASE_ARGS, c);
    if (c >= 0 && c < ncb) ++hit[(size_t)c];
  }
  for (int c = 0; c < ncb; ++c) REQUIRE(hit[(size_t)c] == 1, CASE ": tile %d is walked %d times", CASE_ARGS, c, hit[(size_t)c]);
  if (!walk_modulo)
    for (int i = 0; i < (int)t.order.size(); ++i) REQUIRE(t.order[(size_t)i] == i, CASE ": ascending walk, step %d", CASE_ARGS, i);
  // ---- a row block's tiles: its non-empty column tiles, each once, in the order of the walk
  REQUIRE((int)t.tfirst.size() == nrb + 1 && (int64_t)t.tcol.size() == t.ntiles + 1 && (int64_t)t.tquad.size() == t.ntiles + 1 &&
              (int64_t)t.segq.size() == (int64_t)ncb * (nrb + 1),
          CASE ": table sizes", CASE_ARGS);
  REQUIRE(t.tfirst[0] == 0 && t.tfirst[(size_t)nrb] == t.ntiles, CASE ": tfirst ends", CASE_ARGS);
  int64_t q = 0, tile = 0;
  for (int r = 0; r < nrb; ++r) {
    REQUIRE(t.tfirst[(size_t)r] == tile, CASE ": tfirst[%d]", CASE_ARGS, r);
    for (const int32_t c : t.order) {
      const int64_t k = cnt[(size_t)c * nrb + r];
      if (k == 0) continue;
      REQUIRE(tile < t.ntiles && t.tcol[(size_t)tile] == c, CASE ": tile %lld of row block %d is not column tile %d", CASE_ARGS, (long long)tile, r, c);
      if (tile >= t.ntiles) return;
      // the tile's stream: 4-entry aligned, behind the tile before it, long enough for its entries, where the scatter kernel writes
      REQUIRE(t.tquad[(size_t)tile] * 4 == q && q % 4 == 0 && t.segq[(size_t)c * (nrb + 1) + r] == q, CASE ": tile %lld starts at quad %lld, entry %lld",
              CASE_ARGS, (long long)tile, (long long)t.tquad[(size_t)tile], (long long)q);
      REQUIRE(t.tquad[(size_t)tile + 1] >= t.tquad[(size_t)tile] && (t.tquad[(size_t)tile + 1] - t.tquad[(size_t)tile]) * 4 >= k,
              CASE ": tile %lld holds %lld entries", CASE_ARGS, (long long)tile, (long long)k);
      q = t.tquad[(size_t)tile + 1] * 4;
      ++tile;
    }
  }
  REQUIRE(tile == t.ntiles, CASE ": %lld tiles, list %lld", CASE_ARGS, (long long)tile, (long long)t.ntiles);
  REQUIRE(t.entries % 4 == 0 && t.tquad.back() == t.entries / 4 && t.entries == q, CASE ": entries %lld", CASE_ARGS, (long long)t.entries);
  REQUIRE(!t.tcol.empty(), CASE ": no padding entry", CASE_ARGS);  // (what a row block without tiles reads)
  // ---- the launch order of a sharded context
  if (P == 1) {
    REQUIRE(t.rbmap.empty() && t.n_interior == 0, CASE ": a map on one GPU", CASE_ARGS);
  } else {
    std::vector<int> used((size_t)nrb, 0);
    REQUIRE((int)t.rbmap.size() == nrb && t.n_interior >= 0 && t.n_interior <= nrb, CASE ": map size", CASE_ARGS);
    for (int i = 0; i < (int)t.rbmap.size(); ++i) {
      const int r = t.rbmap[(size_t)i];
      REQUIRE(r >= 0 && r < nrb, CASE ": map holds %d", CASE_ARGS, r);
      if (r < 0 || r >= nrb) continue;
      ++used[(size_t)r];
      bool foreign = false;  // does the row block read a column that is not the rank's own?
      for (int c = 0; c < ncb; ++c)
        if (cnt[(size_t)c * nrb + r] != 0)
          for (int64_t j = (int64_t)c * C; j < std::min<int64_t>((int64_t)(c + 1) * C, sh.n); ++j)
            if (j < sh.row_begin || j >= sh.row_begin + sh.n_local) foreign = true;
      REQUIRE(foreign == (i >= t.n_interior), CASE ": row block %d at place %d, n_interior %d, foreign %d", CASE_ARGS, r, i, t.n_interior, (int)foreign);
    }
    for (int r = 0; r < nrb; ++r) REQUIRE(used[(size_t)r] == 1, CASE ": row block %d launched %d times", CASE_ARGS, r, used[(size_t)r]);
  }
#undef CASE
#undef CASE_ARGS
}

// the verdict: the re-staged x tiles (16 KiB each) cost no more than the stream (sizeof(T) + 4 bytes per padded entry), and the padding
// stays within a quarter of the entries + one pad per row block
static void test_eligibility() {
  TlGeometry g;
  g.nrb = 1;
  g.ncb = 1;
  g.tile_cols = 2048;
  PlanShape sh;
  sh.n = sh.shard = sh.n_local = 2048;
  auto verdict = [&](int32_t k, int64_t nnz) { return tl_plan_tiles(std::vector<int32_t>{k}, g, sh, nnz, true).eligible; };
  REQUIRE(verdict(1376, 1376), "1376 entries of 12 bytes outweigh one tile");  // 1376 * 12 = 16512 >= 16384
  REQUIRE(!verdict(1360, 1360), "1360 entries of 12 bytes do not");            // 1360 * 12 = 16320
  REQUIRE(!verdict(2000, 1500), "2000 slots for 1500 entries: too much padding");  // 2000 > 1.25 * 1500 + 16
}

int main() {
  test_column_plans();
  test_rejections();
  for (int rep = 0; rep < 40; ++rep)
    for (const int64_t pad : {4, 16}) test_segments(1 + (int)(rng() % 9), 1 + (int)(rng() % 9), pad);
  for (const int64_t pad : {4, 16}) test_segments(9, 9, pad), test_segments(1, 1, pad);
  test_arena();
  test_tiled_geometry();
  for (int rep = 0; rep < 40; ++rep)
    for (const bool walk : {false, true}) {
      const int ncb = 1 + (int)(rng() % 9), nrb = 1 + (int)(rng() % 9);
      test_tiles(ncb, nrb, walk, 1, 0, rep == 0);
      for (int rank = 0; rank < 3; ++rank) test_tiles(ncb, nrb, walk, 3, rank, rep == 0);
    }
  test_eligibility();
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
