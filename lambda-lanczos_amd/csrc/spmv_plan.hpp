// Host-side planning of the two SpMV images that are built on the device (spmv_image_build.hip): block geometry, the column
// map, the x-slice tables, the two segment orders and the arena of the propagation-blocked image (kernels: spmv_pb.hip); row
// blocks, tile walk, tile list and row-block launch order of the 2-D tiled image (kernel: spmv_tiled.hip).
// Plain integers in, plain structs and vectors out — standard headers only, so the arithmetic builds with a
// host compiler and is checked on the CPU, property by property, in tests/cpp/spmv_plan_test.cpp.  The builders do the rest:
// count launch, read-back, allocation, upload, scatter launches.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define LL_PLAN_HD __host__ __device__
#else
#define LL_PLAN_HD
#endif

namespace ll {

// ---------------------------------------------------------------- exchange plan of a sharded vector
// The all-gather of a vector whose shards have the stride n_shard is cut into nchunks pieces: piece c = elements
// [start[c], start[c] + len[c]) of EVERY shard.  Region c of the gathered buffer starts at nranks * start[c] elements
// and holds rank s's piece at + s * len[c].  One chunk => the buffer is the vector in global order.
constexpr int kMaxGatherChunks = 8;
struct GatherPlan {
  int nchunks = 1;
  int64_t start[kMaxGatherChunks] = {0};
  int64_t len[kMaxGatherChunks] = {0};
};

// Dynamic LDS the row-block kernels opt in to (PB phases, tiled kernel), and the x ring of the tiled kernel: its row blocks are
// as long as the ring leaves room for.
constexpr int kPbLdsCap = 160 * 1024 - 2048;
constexpr int kTlTileBytes = 16 * 1024;  // one x tile: one 16-byte piece per lane of the workgroup
constexpr int kTlSlots = 4;              // x tiles resident in LDS (a ring; power of two)

// Column -> (table index of its column block, local column).  Blocks never straddle a (rank, gather chunk) region,
// so the x slice of a block is contiguous both in the local shard and in the gathered buffer.
struct PbColMap {
  long long shard;  // shard stride of the vector partition (n when not sharded)
  int nranks, rank, nchunks;
  long long cstart[kMaxGatherChunks];  // chunk start within a shard
  int clen[kMaxGatherChunks];          // chunk length
  int bl[kMaxGatherChunks];            // block length inside the chunk
  int nb[kMaxGatherChunks];            // blocks per (rank, chunk)
  int own_base[kMaxGatherChunks];      // table index of the first own block of chunk c
  int rem_base[kMaxGatherChunks];      // table index of the first remote block of chunk c
};
LL_PLAN_HD inline int pb_block_of(const PbColMap& m, long long colg, int* local) {
  const long long s = colg / m.shard;
  const long long l = colg - s * m.shard;
  int c = 0;
  while (c + 1 < m.nchunks && l >= m.cstart[c + 1]) ++c;
  const int within = (int)(l - m.cstart[c]);
  const int b = within / m.bl[c];
  *local = within - b * m.bl[c];
  if ((int)s == m.rank) return m.own_base[c] + b;
  const int so = (m.rank >= 0 && (int)s > m.rank) ? (int)s - 1 : (int)s;  // rank < 0: no own blocks at all
  return m.rem_base[c] + so * m.nb[c] + b;
}

// ---------------------------------------------------------------- inputs
// The matrix and its partition, as the planners see them.
struct PlanShape {
  int64_t n = 0;          // global order (columns)
  int64_t n_local = 0;    // rows of this rank
  int64_t row_begin = 0;  // first of them
  int64_t shard = 0;      // shard stride of the vector partition (n when not sharded)
  int nranks = 1;
  int rank = 0;           // -1: treat the rank's own columns like everybody else's (test hook pb_test_all_remote)
  size_t elem_bytes = 8;  // sizeof(T)
  size_t acc_bytes = 8;   // sizeof(acc_t<T>)
};
// The tuning values the planners read (Tuning, ll_internal.hpp: same names, same meaning).
struct PlanTuning {
  int pb_block = 0, pb_row_block = 0, pb_col_block = 0;
  int gather_chunks = 0;
  int pb_pad = 0;
  bool tl_walk_modulo = true;
};
// What bounds a plan from outside: LDS per workgroup, columns a 16-bit local index reaches (the CPU test lowers it so that small
// shapes get several blocks per chunk), CUs of the device.
struct PlanLimits {
  int64_t lds_cap = kPbLdsCap;
  int64_t col_cap = 65536;
  int cus = 256;
};

// ================================================================= propagation-blocked image
struct PbGeometry {
  int64_t rb_rows = 0, nrb = 0, ncb = 0;
  int cb_cols = 0;    // longest column block (LDS sizing)
  int own_total = 0;  // table range [0, own_total): blocks over the rank's own columns
  int64_t pad = 16;   // entries every segment is padded to
  PbColMap map;
  GatherPlan gather;
  int chunk_first[kMaxGatherChunks] = {0};  // remote blocks of gather chunk c: [first, first + count)
  int chunk_count[kMaxGatherChunks] = {0};
  std::vector<int64_t> xoff;   // [ncb] element offset of the block's x slice in ITS source buffer
  std::vector<int32_t> ncols;  // [ncb] columns of the block
};

// Block geometry and the per-block tables.  Returns false when the image cannot be built for this shape (segment tables too
// large, or the LDS budget cannot hold a slice and its tables).
inline bool pb_plan_geometry(const PlanShape& sh, const PlanTuning& tune, const PlanLimits& lim, PbGeometry* out) {
  PbGeometry& g = *out;
  const int64_t nr = sh.n_local;
  const int P = std::max(1, sh.nranks);
  const int64_t S = sh.shard;
  // ---- row blocks (y slice in LDS, 152 KiB at most)
  // (the fixed-point form of phase 2 keeps a 16-bit exponent per row next to the accumulator)
  const int64_t row_max = std::min<int64_t>(65536, (152 * 1024) / (int64_t)(sh.acc_bytes + sizeof(int16_t)));
  auto block_len = [&](int64_t len, int64_t slice_max, int forced) {
    int64_t m = std::max<int64_t>(1, (len + 256 * slice_max - 1) / (256 * slice_max));
    int64_t b = std::max<int64_t>(16, (len + 256 * m - 1) / (256 * m));
    if (tune.pb_block > 0) b = std::max(4, tune.pb_block);
    if (forced > 0) b = std::max(4, forced);
    return std::min<int64_t>(b, slice_max);
  };
  const int64_t rb_rows = block_len(nr, row_max, tune.pb_row_block);
  const int64_t nrb = std::max<int64_t>(1, (nr + rb_rows - 1) / rb_rows);
  // ---- LDS budget of phase 1: x slice + two tables of nrb entries (the advisor's round-1 finding: check it here)
  const int64_t table_bytes = (2 * nrb + 1) * (int64_t)sizeof(long long) + 16;
  if (table_bytes + 1024 > lim.lds_cap) return false;
  const int64_t col_max =
      std::min<int64_t>(lim.col_cap, std::min<int64_t>(104 * 1024, lim.lds_cap - table_bytes) / (int64_t)sh.elem_bytes);
  if (col_max < 16) return false;

  // ---- gather chunks and column blocks
  PbColMap& m = g.map;
  std::memset(&m, 0, sizeof(m));
  m.shard = S;
  m.nranks = P;
  m.rank = sh.rank;
  const int nrem = m.rank >= 0 ? P - 1 : P;  // ranks whose columns are remote
  GatherPlan gp;
  {
    // Chunks pipeline the remote-column part of phase 1 behind the transfer, but every extra collective costs launch
    // latency and small messages use xGMI less efficiently: 4 pieces on 2 GPUs (half of the columns are own, long
    // transfer over one link pair), 2 pieces on more (the own part is 1/P, the transfer uses all links at once).
    int want = P > 1 ? (tune.gather_chunks > 0 ? tune.gather_chunks : (P == 2 ? 4 : 2)) : 1;
    want = std::max(1, std::min(want, kMaxGatherChunks));
    int64_t lc = (S + want - 1) / want;
    lc = std::max<int64_t>(256, (lc + 255) / 256 * 256);  // chunk starts stay 2 KiB aligned
    gp.nchunks = (int)std::max<int64_t>(1, (S + lc - 1) / lc);
    for (int c = 0; c < gp.nchunks; ++c) {
      gp.start[c] = c * lc;
      gp.len[c] = std::min<int64_t>(lc, S - c * lc);
    }
  }
  m.nchunks = gp.nchunks;
  int own_total = 0;
  for (int c = 0; c < gp.nchunks; ++c) {
    m.cstart[c] = gp.start[c];
    m.clen[c] = (int)gp.len[c];
    int64_t bl;
    if (P == 1) bl = block_len(gp.len[c], col_max, tune.pb_col_block);
    else {
      // Sharded: one launch of phase 1 covers the nrem other ranks' blocks of this chunk, one workgroup per block and
      // per CU at a time.  Its duration is rounds x (fixed + per-column work) with rounds = ceil(blocks / CUs), so the
      // block count per (rank, chunk) is chosen to fill whole rounds instead of the fewest blocks that fit the LDS:
      // N = 8, two chunks: 48 blocks of 13 021 columns per rank give launches of 336 blocks = 1.31 -> 2 rounds; 73
      // blocks of 8 562 columns give 511 blocks = 2 full rounds of 2/3 the length (measured on the shard shapes with
      // tools/shard_compute_probe.py).  kFixedCols: the per-workgroup fixed cost in units of one column's work.
      const int64_t nb_min = (gp.len[c] + col_max - 1) / col_max;
      const double kFixedCols = 1500.0;
      int64_t best_nb = nb_min;
      double best_cost = 1e300;
      for (int64_t nb = nb_min; nb <= 4 * nb_min + 8; ++nb) {
        const int64_t len_b = (gp.len[c] + nb - 1) / nb;
        const int64_t launch = (int64_t)std::max(1, nrem) * nb;
        const double cost = (double)((launch + lim.cus - 1) / lim.cus) * (kFixedCols + (double)len_b);
        if (cost < best_cost * 0.999) {
          best_cost = cost;
          best_nb = nb;
        }
      }
      bl = (gp.len[c] + best_nb - 1) / best_nb;
      bl = std::min<int64_t>(col_max, (bl + 3) / 4 * 4);
      if (tune.pb_block > 0) bl = std::min<int64_t>(col_max, std::max(4, tune.pb_block));
      if (tune.pb_col_block > 0) bl = std::min<int64_t>(col_max, std::max(4, tune.pb_col_block));
    }
    m.bl[c] = (int)bl;
    m.nb[c] = (int)((gp.len[c] + bl - 1) / bl);
    m.own_base[c] = own_total;
    if (m.rank >= 0) own_total += m.nb[c];
  }
  int64_t ncb = own_total;
  for (int c = 0; c < gp.nchunks; ++c) {
    m.rem_base[c] = (int)ncb;
    g.chunk_first[c] = (int)ncb;
    g.chunk_count[c] = nrem * m.nb[c];
    ncb += (int64_t)nrem * m.nb[c];
  }
  if (ncb * nrb > (int64_t)24 << 20) return false;  // segment tables would not pay off (n beyond ~6e7): keep CSR
  if (ncb * (int64_t)sizeof(int) > 60 * 1024) return false;  // LDS histogram of the build kernels
  int cb_cols = 0;
  g.xoff.assign((size_t)ncb, 0);
  g.ncols.assign((size_t)ncb, 0);
  for (int c = 0; c < gp.nchunks; ++c) {
    cb_cols = std::max(cb_cols, m.bl[c]);
    for (int sr = 0; sr < P; ++sr)
      for (int b = 0; b < m.nb[c]; ++b) {
        const bool own = sr == m.rank;
        const int idx = own ? m.own_base[c] + b
                            : m.rem_base[c] + ((m.rank >= 0 && sr > m.rank) ? sr - 1 : sr) * m.nb[c] + b;
        // the slice ends with the vector: the last rank's shard is shorter than the stride S, and what the padded all-gather ships
        // behind it is no part of x (the max |x| scan of phase 1 would take it into the fixed-point scale)
        const int64_t first_col = (int64_t)sr * S + gp.start[c] + (int64_t)b * m.bl[c];
        g.ncols[(size_t)idx] = (int32_t)std::max<int64_t>(
            0, std::min<int64_t>({(int64_t)m.bl[c], gp.len[c] - (int64_t)b * m.bl[c], sh.n - first_col}));
        g.xoff[(size_t)idx] = own ? gp.start[c] + (int64_t)b * m.bl[c]
                                  : (int64_t)P * gp.start[c] + (int64_t)sr * gp.len[c] + (int64_t)b * m.bl[c];
      }
  }
  // every segment is padded to 16 entries: kernels move quads (4 entries per lane, 16-byte accesses) and every run of
  // products written by phase 1 starts and ends on a 128-byte line (measured 3.5 % faster than quad padding)
  // (sharded images: quad padding.  Their segments hold 105 entries at N = 8 instead of 840, the 16-entry padding costs 8 % of both
  // streams there, and phase 2 measured 54.9 -> 47.8 us without it)
  g.pad = tune.pb_pad > 0 ? tune.pb_pad : (P > 1 ? 4 : 16);
  g.rb_rows = rb_rows;
  g.nrb = nrb;
  g.ncb = ncb;
  g.cb_cols = cb_cols;
  g.own_total = own_total;
  g.gather = gp;
  return true;
}

// the y slice of the fixed-point phase 2 holds 64-bit integers + one 16-bit exponent per row: it must still fit the LDS
inline bool pb_fixed_fits(int64_t rb_rows, size_t acc_bytes, int64_t lds_cap) {
  return (size_t)rb_rows * (acc_bytes + sizeof(int16_t)) + 16 <= (size_t)lds_cap;
}

// The two orders of the segments, from the count table cnt[ncb][nrb].  Column-block order: segments (c, r) with r fastest;
// row-block order: (r, c) with c fastest.
struct PbSegments {
  std::vector<int64_t> segq;     // [ncb][nrb+1] entry offsets of the segments in column-block order
  std::vector<int64_t> segdest;  // [ncb][nrb]   position of each segment in row-block order
  std::vector<int64_t> rptr;     // [nrb+1]      entry offsets of the row blocks in row-block order
  int64_t entries = 0;           // padded entry count of the image
};
inline PbSegments pb_plan_segments(const std::vector<int32_t>& cnt, int64_t ncb, int64_t nrb, int64_t pad) {
  PbSegments sg;
  sg.segq.resize((size_t)ncb * (nrb + 1));
  sg.segdest.resize((size_t)ncb * nrb);
  sg.rptr.resize((size_t)nrb + 1);
  int64_t q = 0;
  for (int64_t c = 0; c < ncb; ++c) {
    for (int64_t r = 0; r < nrb; ++r) {
      sg.segq[(size_t)c * (nrb + 1) + r] = q;
      q += ((int64_t)cnt[(size_t)c * nrb + r] + pad - 1) / pad * pad;
    }
    sg.segq[(size_t)c * (nrb + 1) + nrb] = q;
  }
  int64_t d = 0;
  for (int64_t r = 0; r < nrb; ++r) {
    sg.rptr[(size_t)r] = d;
    for (int64_t c = 0; c < ncb; ++c) {
      sg.segdest[(size_t)c * nrb + r] = d;
      d += ((int64_t)cnt[(size_t)c * nrb + r] + pad - 1) / pad * pad;
    }
  }
  sg.rptr[(size_t)nrb] = d;
  sg.entries = d;
  return sg;
}

// ONE allocation for the four big streams (values, local columns, local rows, product buffer) of `cap` entries each, starts
// 2 MiB aligned (staggering the starts against the HBM channel interleave was measured in round 2: no effect).
struct PbArena {
  size_t o_val = 0, o_col = 0, o_row = 0, o_prod = 0, total = 0;
};
inline PbArena pb_plan_arena(size_t cap, size_t elem_bytes) {
  auto up2m = [](size_t v) { return (v + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1); };
  PbArena a;
  a.o_val = 0;
  a.o_col = up2m(a.o_val + cap * elem_bytes);
  a.o_row = up2m(a.o_col + cap * sizeof(uint16_t));
  a.o_prod = up2m(a.o_row + cap * sizeof(uint16_t));
  a.total = a.o_prod + cap * elem_bytes;
  return a;
}

// ================================================================= 2-D tiled image
struct TlGeometry {
  int64_t rb_rows = 0, nrb = 0, ncb = 0;
  int tile_cols = 0;  // columns per x tile
  PbColMap map;       // one chunk, one "rank": column tile = column / tile_cols
};
// Row blocks: as long as the LDS allows (the longer the block, the smaller the share of re-staged x per entry), in whole rounds
// of 256 workgroups.  false: the shape does not fit the tables.
inline bool tl_plan_geometry(const PlanShape& sh, const PlanTuning& tune, const PlanLimits& lim, TlGeometry* out) {
  TlGeometry& g = *out;
  const int64_t nr = sh.n_local;
  const int C = kTlTileBytes / (int)sh.elem_bytes;
  const int64_t row_max =
      std::min<int64_t>(65536, (lim.lds_cap - kTlSlots * kTlTileBytes - 2048 - 64) / (int64_t)sh.acc_bytes / 256 * 256);
  int64_t rounds = std::max<int64_t>(1, (nr + 256 * row_max - 1) / (256 * row_max));
  int64_t rb_rows = std::min<int64_t>(row_max, std::max<int64_t>(16, (nr + 256 * rounds - 1) / (256 * rounds)));
  if (tune.pb_block > 0) rb_rows = std::min<int64_t>(row_max, std::max(4, tune.pb_block));
  if (tune.pb_row_block > 0) rb_rows = std::min<int64_t>(row_max, std::max(4, tune.pb_row_block));
  rb_rows = (rb_rows + 1) & ~(int64_t)1;  // even: the x buffers behind the accumulators stay 16-byte aligned
  const int64_t nrb = (nr + rb_rows - 1) / rb_rows;
  const int64_t ncb = (sh.n + C - 1) / C;
  if (ncb * (int64_t)sizeof(int) > 60 * 1024) return false;  // LDS histogram of the build kernels
  if (ncb * nrb > (int64_t)24 << 20) return false;           // count table
  PbColMap& m = g.map;
  std::memset(&m, 0, sizeof(m));
  m.shard = sh.n;
  m.nranks = 1;
  m.rank = 0;
  m.nchunks = 1;
  m.cstart[0] = 0;
  m.clen[0] = (int)std::min<int64_t>(sh.n, 0x7fffffff);
  m.bl[0] = C;
  m.nb[0] = (int)ncb;
  m.own_base[0] = 0;
  m.rem_base[0] = (int)ncb;
  g.rb_rows = rb_rows;
  g.nrb = nrb;
  g.ncb = ncb;
  g.tile_cols = C;
  return true;
}

// The tile list (non-empty tiles only), row block by row block, from the count table cnt[ncb][nrb]; every tile padded to 16
// entries (whole quads, the stream of a tile starts on a 128-byte line of both arrays).
struct TlTiles {
  std::vector<int32_t> order;   // the walk: column tiles in the order every row block visits them
  std::vector<int32_t> tfirst;  // [nrb + 1]     first tile of each row block in the tile list
  std::vector<int32_t> tcol;    // [ntiles + 1]  column tile index (+ one padding entry)
  std::vector<int64_t> tquad;   // [ntiles + 1]  first quad (4 entries) of each tile in the entry stream
  std::vector<int64_t> segq;    // [ncb][nrb+1]  entry offset of tile (c, r) (what the scatter kernel reads)
  std::vector<int32_t> rbmap;   // sharded: [nrb] row blocks in launch order (interior first); empty on one GPU
  int n_interior = 0;           // sharded: row blocks whose tiles are all own-column tiles
  int64_t entries = 0, ntiles = 0;
  bool eligible = false;        // the re-staged x slices cost less than the matrix stream, and the padding stays small
};
inline TlTiles tl_plan_tiles(const std::vector<int32_t>& cnt, const TlGeometry& g, const PlanShape& sh, int64_t nnz, bool walk_modulo) {
  TlTiles t;
  const int64_t nrb = g.nrb, ncb = g.ncb;
  const int C = g.tile_cols;
  const int64_t pad = 16;
  t.tfirst.resize((size_t)nrb + 1);
  t.segq.assign((size_t)ncb * (nrb + 1), 0);
  // Order of a row block's tiles (the sums are integers: any order gives the same bits).  Neighbouring row blocks of a banded
  // matrix share most of their column tiles, and with one contiguous eighth of the row blocks per XCD (tl_xcd_order) they
  // run at the same time behind the same L2: walking the tiles by column index MODULO the longest tile list makes every
  // row block reach the tile of residue t at about step t, so a staged x slice is fetched from the fabric once per group of
  // row blocks that share it rather than once per row block (LL_TL_WALK=0: ascending column index; A/B in DESIGN.md §3.1).
  int64_t period = 1;
  for (int64_t r = 0; r < nrb; ++r) {
    int64_t k = 0;
    for (int64_t c = 0; c < ncb; ++c) k += cnt[(size_t)c * nrb + r] != 0;
    period = std::max(period, k);
  }
  if (!walk_modulo) period = ncb;
  t.order.reserve((size_t)ncb);
  for (int64_t c0 = 0; c0 < std::min(period, ncb); ++c0)
    for (int64_t c = c0; c < ncb; c += period) t.order.push_back((int32_t)c);
  int64_t q = 0;
  for (int64_t r = 0; r < nrb; ++r) {
    t.tfirst[(size_t)r] = (int32_t)t.tcol.size();
    for (const int32_t c : t.order) {
      const int64_t k = cnt[(size_t)c * nrb + r];
      t.segq[(size_t)c * (nrb + 1) + r] = q;
      if (k == 0) continue;
      t.tcol.push_back(c);
      t.tquad.push_back(q >> 2);
      q += (k + pad - 1) / pad * pad;
    }
  }
  t.tfirst[(size_t)nrb] = (int32_t)t.tcol.size();
  t.tquad.push_back(q >> 2);
  // Sharded contexts: the row blocks whose tiles all lie inside the rank's OWN columns come first — their launch needs nothing from
  // the other ranks and runs under the all-gather; the rest follows behind it (banded matrices: the blocks next to the shard's ends).
  if (sh.nranks > 1) {
    std::vector<int32_t> rest;
    for (int64_t r = 0; r < nrb; ++r) {
      bool own = true;
      for (int32_t i = t.tfirst[(size_t)r]; i < t.tfirst[(size_t)r + 1] && own; ++i) {
        const int64_t c0 = (int64_t)t.tcol[(size_t)i] * C, c1 = std::min<int64_t>(c0 + C, sh.n);
        own = c0 >= sh.row_begin && c1 <= sh.row_begin + sh.n_local;
      }
      (own ? t.rbmap : rest).push_back((int32_t)r);
    }
    t.n_interior = (int)t.rbmap.size();
    t.rbmap.insert(t.rbmap.end(), rest.begin(), rest.end());
  }
  t.entries = q;
  t.ntiles = (int64_t)t.tcol.size();
  t.tcol.push_back(t.tcol.empty() ? 0 : t.tcol.back());  // padding entry: what a row block without tiles reads (and ignores)
  // ---- eligibility: the re-staged x slices must cost less than the matrix stream, and the padding must stay small
  const double staged = (double)t.ntiles * kTlTileBytes, stream = (double)t.entries * (sh.elem_bytes + 4);
  // (measured at twice the stream — an eighth of the banded config 3, row blocks of 4 883 rows: 0.109 ms against CSR-stream's 0.099 ms)
  t.eligible = staged <= stream && (double)t.entries <= 1.25 * (double)nnz + 16.0 * (double)nrb;
  return t;
}

}  // namespace ll
