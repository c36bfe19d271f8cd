// The host-side planning of ll_pauli_rdm_tiled (lambda-lanczos_amd/csrc/pauli_rdm_tiled_plan.hpp) against properties that follow
// from what the kernels READ and from the definition rho[a][a'] = sum_e psi(a, e) conj psi(a', e), by brute force over m = 4 .. 9
// at up to 12 sites, sites low / high / scattered / unsorted, KC = 4, 8, 16 and several ksplit:
//   - every (row, k) of a panel is loaded exactly once, into an LDS place of its own, and the states ascend in the lane counter;
//   - every state of psi belongs to exactly one (block, row, e), and it is the state of that internal index and configuration;
//   - every entry a <= a' (internal order) has exactly one (macro-tile, wave, MFMA tile, lane, register), and every partial its
//     own place;
//   - internal <-> caller order is a bijection that sorts the sites;
//   - ksplit is a power of two that divides the K-steps, fills the stated multiple of the CUs where K and the cap allow;
//   - the sector admits exactly the sector's states, and the skip rule drops exactly the tiles without an admitted pair;
//   - a CPU emulation of the whole kernel pair — the panel loads, the 16 x 16 x 4 step through the lane-map functions, the k-slices,
//     the finishing fold and mirror — reproduces F F^H on integer data, full space and sector.
// Built (plain, and with the address and undefined-behaviour sanitizers) and run by tests/test_pauli_rdm_tiled_plan_host.py.
#include <algorithm>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "pauli_rdm_tiled_plan.hpp"

using namespace ll;

static std::mt19937_64 rng(20261021);
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

static int popc(uint32_t v) { return __builtin_popcount(v); }

static std::vector<std::vector<int32_t>> site_lists(int n_sites, int m) {
  std::vector<std::vector<int32_t>> out;
  std::vector<int32_t> low, high, all((size_t)n_sites);
  for (int k = 0; k < m; ++k) low.push_back(k), high.push_back(n_sites - m + k);
  out.push_back(low);
  out.push_back(high);
  for (int s = 0; s < n_sites; ++s) all[(size_t)s] = s;
  for (int rep = 0; rep < 2; ++rep) {
    std::shuffle(all.begin(), all.end(), rng);
    std::vector<int32_t> pick(all.begin(), all.begin() + m);
    out.push_back(pick);  // scattered and unsorted
    std::sort(pick.begin(), pick.end());
    out.push_back(pick);  // scattered, ascending
  }
  std::reverse(high.begin(), high.end());
  out.push_back(high);  // descending
  return out;
}

static uint32_t caller_state(const std::vector<int32_t>& sites, uint32_t a) {
  uint32_t s = 0;
  for (size_t k = 0; k < sites.size(); ++k)
    if ((a >> k) & 1u) s |= 1u << sites[k];
  return s;
}

static void check_geometry(int n_sites, const std::vector<int32_t>& sites, int kc) {
  const int m = (int)sites.size();
  int which = 0;
  REQUIRE(pauli_rdm_tiled_check_sites(n_sites, m, sites.data(), &which) == kRdmSitesOk, "n=%d m=%d: sites refused", n_sites, m);
  const PauliRdmTiledGeom g = pauli_rdm_tiled_geom(n_sites, m, sites.data(), kc);
  const uint32_t dim = 1u << m, nb = (uint32_t)pauli_rdm_tiled_blocks_per_side(g), nk = (uint32_t)pauli_rdm_tiled_ksteps(g);
  REQUIRE(g.rb == std::min(m, 6) && g.rb + g.bb == m && (1 << g.kc_log) == kc && g.kb == std::min(g.kc_log, n_sites - m), "n=%d m=%d kc=%d: bits",
          n_sites, m, kc);
  REQUIRE(((uint64_t)nk << g.kb) == ((uint64_t)1 << (n_sites - m)), "n=%d m=%d kc=%d: K-steps", n_sites, m, kc);
  // internal <-> caller order
  std::vector<int> hit(dim, 0);
  for (uint32_t a = 0; a < dim; ++a) {
    const uint32_t ia = pauli_rdm_tiled_internal(g, a);
    REQUIRE(ia < dim && pauli_rdm_tiled_caller(g, ia) == a, "n=%d m=%d: internal(%u) = %u does not come back", n_sites, m, a, ia);
    if (ia < dim) ++hit[ia];
    REQUIRE(pauli_rdm_tiled_state(g, ia, 0) == caller_state(sites, a), "n=%d m=%d: internal %u is another subsystem configuration", n_sites, m, ia);
  }
  REQUIRE(std::all_of(hit.begin(), hit.end(), [](int c) { return c == 1; }), "n=%d m=%d: internal order is no bijection", n_sites, m);
  for (int k = 1; k < m; ++k) REQUIRE(g.all_bit[k - 1] < g.all_bit[k], "n=%d m=%d: the sites are not sorted", n_sites, m);
  // the panels
  std::vector<int> seen((size_t)1 << n_sites, 0);
  const uint32_t elems = pauli_rdm_tiled_panel_elems(g);
  REQUIRE(elems <= (uint32_t)(kPauliRdmTiledEdge * kc), "n=%d m=%d kc=%d: a panel of %u elements", n_sites, m, kc, elems);
  for (uint32_t blk = 0; blk < nb; ++blk)
    for (uint32_t step = 0; step < nk; ++step) {
      const uint32_t base = pauli_rdm_tiled_panel_base(g, blk, step);
      std::vector<int> place((size_t)kc * kPauliRdmTiledLdsStride, 0), rk((size_t)elems, 0);
      int64_t before = -1;
      for (uint32_t c = 0; c < elems; ++c) {
        const uint32_t off = pauli_rdm_tiled_panel_offset(g, c), state = base | off;
        REQUIRE((base & off) == 0 && (int64_t)state > before, "n=%d m=%d kc=%d: the states do not ascend in the counter", n_sites, m, kc);
        before = state;
        const uint32_t r = pauli_rdm_tiled_offset_row(g, off), k = pauli_rdm_tiled_offset_k(g, off);
        REQUIRE(r < (1u << g.rb) && k < (1u << g.kb), "n=%d m=%d kc=%d: (row %u, k %u) outside the panel", n_sites, m, kc, r, k);
        if (r >= (1u << g.rb) || k >= (1u << g.kb)) continue;
        ++rk[(size_t)((k << g.rb) | r)];
        const uint32_t li = pauli_rdm_tiled_lds_index(r, k);
        REQUIRE(li < place.size(), "n=%d m=%d kc=%d: LDS index %u", n_sites, m, kc, li);
        if (li < place.size()) ++place[li];
        REQUIRE(state < seen.size(), "n=%d m=%d kc=%d: state %u past the vector", n_sites, m, kc, state);
        if (state >= seen.size()) continue;
        ++seen[state];
        const uint32_t ia = (blk << kPauliRdmTiledRowBits) | r, e = (step << g.kb) | k;
        REQUIRE(pauli_rdm_tiled_state(g, ia, e) == state, "n=%d m=%d kc=%d: (block %u, row %u, e %u) is another state", n_sites, m, kc, blk, r, e);
        REQUIRE(pauli_rdm_remove_bits(state, g.all_bit, m) == e, "n=%d m=%d kc=%d: the environment of state %u", n_sites, m, kc, state);
      }
      REQUIRE(std::all_of(rk.begin(), rk.end(), [](int c) { return c == 1; }), "n=%d m=%d kc=%d: a (row, k) is not loaded exactly once", n_sites, m, kc);
      REQUIRE(std::all_of(place.begin(), place.end(), [](int c) { return c <= 1; }), "n=%d m=%d kc=%d: two elements share an LDS place", n_sites, m, kc);
    }
  REQUIRE(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }), "n=%d m=%d kc=%d: a state is not in exactly one (block, row, e)", n_sites, m, kc);
  // the owners of the entries
  const int64_t tiles = pauli_rdm_tiled_tiles(g);
  std::vector<int> owners((size_t)dim * dim, 0);
  std::vector<char> slot((size_t)tiles * 4096, 0);
  for (int64_t t = 0; t < tiles; ++t) {
    const PauliRdmBlock b = pauli_rdm_block_of((int)nb, (int)t);
    REQUIRE(b.bi <= b.bj && b.bj < (int)nb && pauli_rdm_block_number((int)nb, b.bi, b.bj) == (int)t, "nb=%u: tile %lld", nb, (long long)t);
    for (int wave = 0; wave < 4; ++wave) {
      if (!pauli_rdm_tiled_wave_live(b.bi == b.bj, wave)) continue;
      for (int ti = 0; ti < 2; ++ti)
        for (int tj = 0; tj < 2; ++tj)
          for (int lane = 0; lane < 64; ++lane)
            for (int reg = 0; reg < 4; ++reg) {
              const int row = pauli_rdm_tiled_entry_row(wave, ti, lane, reg), col = pauli_rdm_tiled_entry_col(wave, tj, lane);
              REQUIRE(row >= 0 && row < 64 && col >= 0 && col < 64, "entry (%d, %d) outside the macro-tile", row, col);
              const int64_t pi = pauli_rdm_tiled_partial_index(tiles, false, 0, t, 0, row, col);
              REQUIRE(pi >= 0 && pi < (int64_t)slot.size() && !slot[(size_t)pi], "tile %lld: partial (%d, %d) written twice", (long long)t, row, col);
              if (pi >= 0 && pi < (int64_t)slot.size()) slot[(size_t)pi] = 1;
              const uint32_t ia = ((uint32_t)b.bi << 6) | (uint32_t)row, iap = ((uint32_t)b.bj << 6) | (uint32_t)col;
              if (ia < dim && iap < dim && ia <= iap) ++owners[(size_t)ia * dim + iap];
            }
    }
  }
  bool once = true;
  for (uint32_t ia = 0; ia < dim; ++ia)
    for (uint32_t iap = ia; iap < dim; ++iap) once = once && owners[(size_t)ia * dim + iap] == 1;
  REQUIRE(once, "n=%d m=%d: an entry a <= a' has not exactly one owner", n_sites, m);
  // complex partials: every (slice, tile, part, row, col) its own place inside the buffer
  REQUIRE(pauli_rdm_tiled_partial_index(tiles, true, 2, tiles - 1, 1, 63, 63) == 3 * tiles * 8192 - 1, "the last complex partial of slice 2");
  REQUIRE(pauli_rdm_tiled_partial_index(tiles, true, 1, 0, 0, 0, 0) == tiles * 8192 && pauli_rdm_tiled_partial_index(tiles, true, 0, 1, 0, 0, 0) == 8192 &&
              pauli_rdm_tiled_partial_index(tiles, true, 0, 0, 1, 0, 0) == 4096,
          "the strides of the complex partials");
  // split-K
  for (int cplx = 0; cplx < 2; ++cplx)
    for (int forced : {0, 1, 2, 3, 8, 1000}) {
      const int64_t ks = pauli_rdm_tiled_ksplit(g, cplx != 0, forced, 256);
      REQUIRE(ks >= 1 && (ks & (ks - 1)) == 0 && nk % ks == 0, "n=%d m=%d kc=%d forced=%d: ksplit %lld of %u K-steps", n_sites, m, kc, forced, (long long)ks, nk);
      const int64_t bytes = ks * tiles * 8 * pauli_rdm_tiled_tile_doubles(cplx != 0);
      if (forced > 0) REQUIRE(ks <= forced && (2 * ks > forced || 2 * ks > nk), "forced=%d: ksplit %lld", forced, (long long)ks);
      else
        REQUIRE((ks == 1 || bytes <= kPauliRdmTiledSplitBytes) &&
                    (tiles * ks >= 2 * 256 || 2 * ks > nk || 2 * bytes > kPauliRdmTiledSplitBytes) && (ks == 1 || tiles * ks / 2 < 2 * 256),
                "n=%d m=%d kc=%d: default ksplit %lld", n_sites, m, kc, (long long)ks);
    }
}

// the sector's states through (internal index, e), and the skip rule
static void check_sector(int n_sites, const std::vector<int32_t>& sites) {
  const int m = (int)sites.size();
  const PauliRdmTiledGeom g = pauli_rdm_tiled_geom(n_sites, m, sites.data(), 4);
  for (int n_down = 0; n_down <= n_sites; ++n_down) {
    std::vector<int> seen((size_t)1 << n_sites, 0);
    for (uint32_t ia = 0; ia < (1u << m); ++ia) {
      bool any = false;
      for (uint32_t e = 0; e < (1u << (n_sites - m)); ++e) {
        const uint32_t s = pauli_rdm_tiled_state(g, ia, e);
        const bool in = pauli_rdm_tiled_admits(n_down, s);
        REQUIRE(in == (popc(ia) + popc(e) == n_down), "n=%d m=%d nd=%d: admits", n_sites, m, n_down);
        if (in) ++seen[s], any = true;
      }
      REQUIRE(pauli_rdm_tiled_row_is_zero(n_sites, m, n_down, ia) == !any, "n=%d m=%d nd=%d: row %u", n_sites, m, n_down, ia);
    }
    for (uint32_t s = 0; s < seen.size(); ++s) REQUIRE(seen[s] == (popc(s) == n_down ? 1 : 0), "n=%d m=%d nd=%d: state %u", n_sites, m, n_down, s);
  }
}
static void check_skip_rule() {
  for (int row_bits = 1; row_bits <= 6; ++row_bits)
    for (uint32_t bi = 0; bi < 128; ++bi)
      for (uint32_t bj = bi; bj < 128; ++bj) {
        bool pair = false;  // rows ra of block bi and rb of block bj with the same popcount: an entry that is not zero by rule
        for (uint32_t ra = 0; ra < (1u << row_bits) && !pair; ++ra)
          for (uint32_t rb = 0; rb < (1u << row_bits) && !pair; ++rb) pair = popc(bi) + popc(ra) == popc(bj) + popc(rb);
        REQUIRE(pauli_rdm_tiled_tile_live(bi, bj, row_bits) == pair, "row_bits=%d: tile (%u, %u) live %d", row_bits, bi, bj, (int)pair);
      }
}

// The kernel pair on the CPU, on integer data: exact sums, so rho must equal the definition entry by entry
typedef std::complex<double> Z;
static void emulate(int n_sites, const std::vector<int32_t>& sites, int kc, int forced_ksplit, int n_down /* -1: full space */) {
  const int m = (int)sites.size();
  const PauliRdmTiledGeom g = pauli_rdm_tiled_geom(n_sites, m, sites.data(), kc);
  const uint32_t dim = 1u << m, nb = (uint32_t)pauli_rdm_tiled_blocks_per_side(g);
  const int64_t tiles = pauli_rdm_tiled_tiles(g), ks = pauli_rdm_tiled_ksplit(g, true, forced_ksplit, 256);
  const uint32_t steps = (uint32_t)(pauli_rdm_tiled_ksteps(g) / ks);
  std::vector<Z> psi((size_t)1 << n_sites);
  for (size_t s = 0; s < psi.size(); ++s) {
    psi[s] = Z((double)((int)(rng() % 7) - 3), (double)((int)(rng() % 5) - 2));
    if (n_down >= 0 && popc((uint32_t)s) != n_down) psi[s] = Z(777.0, 777.0);  // outside the sector: never read
  }
  std::vector<double> partials((size_t)(ks * tiles) * 8192, -1e300);
  const int S = kPauliRdmTiledLdsStride;
  for (int64_t t = 0; t < tiles; ++t) {
    const PauliRdmBlock b = pauli_rdm_block_of((int)nb, (int)t);
    if (n_down >= 0 && !pauli_rdm_tiled_tile_live((uint32_t)b.bi, (uint32_t)b.bj, g.rb)) continue;
    for (int64_t slice = 0; slice < ks; ++slice) {
      std::vector<double> c_re((size_t)4 * 2 * 2 * 64 * 4, 0.0), c_im(c_re.size(), 0.0);  // [wave][ti][tj][lane][reg]
      for (uint32_t st = 0; st < steps; ++st) {
        std::vector<double> lds((size_t)4 * kc * S, 0.0);  // [A re, A im, B re, B im]
        for (int side = 0; side < 2; ++side) {
          const uint32_t base = pauli_rdm_tiled_panel_base(g, (uint32_t)(side ? b.bj : b.bi), (uint32_t)slice * steps + st);
          for (uint32_t c = 0; c < pauli_rdm_tiled_panel_elems(g); ++c) {
            const uint32_t off = pauli_rdm_tiled_panel_offset(g, c), state = base | off;
            const uint32_t li = pauli_rdm_tiled_lds_index(pauli_rdm_tiled_offset_row(g, off), pauli_rdm_tiled_offset_k(g, off));
            const Z v = (n_down < 0 || pauli_rdm_tiled_admits(n_down, state)) ? psi[state] : Z(0.0, 0.0);
            lds[(size_t)(2 * side) * kc * S + li] = v.real();
            lds[(size_t)(2 * side + 1) * kc * S + li] = v.imag();
          }
        }
        const double *a_re = lds.data(), *a_im = a_re + kc * S, *b_re = a_im + kc * S, *b_im = b_re + kc * S;
        for (int wave = 0; wave < 4; ++wave) {
          if (!pauli_rdm_tiled_wave_live(b.bi == b.bj, wave)) continue;
          for (int kk = 0; kk < kc / 4; ++kk)
            for (int ti = 0; ti < 2; ++ti)
              for (int tj = 0; tj < 2; ++tj) {
                double ar[64], ai[64], br[64], bi[64];  // one operand double per lane
                for (int lane = 0; lane < 64; ++lane) {
                  const uint32_t k = (uint32_t)(kk * 4 + pauli_mfma_f64_ab_k(lane));
                  const uint32_t ra = (uint32_t)(pauli_rdm_tiled_wave_row0(wave) + 16 * ti + pauli_mfma_f64_ab_row(lane));
                  const uint32_t rb = (uint32_t)(pauli_rdm_tiled_wave_col0(wave) + 16 * tj + pauli_mfma_f64_ab_row(lane));
                  ar[lane] = a_re[pauli_rdm_tiled_lds_index(ra, k)], ai[lane] = a_im[pauli_rdm_tiled_lds_index(ra, k)];
                  br[lane] = b_re[pauli_rdm_tiled_lds_index(rb, k)], bi[lane] = b_im[pauli_rdm_tiled_lds_index(rb, k)];
                }
                // D[i][j] += sum_k A[i][k] B[k][j]: A[i][k] is in the lane with (ab_row, ab_k) = (i, k), B[k][j] in the one with (j, k)
                for (int lane = 0; lane < 64; ++lane)
                  for (int reg = 0; reg < 4; ++reg) {
                    const int i = pauli_mfma_f64_cd_row(lane, reg), j = pauli_mfma_f64_cd_col(lane);
                    const size_t at = ((((size_t)wave * 2 + ti) * 2 + tj) * 64 + lane) * 4 + reg;
                    for (int k = 0; k < 4; ++k) {
                      int la = -1, lb = -1;
                      for (int l = 0; l < 64; ++l) {
                        if (pauli_mfma_f64_ab_row(l) == i && pauli_mfma_f64_ab_k(l) == k) la = l;
                        if (pauli_mfma_f64_ab_row(l) == j && pauli_mfma_f64_ab_k(l) == k) lb = l;
                      }
                      c_re[at] += ar[la] * br[lb] + ai[la] * bi[lb];
                      c_im[at] += ai[la] * br[lb] + ar[la] * (-bi[lb]);
                    }
                  }
              }
        }
      }
      for (int wave = 0; wave < 4; ++wave) {
        if (!pauli_rdm_tiled_wave_live(b.bi == b.bj, wave)) continue;
        for (int ti = 0; ti < 2; ++ti)
          for (int tj = 0; tj < 2; ++tj)
            for (int lane = 0; lane < 64; ++lane)
              for (int reg = 0; reg < 4; ++reg) {
                const size_t at = ((((size_t)wave * 2 + ti) * 2 + tj) * 64 + lane) * 4 + reg;
                const int row = pauli_rdm_tiled_entry_row(wave, ti, lane, reg), col = pauli_rdm_tiled_entry_col(wave, tj, lane);
                partials[(size_t)pauli_rdm_tiled_partial_index(tiles, true, slice, t, 0, row, col)] = c_re[at];
                partials[(size_t)pauli_rdm_tiled_partial_index(tiles, true, slice, t, 1, row, col)] = c_im[at];
              }
      }
    }
  }
  // the finishing kernel, then the definition
  long long wrong = 0;
  for (uint32_t a = 0; a < dim; ++a)
    for (uint32_t ap = a; ap < dim; ++ap) {
      Z got(0.0, 0.0);
      const bool by_rule = n_down >= 0 && (popc(a) != popc(ap) || pauli_rdm_tiled_row_is_zero(n_sites, m, n_down, a));
      if (!by_rule) {
        uint32_t ia = pauli_rdm_tiled_internal(g, a), iap = pauli_rdm_tiled_internal(g, ap);
        const bool swapped = ia > iap;
        if (swapped) std::swap(ia, iap);
        const int tile = pauli_rdm_block_number((int)nb, (int)(ia >> 6), (int)(iap >> 6));
        double re = 0.0, im = 0.0;
        for (int64_t s = 0; s < ks; ++s) {
          re += partials[(size_t)pauli_rdm_tiled_partial_index(tiles, true, s, tile, 0, (int)(ia & 63), (int)(iap & 63))];
          im += partials[(size_t)pauli_rdm_tiled_partial_index(tiles, true, s, tile, 1, (int)(ia & 63), (int)(iap & 63))];
        }
        got = Z(re, swapped ? -im : im);
      }
      Z want(0.0, 0.0);
      const uint32_t sa = caller_state(sites, a), sap = caller_state(sites, ap);
      for (uint32_t e = 0; e < (1u << (n_sites - m)); ++e) {
        const uint32_t env = pauli_rdm_insert_zeros(e, g.all_bit, m);
        if (n_down >= 0 && (popc(env | sa) != n_down || popc(env | sap) != n_down)) continue;
        want += psi[env | sa] * std::conj(psi[env | sap]);
      }
      if (got != want) ++wrong;
    }
  REQUIRE(wrong == 0, "n=%d m=%d kc=%d ksplit=%lld n_down=%d: %lld entries differ from F F^H", n_sites, m, kc, (long long)ks, n_down, wrong);
}

int main() {
  // the lane maps: every (row, k) of an operand and every (row, column) of a result in exactly one (lane[, register])
  {
    int ab[16][4] = {}, cd[16][16] = {};
    for (int lane = 0; lane < 64; ++lane) {
      ++ab[pauli_mfma_f64_ab_row(lane)][pauli_mfma_f64_ab_k(lane)];
      for (int reg = 0; reg < 4; ++reg) ++cd[pauli_mfma_f64_cd_row(lane, reg)][pauli_mfma_f64_cd_col(lane)];
    }
    bool ok = true;
    for (int i = 0; i < 16; ++i) {
      for (int k = 0; k < 4; ++k) ok = ok && ab[i][k] == 1;
      for (int j = 0; j < 16; ++j) ok = ok && cd[i][j] == 1;
    }
    REQUIRE(ok, "the MFMA lane maps are no bijections");
  }
  for (uint32_t mask : {0x0u, 0x1u, 0xF0u, 0x8421u, 0xFFFFFFFFu, 0x80000001u})
    for (uint32_t v = 0; v < 64; ++v) {
      const uint32_t d = pauli_rdm_tiled_pdep(v, mask);
      REQUIRE((d & ~mask) == 0 && pauli_rdm_tiled_pext(d, mask) == (v & ((popc(mask) >= 32 ? 0u : (1u << popc(mask))) - 1u)),
              "pdep / pext through mask %x", mask);
    }
  int which = 0;
  const int32_t three[3] = {0, 1, 2}, rep[4] = {0, 1, 2, 1}, far[4] = {0, 1, 2, 9};
  std::vector<int32_t> fourteen;
  for (int s = 0; s < 14; ++s) fourteen.push_back(s);
  REQUIRE(pauli_rdm_tiled_check_sites(8, 3, three, &which) == kRdmBadCount, "three sites pass");
  REQUIRE(pauli_rdm_tiled_check_sites(20, 14, fourteen.data(), &which) == kRdmBadCount, "fourteen sites pass");
  REQUIRE(pauli_rdm_tiled_check_sites(20, 13, fourteen.data(), &which) == kRdmSitesOk, "thirteen sites do not pass");
  REQUIRE(pauli_rdm_tiled_check_sites(3, 4, rep, &which) == kRdmBadCount, "more sites than the system has");
  REQUIRE(pauli_rdm_tiled_check_sites(8, 4, rep, &which) == kRdmSiteRepeated && which == 3, "the repeated site");
  REQUIRE(pauli_rdm_tiled_check_sites(8, 4, far, &which) == kRdmSiteOutOfRange && which == 3, "the site outside");
  REQUIRE(pauli_rdm_tiled_kc(0) == 16 && pauli_rdm_tiled_kc(4) == 4 && pauli_rdm_tiled_kc(7) == 4 && pauli_rdm_tiled_kc(8) == 8 &&
              pauli_rdm_tiled_kc(1) == 4 && pauli_rdm_tiled_kc(64) == 16,
          "the forced KC");
  for (int m = 4; m <= 9; ++m)
    for (int n_sites : {m, m + 1, m + 2, m + 3, 12}) {
      if (n_sites < m || n_sites > 12) continue;
      for (const std::vector<int32_t>& sites : site_lists(n_sites, m))
        for (int kc : {4, 8, 16}) check_geometry(n_sites, sites, kc);
    }
  for (int m : {4, 5, 7})
    for (int n_sites : {m, m + 2, 10})
      for (const std::vector<int32_t>& sites : site_lists(n_sites, m)) check_sector(n_sites, sites);
  check_skip_rule();
  struct Emu { int n, m, kc, ks, nd; };
  for (const Emu& e : {Emu{4, 4, 16, 0, -1}, Emu{5, 4, 4, 0, -1}, Emu{7, 5, 8, 1, -1}, Emu{9, 6, 4, 2, -1}, Emu{9, 7, 4, 0, -1}, Emu{10, 7, 4, 2, -1},
                       Emu{10, 8, 4, 1, -1}, Emu{10, 7, 4, 2, 5}, Emu{9, 5, 8, 2, 3}, Emu{10, 7, 16, 0, 1}})
    for (const std::vector<int32_t>& sites : site_lists(e.n, e.m)) emulate(e.n, sites, e.kc, e.ks, e.nd);
  std::printf("%lld checks, %lld failures\n", checks, fails);
  return fails == 0 ? 0 : 1;
}
