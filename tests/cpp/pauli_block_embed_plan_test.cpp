// lambda-lanczos_amd/csrc/pauli_block_embed_plan.hpp on the CPU: the block / target compatibility rule over every combination of
// (block kind, n_down or none, target kind, n_down), the two factor tables and the launch geometry.
//
// Without arguments the program checks the properties below and prints "<n> failures".  With the argument "ask" it answers the
// questions on its standard input, one line each, so that tests/test_pauli_block_embed_plan_host.py can compare a Python
// restatement with the header itself:
//   fault <block role> <n_sites> <n_down> <elem_bytes> <complex> <target role> <n_sites> <n_down> <elem_bytes> <complex>
//                                         -> "ok" or the cause
//   expand_factors                        -> 121 doubles as hexadecimal floats
//   project_factors <|G|>                 -> the same
//   launch <count> <forced> <default> <max grid>   -> bits units grid
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "pauli_block_embed_plan.hpp"

using namespace ll;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++failures;                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
    }                                                                 \
  } while (0)

static PauliEmbedSide side(PauliEmbedRole r, int n_sites, int n_down, int eb = 8, bool cx = false) {
  PauliEmbedSide s;
  s.role = r;
  s.n_sites = n_sites;
  s.n_down = n_down;
  s.elem_bytes = eb;
  s.is_complex = cx;
  return s;
}

static void print_table(const std::vector<double>& f) {
  for (size_t i = 0; i < f.size(); ++i) std::printf("%s%a", i ? " " : "", f[i]);
  std::printf("\n");
}

static int ask() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "fault") {
      int v[10];
      for (int& x : v) in >> x;
      const char* f = pauli_block_embed_fault(side((PauliEmbedRole)v[0], v[1], v[2], v[3], v[4] != 0),
                                              side((PauliEmbedRole)v[5], v[6], v[7], v[8], v[9] != 0));
      std::printf("%s\n", f ? f : "ok");
    } else if (what == "expand_factors") {
      print_table(pauli_block_expand_factors());
    } else if (what == "project_factors") {
      int g = 0;
      in >> g;
      print_table(pauli_block_project_factors(g));
    } else if (what == "launch") {
      long long count = 0;
      int forced = 0, dflt = 0, max_grid = 0;
      in >> count >> forced >> dflt >> max_grid;
      const PauliEmbedLaunch l = pauli_block_embed_launch((int64_t)count, forced, dflt, max_grid);
      std::printf("%d %" PRId64 " %d\n", l.bits, l.units, l.grid);
    } else {
      return 2;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "ask") == 0) return ask();

  // ---- the compatibility rule, restated: a sector target takes the sector blocks of its n_down, a full-space target every block
  const PauliEmbedRole blocks[] = {kPauliEmbedBlockMomentum, kPauliEmbedBlockMomentumFull, kPauliEmbedBlockSymmetric};
  const PauliEmbedRole targets[] = {kPauliEmbedTargetFull, kPauliEmbedTargetSector};
  int admitted = 0, refused = 0;
  for (PauliEmbedRole br : blocks)
    for (int bd = -1; bd <= 6; ++bd) {
      if (br == kPauliEmbedBlockMomentum && bd < 0) continue;      // a momentum block of a sector always has one
      if (br == kPauliEmbedBlockMomentumFull && bd >= 0) continue; // the full-space block never
      for (PauliEmbedRole tr : targets)
        for (int td = -1; td <= 6; ++td) {
          if ((tr == kPauliEmbedTargetSector) != (td >= 0)) continue;
          const bool sector_block = bd >= 0;
          const bool want = tr == kPauliEmbedTargetFull || (sector_block && bd == td);
          const char* f = pauli_block_embed_fault(side(br, 6, bd), side(tr, 6, td));
          CHECK((f == nullptr) == want);
          if (f && tr == kPauliEmbedTargetSector && !sector_block) CHECK(std::strstr(f, "full-space block") != nullptr);
          if (f && tr == kPauliEmbedTargetSector && sector_block) CHECK(std::strstr(f, "n_down") != nullptr);
          (f ? refused : admitted)++;
        }
    }
  CHECK(admitted == 7 + 1 + 8 + 7 + 7 && refused > 0);  // full target: 7 + 1 + 8 blocks; sector target: equal n_down, twice 7
  // n_sites, the storage type, the roles
  CHECK(std::strstr(pauli_block_embed_fault(side(kPauliEmbedBlockMomentum, 6, 3), side(kPauliEmbedTargetSector, 8, 3)), "n_sites"));
  CHECK(std::strstr(pauli_block_embed_fault(side(kPauliEmbedBlockMomentum, 6, 3, 8, false), side(kPauliEmbedTargetSector, 6, 3, 4, false)),
                    "storage type"));
  CHECK(std::strstr(pauli_block_embed_fault(side(kPauliEmbedBlockMomentum, 6, 3, 8, false), side(kPauliEmbedTargetSector, 6, 3, 8, true)),
                    "storage type"));
  CHECK(pauli_block_embed_fault(side(kPauliEmbedBlockSymmetric, 6, 3, 16, true), side(kPauliEmbedTargetSector, 6, 3, 16, true)) == nullptr);
  for (PauliEmbedRole r : {kPauliEmbedOther, kPauliEmbedTargetFull, kPauliEmbedTargetSector})
    CHECK(std::strstr(pauli_block_embed_fault(side(r, 6, -1), side(kPauliEmbedTargetFull, 6, -1)), "no symmetry block"));
  for (PauliEmbedRole r : {kPauliEmbedOther, kPauliEmbedBlockMomentum, kPauliEmbedBlockMomentumFull, kPauliEmbedBlockSymmetric})
    CHECK(std::strstr(pauli_block_embed_fault(side(kPauliEmbedBlockMomentumFull, 6, -1), side(r, 6, -1)), "target operator"));

  // ---- the factor tables
  const std::vector<double> ef = pauli_block_expand_factors();
  CHECK(ef.size() == 121 && ef[0] == 0.0 && ef[1] == 1.0 && ef[4] == 0.5);
  for (int R = 1; R <= 120; ++R) {
    CHECK(ef[(size_t)R] == 1.0 / std::sqrt((double)R));
    CHECK(std::fabs(ef[(size_t)R] * ef[(size_t)R] * R - 1.0) <= 4 * 2.3e-16);
  }
  for (int L : {1, 4, 7, 12, 30})
    for (int mult : {1, 2, 4}) {
      const int G = L * mult;
      CHECK(pauli_block_group_size(L, mult >= 2, mult == 4) == G || mult == 2);
      const std::vector<double> pf = pauli_block_project_factors(G);
      CHECK(pf.size() == 121 && pf[0] == 0.0);
      for (int R = 1; R <= 120; ++R) {
        CHECK(pf[(size_t)R] == (R <= G ? std::sqrt((double)R) / (double)G : 0.0));
        // the |G| / R elements that reach a state of the orbit, each with 1 / sqrt(R): (|G| / R) * factor = 1 / sqrt(R)
        if (R <= G && G % R == 0) CHECK(std::fabs(pf[(size_t)R] * (G / R) - ef[(size_t)R]) <= 4 * 2.3e-16 * ef[(size_t)R]);
      }
    }
  CHECK(pauli_block_group_size(30, true, true) == 120 && pauli_block_group_size(30, false, true) == 60 &&
        pauli_block_group_size(7, false, false) == 7);

  // ---- the launch geometry
  {
    PauliEmbedLaunch l = pauli_block_embed_launch((int64_t)1 << 30, -1, kPauliBlockExpandBlockBits, 2048);
    CHECK(l.bits == 10 && l.units == ((int64_t)1 << 20) && l.grid == 2048);
    l = pauli_block_embed_launch(142506, 6, kPauliBlockExpandBlockBits, 2048);
    CHECK(l.bits == 6 && l.units == 2227 && l.grid == 2048);
    l = pauli_block_embed_launch(142506, -1, kPauliBlockExpandBlockBits, 2048);
    CHECK(l.bits == 10 && l.units == 140 && l.grid == 140);
    l = pauli_block_embed_launch(4750, 0, kPauliBlockProjectBlockBits, 2048);
    CHECK(l.bits == 0 && l.units == 4750 && l.grid == 2048);
    l = pauli_block_embed_launch(4750, -1, kPauliBlockProjectBlockBits, 2048);
    CHECK(l.bits == 8 && l.units == 19 && l.grid == 19);
    l = pauli_block_embed_launch(1, 99, kPauliBlockProjectBlockBits, 2048);
    CHECK(l.bits == 30 && l.units == 1 && l.grid == 1);
    for (int64_t count : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)99860, (int64_t)1 << 21})
      for (int bits = 0; bits <= 12; ++bits) {
        l = pauli_block_embed_launch(count, bits, 8, 2048);
        CHECK((l.units << bits) >= count && ((l.units - 1) << bits) < count && l.grid >= 1 && l.grid <= 2048 && l.grid <= l.units);
      }
  }
  std::printf("pauli_block_embed_plan_test: %d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
