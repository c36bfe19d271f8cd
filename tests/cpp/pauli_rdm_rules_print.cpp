// Prints what csrc/pauli_rdm_plan.hpp plans for the requests on standard input, one answer per line, so that
// tests/test_pauli_measure_large_host.py can hold its Python restatement of the launch rules against the header the kernels use.
//   blocks m                                   -> edge blocks slices partials(real) partials(complex)
//   full n_sites itemsize forced m s_0 .. s_m-1 -> t h super_tiles          (budget: the 32 KiB of kPauliTileBytes)
//   sector n_sites itemsize forced m           -> b batches
// forced = -1: the default.
#include <cstdint>
#include <iostream>
#include <string>

#include "pauli_rdm_plan.hpp"

int main() {
  const int64_t budget = 32 << 10;
  std::string what;
  while (std::cin >> what) {
    if (what == "blocks") {
      int m;
      std::cin >> m;
      std::cout << ll::pauli_rdm_block_edge(m) << ' ' << ll::pauli_rdm_blocks(m) << ' ' << ll::pauli_rdm_slices(m) << ' '
                << ll::pauli_rdm_partials(m, false) << ' ' << ll::pauli_rdm_partials(m, true) << '\n';
    } else if (what == "full") {
      int n, itemsize, forced, m;
      int32_t sites[ll::kPauliRdmMaxSites] = {};
      std::cin >> n >> itemsize >> forced >> m;
      if (m < 1 || m > ll::kPauliRdmMaxSites) return 2;
      for (int k = 0; k < m; ++k) std::cin >> sites[k];
      int which = -1;
      if (ll::pauli_rdm_check_sites(n, m, sites, &which) != ll::kRdmSitesOk) return 2;
      const int t = ll::pauli_rdm_tile_bits(n, m, sites, itemsize, forced, budget);
      const ll::PauliRdmGeom g = ll::pauli_rdm_geom(n, m, sites, t);
      std::cout << t << ' ' << g.h << ' ' << ll::pauli_rdm_super_tiles(g) << '\n';
    } else if (what == "sector") {
      int n, itemsize, forced, m;
      std::cin >> n >> itemsize >> forced >> m;
      const int b = ll::pauli_rdm_block_bits(n, m, itemsize, forced, budget);
      const int64_t nenv = (int64_t)1 << (n - m);
      std::cout << b << ' ' << ((nenv + ((int64_t)1 << b) - 1) >> b) << '\n';
    } else {
      return 2;
    }
  }
  return 0;
}
