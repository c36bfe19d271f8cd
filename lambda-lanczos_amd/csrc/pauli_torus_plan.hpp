// Host-side arithmetic of the translation group of an Lx x Ly torus (kernel: pauli_torus.hip; creation: pauli_operators.cpp
// create_pauli_torus; measuring: pauli_expect_block_plan.hpp): the two translations on a state or a mask, the code of an element
// and of its inverse, the numerator of its character, and the enumeration of a block's representatives.  Plain integers in,
// plain vectors out — standard headers only, so the arithmetic builds with a host compiler and is checked on the CPU, property
// by property, in tests/cpp/pauli_torus_plan_test.cpp.
//
// Site (x, y) is bit x + Lx y, n = Lx Ly <= 30.  T_x rotates each of the Ly fields of Lx bits left by one: site (x, y) goes to
// ((x + 1) mod Lx, y).  T_y rotates the n-bit word left by Lx bits: site (x, y) goes to (x, (y + 1) mod Ly).  The element
// T_x^a T_y^b has the code a + Lx b and the character e^(-2 pi i k / n) with k = (m_x a Ly + m_y b Lx) mod n; with Ly = 1 (or
// Lx = 1) codes and k are the ring's shift j and (m j) mod L.
#pragma once

#include <cstdint>
#include <vector>

namespace ll {

struct PauliTorus {
  int lx, ly;
  uint32_t smask, c0;  // the n site bits; the bits of the sites (0, y): where T_x brings the top bit of each field
  PauliTorus(int lx_, int ly_) : lx(lx_), ly(ly_), smask((uint32_t)(((uint64_t)1 << (lx_ * ly_)) - 1)), c0(0) {
    for (int y = 0; y < ly; ++y) c0 |= (uint32_t)1 << (lx * y);
  }
  int sites() const { return lx * ly; }
  uint32_t site_mask() const { return smask; }
  uint32_t col0() const { return c0; }
  uint32_t tx(uint32_t v) const { return ((v << 1) & smask & ~c0) | ((v >> (lx - 1)) & c0); }
  uint32_t ty(uint32_t v) const {
    const uint64_t w = v;
    return (uint32_t)(((w << lx) | (w >> (sites() - lx))) & smask);
  }
  // T_x^a T_y^b v, 0 <= a < lx, 0 <= b < ly
  uint32_t move(uint32_t v, int a, int b) const {
    for (int j = 0; j < b; ++j) v = ty(v);
    for (int j = 0; j < a; ++j) v = tx(v);
    return v;
  }
  int code(int a, int b) const { return a + lx * b; }
  int inverse_code(int c) const {
    const int a = c % lx, b = c / lx;
    return (a == 0 ? 0 : lx - a) + lx * (b == 0 ? 0 : ly - b);
  }
  // k of the character e^(-2 pi i k / n) of the element `c`: (m_x a / Lx + m_y b / Ly) as one fraction over n
  int phase_num(int mx, int my, int c) const {
    const int a = c % lx, b = c / lx;
    return (int)(((int64_t)mx * a * ly + (int64_t)my * b * lx) % sites());
  }
};

// Is r the representative of its orbit (no image below it) with the character (m_x, m_y) equal to 1 on its stabiliser?  Returns
// the stabiliser's size then, 0 otherwise.  The walk is the kernel's: b outer, a inner; it ends at the first smaller image.
inline int pauli_torus_admit(const PauliTorus& g, int mx, int my, uint32_t r) {
  int stab = 0;
  bool admitted = true;
  uint32_t cur = r;
  for (int b = 0, c = 0; b < g.ly; ++b) {
    for (int a = 0; a < g.lx; ++a, ++c) {
      if (cur < r) return 0;
      if (cur == r) {
        ++stab;
        if (g.phase_num(mx, my, c) != 0) admitted = false;
      }
      cur = g.tx(cur);
    }
    cur = g.ty(cur);
  }
  return admitted ? stab : 0;
}

// The admitted representatives among the states top << low_bits | low, low < 2^low_bits, of the full space (n_down < 0) or with
// n_down set bits, ascending, with their orbit lengths n / |stabiliser| appended to reps / orbit_len: one slice of a block's
// basis, so that slices taken in ascending `top` concatenate to the basis (creation runs them on several threads).
inline void pauli_torus_slice(const PauliTorus& g, int n_down, int mx, int my, uint32_t top, int low_bits, std::vector<uint32_t>& reps,
                              std::vector<uint8_t>& orbit_len) {
  const int n = g.sites();
  const uint64_t span = (uint64_t)1 << low_bits;
  const uint32_t high = (uint32_t)((uint64_t)top << low_bits);
  auto visit = [&](uint32_t r) {
    const int stab = pauli_torus_admit(g, mx, my, r);
    if (stab != 0) {
      reps.push_back(r);
      orbit_len.push_back((uint8_t)(n / stab));
    }
  };
  if (n_down < 0) {
    for (uint64_t low = 0; low < span; ++low) visit(high | (uint32_t)low);
    return;
  }
  const int k = n_down - __builtin_popcount(top);  // set bits left for the low part
  if (k < 0 || k > low_bits) return;
  if (k == 0) {
    visit(high);
    return;
  }
  for (uint64_t low = ((uint64_t)1 << k) - 1; low < span;) {  // the next word with as many set bits follows (Gosper)
    visit(high | (uint32_t)low);
    const uint64_t c = low & (0 - low), r = low + c;
    low = (((r ^ low) >> 2) >> __builtin_ctzll(low)) | r;
  }
}

}  // namespace ll
