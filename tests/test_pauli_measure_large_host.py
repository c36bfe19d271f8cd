"""What tests/test_gpu_pauli_measure_large.py rests on, without a GPU: the trip counts of its cases by a Python restatement of the
four launch rules (and that no case of the 14-site files of the measuring kernels ever took a second trip), the restatement
against csrc/pauli_rdm_plan.hpp itself, the integer state and its exactness condition, and the fast host references against the
plain ones of generators.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import pauli_large_cases as PL
import pauli_measure_large_cases as C
import test_gpu_pauli_expect as TE
import test_gpu_pauli_rdm as TR
from lambda_lanczos_amd import generators as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trips(units, grid):
    """(the fewest, the most) trips a workgroup takes."""
    return units // grid, -(-units // grid)


# ------------------------------------------------------------------ the trip counts
@pytest.mark.parametrize("kernel", list(C.TABLES))
def test_every_case_wraps(kernel):
    """units > grid for every case but those of BELOW_WRAP, which do not; a grid that is no power of two leaves a ragged last
    trip; every storage type has a case of three or more trips."""
    most = {t: 0 for t in C.ALL}
    for case in C.TABLES[kernel]:
        units, grid = C.launch_of(kernel, case)
        assert grid <= C.MAX_GRID and (grid == units or grid == C.MAX_GRID or kernel.startswith("rdm")), case
        if C.case_key(kernel, case) in C.BELOW_WRAP:
            assert units <= grid, case
            continue
        assert units > grid, (case, units, grid)
        if grid & (grid - 1):
            assert units % grid != 0, (case, units, grid)
        most[case[0]] = max(most[case[0]], _trips(units, grid)[1])
    assert all(v >= 3 for v in most.values()), (kernel, most)
    assert {k[0] for k in C.BELOW_WRAP} <= set(C.TABLES) and all(
        any(C.case_key(k[0], c) == k for c in C.TABLES[k[0]]) for k in C.BELOW_WRAP)   # no stale exception


def test_the_pinned_numbers_of_the_case_tables():
    for t in C.ALL:
        isz = np.dtype(C.TYPES[t]).itemsize
        assert C.expect_full_launch(20, isz, 6) == (16384, 2048) and C.expect_full_launch(20, isz, 9) == (2048, 2048)
        assert C.launch_of("expect_sector", (t, (20, 10), "small")) == (11548, 2048)
        assert C.launch_of("expect_sector", (t, (30, 4), "small")) == (6852, 2048)
        assert C.launch_of("rdm_sector", (t, (20, 10), [19], 4)) == (32768, 2048)
        assert C.launch_of("rdm_sector", (t, (20, 10), C.SIX_20, 4)) == (1024, 240 if t in "zc" else 481)
        for sites in ([29], [0, 15, 14], C.SIX_30):
            units, grid = C.launch_of("rdm_sector", (t, (30, 4), sites, None))
            assert 131072 <= units <= 524288 and units // grid >= 64, (t, sites, units, grid)
    assert max(C.launch_of("rdm_sector", (t, (30, 4), C.SIX_30, None))[0] // C.launch_of("rdm_sector", (t, (30, 4), C.SIX_30, None))[1]
               for t in C.ALL) > 2000
    assert C.expect_full_launch(23, 16) == (4096, 2048) and C.expect_full_launch(24, 8) == (4096, 2048)
    assert C.launch_of("expect_sector", ("d", (24, 12), None)) == (2641, 2048)
    assert C.launch_of("rdm_sector", ("z", (20, 10), [1, 3, 5, 9, 13, 19], None)) == (512, 240)
    assert C.launch_of("rdm_sector", ("d", (24, 12), [0, 23], None))[0] > 2048
    for case in C.RDM_FULL:
        assert C.launch_of("rdm_full", case) == case[4:6], case
    assert PL.small_bits(math.comb(20, 10)) == 4 and PL.small_bits(math.comb(30, 4)) == 2
    assert math.comb(30, 4) == 27405 and (30 + 1) // 2 == 15      # the admitted (a, e) of 2^30; both rank tables at 2^15 entries
    unsorted = [c for c in C.RDM_FULL + C.RDM_SECTOR if list(c[2]) != sorted(c[2])]
    assert len({tuple(c[2]) for c in unsorted}) >= 2
    assert {tuple(sorted(c[2])) for c in C.RDM_SECTOR if c[1] == (30, 4)} == {(29,), (0, 14, 15), (2, 7, 14, 15, 22, 29)}
    assert C.rdm_grid(10 ** 9, 5, False) == 1820 and C.rdm_grid(10 ** 9, 5, True) == 910
    assert C.rdm_grid(10 ** 9, 6, False) == 481 and C.rdm_grid(10 ** 9, 6, True) == 240
    assert all(C.rdm_grid(10 ** 9, m, cplx) == 2048 for m in (1, 2, 3, 4) for cplx in (False, True))


def test_the_14_site_files_never_take_a_second_trip():
    """The statement the large file rests on: over every case of tests/test_gpu_pauli_expect.py and tests/test_gpu_pauli_rdm.py, at
    every forced tile or block size and in every storage type, the units of work never exceed the grid.  A later change that
    gives those files a wrapping case updates this assertion."""
    worst = {"expect_full": 0, "expect_sector": 0, "rdm_full": 0, "rdm_sector": 0}
    for dtype in TE.TYPES:
        isz = np.dtype(dtype).itemsize
        for n_sites in TE.FULL_SITES:
            for bits in TE.TILE_BITS:
                units, grid = C.expect_full_launch(n_sites, isz, bits)
                assert units <= grid
                worst["expect_full"] = max(worst["expect_full"], units)
        for n_sites, n_down in TE.SECTORS:
            for bits in TE.BLOCK_BITS:
                units, grid = C.expect_sector_launch(math.comb(n_sites, n_down), bits)
                assert units <= grid
                worst["expect_sector"] = max(worst["expect_sector"], units)
    for dtype in TR.TYPES:
        for n_sites, sites in TR.FULL_CASES:
            for bits in TR.TILE_BITS:
                units, grid = C.rdm_full_launch(n_sites, sites, dtype, bits)
                assert units <= grid, (n_sites, sites, bits)
                worst["rdm_full"] = max(worst["rdm_full"], units)
        for n_sites, n_down in TR.SECTORS:
            for sites in TR.sector_site_lists(n_sites):
                for bits in TR.BLOCK_BITS:
                    units, grid = C.rdm_sector_launch(n_sites, len(sites), dtype, bits)
                    assert units <= grid, (n_sites, sites, bits)
                    worst["rdm_sector"] = max(worst["rdm_sector"], units)
    assert worst == {"expect_full": 256, "expect_sector": 215, "rdm_full": 128, "rdm_sector": 512}      # against 2048, or 240 at least


# ------------------------------------------------------------------ the restated rules against the header
def _ask(tmp_path, lines):
    exe = str(tmp_path / "pauli_rdm_rules_print")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pauli_rdm_rules_print.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True)
    out = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def test_the_restated_rdm_rules_are_those_of_the_plan_header(tmp_path):
    """pauli_rdm_blocks, pauli_rdm_partials, pauli_rdm_tile_bits, pauli_rdm_super_tiles and pauli_rdm_block_bits of
    csrc/pauli_rdm_plan.hpp, asked through a host program, for m = 1 .. 6, every case of the large tables and every case of the
    14-site file."""
    assert [C.rdm_blocks(m) for m in range(1, 7)] == [3, 10, 10, 10, 36, 136]      # NB of the header comment of pauli_rdm.hip
    assert [C.RDM_THREADS // C.rdm_blocks(m) for m in range(1, 7)] == [85, 25, 25, 25, 7, 1]
    lines, want = [], []
    for m in range(1, 7):
        lines.append("blocks %d" % m)
        want.append([C.rdm_block_edge(m), C.rdm_blocks(m), C.RDM_THREADS // C.rdm_blocks(m), C.rdm_partials(m, False),
                     C.rdm_partials(m, True)])
    full = [(C.TYPES[c[0]], c[1], c[2], c[3]) for c in C.RDM_FULL]
    full += [(d, n, s, b) for d in TR.TYPES for n, s in TR.FULL_CASES for b in TR.TILE_BITS]
    for dtype, n, sites, forced in full:
        isz = np.dtype(dtype).itemsize
        lines.append("full %d %d %d %d %s" % (n, isz, -1 if forced is None else forced, len(sites), " ".join(map(str, sites))))
        t, h = C.rdm_tile_bits(n, sites, isz, forced)
        want.append([t, h, C.rdm_full_launch(n, sites, dtype, forced)[0]])
    sector = [(C.TYPES[c[0]], c[1][0], len(c[2]), c[3]) for c in C.RDM_SECTOR]
    sector += [(d, n, len(s), b) for d in TR.TYPES for n, _ in TR.SECTORS for s in TR.sector_site_lists(n) for b in TR.BLOCK_BITS]
    for dtype, n, m, forced in sector:
        isz = np.dtype(dtype).itemsize
        lines.append("sector %d %d %d %d" % (n, isz, -1 if forced is None else forced, m))
        want.append([C.rdm_block_bits(n, m, isz, forced), C.rdm_sector_launch(n, m, dtype, forced)[0]])
    got = _ask(tmp_path, lines)
    for ln, g, w in zip(lines, got, want):
        assert g == w, (ln, g, w)


# ------------------------------------------------------------------ the instrument
def test_integer_states_are_exact_in_every_storage_type():
    n = 4096
    for t, dtype in C.TYPES.items():
        x = C.integer_state(n, dtype, 5)
        assert x.dtype == np.dtype(dtype) and x.shape == (n,)
        wide = x.astype(np.complex128)
        ref = C.integer_state(n, np.complex128 if t in "zc" else np.float64, 5).astype(np.complex128)
        assert np.array_equal(wide, ref)                                   # the same integers in the narrow type
        parts = [wide.real] + ([wide.imag] if t in "zc" else [])
        for p in parts:
            assert np.array_equal(p, np.rint(p)) and np.all(np.abs(p) >= 1) and np.all(np.abs(p) <= C.AMP)
            assert set(np.unique(p).tolist()) == set(range(-C.AMP, 0)) | set(range(1, C.AMP + 1))
        if t in "ds":
            assert not np.iscomplexobj(x)
        assert np.array_equal(x, C.integer_state(n, dtype, 5)) and not np.array_equal(x, C.integer_state(n, dtype, 6))
    largest = max([1 << c[1] for c in C.EXPECT_FULL + C.RDM_FULL] + [math.comb(*c[1]) for c in C.EXPECT_SECTOR + C.RDM_SECTOR])
    assert largest == 1 << 24 and C.exact_condition(largest) and 2 * 7 * 7 * largest < 2 ** 32 < 2 ** 53
    assert not C.exact_condition(2 ** 47)


# ------------------------------------------------------------------ the observables
@pytest.mark.parametrize("sector", [False, True], ids=["full", "sector"])
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_observables(cplx, sector):
    for n_sites, k in ((20, 6), (20, 9), (23, 11), (24, 12), (20, 10), (30, 15)):
        if sector and n_sites % 2:
            continue   # the sectors of the cases have an even number of sites: X...X flips an even number of bits
        obs = C.observables(n_sites, k, cplx, sector)
        top = n_sites - 1
        slots = C.slots_of(obs, cplx, sector)
        assert 35 <= len(obs) <= 45 and 32 < slots < 64 and slots % C.EXPECT_BATCH != 0          # two batches, the second ragged
        assert obs == C.observables(n_sites, k, cplx, sector)
        masks = {(x, z) for x, z, _ in obs}
        bit = lambda *s: sum(1 << j for j in s)   # noqa: E731
        assert {(0, 0), (bit(top), 0), (bit(top), bit(top)), (0, bit(top)), (bit(0, top), 0), (bit(k - 1, k), 0),
                (0, bit(k - 1, k)), (bit(k + 1, top), 0), ((1 << n_sites) - 1, 0), (0, (1 << n_sites) - 1)} <= masks
        ny = [bin(x & z).count("1") for x, z, _ in obs]
        assert 2 in ny and ({1, 3} <= set(ny)) == cplx
        assert all((x | z) >> n_sites == 0 for x, z, _ in obs)
        assert all(math.frexp(abs(c))[0] != 0.5 for _, _, c in obs)                          # no power of two
        odd = [t for t in obs if bin(t[0]).count("1") % 2]
        if sector:
            assert [t[:2] for t in odd] == [(bit(top), 0), (bit(top), bit(top))]             # X and Y on the top site
        else:
            assert len(odd) > 4
        if not cplx:   # only Y on the top site is left to the zero rule of real storage
            assert [t[:2] for t in obs if bin(t[0] & t[1]).count("1") % 2] == [(bit(top), bit(top))]
        assert len({x for x, _, _ in obs if x >> k}) >= 6                                  # partner tiles / both rank tables


# ------------------------------------------------------------------ the fast references against the plain ones
@pytest.mark.parametrize("tid", list(C.TYPES))
def test_expectation_sums_are_those_of_the_plain_reference(tid):
    """expect_sums_full and expect_sums_sector against <psi, P psi> with P psi by generators.pauli_string_apply_np, summed in
    double: all integers, so equal."""
    dtype = C.TYPES[tid]
    cplx = tid in "zc"
    for n_sites, n_down, k in ((12, None, 6), (11, None, 4), (12, 6, 6), (13, 4, 7), (26, 3, 13)):
        sector = n_down is not None
        states = G.sector_states(n_sites, n_down) if sector else None
        n = states.shape[0] if sector else 1 << n_sites
        psi = C.integer_state(n, dtype, 3)
        obs = C.observables(n_sites, k, cplx, sector)
        sums = C.expect_sums_sector(n_sites, n_down, psi, obs) if sector else C.expect_sums_full(n_sites, psi, obs)
        got = C.expect_values(sums, obs, cplx, sector)
        wide = psi.astype(np.complex128)
        for j, t in enumerate(obs):
            q = G.pauli_string_apply_np(n_sites, t, psi, states=states).astype(np.complex128)
            s = np.sum(np.conj(wide) * q)
            assert s.real == np.rint(s.real)
            if C.is_zero(t, cplx, sector):
                assert s.real == 0.0 and got[j] == 0.0 and not np.signbit(got[j])
            else:
                assert got[j] == t[2] * float(s.real), (n_sites, n_down, j, t)
        assert np.count_nonzero(got) > len(obs) // 2


@pytest.mark.parametrize("n_sites,n_down", [(12, 6), (13, 4), (14, 7)])
def test_sector_fibres_give_the_rho_of_the_dense_generator(n_sites, n_down):
    n = n_sites
    for sites in ([n - 1], [0], [3, n - 1, 1], [0, n // 2, n // 2 - 1], [n - 1, 2, n // 2, 5, 1, n - 3], [0, 1, 2, 3, 4, 5]):
        for tid in ("d", "z", "s", "c"):
            psi = C.integer_state(math.comb(n_sites, n_down), C.TYPES[tid], 9)
            fib = C.sector_fibres(n_sites, n_down, sites, psi)
            rho, dense = G.reduced_density_matrix_np(n_sites, sites, psi, states=G.sector_states(n_sites, n_down))
            assert fib.dtype == psi.dtype and fib.shape[0] == 1 << len(sites) and fib.shape[1] <= min(psi.shape[0], dense.shape[1])
            assert np.count_nonzero(fib) == psi.shape[0] == np.count_nonzero(dense)
            assert np.array_equal(C.gram(fib), rho), (sites, tid)
            assert np.array_equal(C.gram(dense), rho)
            pc = np.array([bin(a).count("1") for a in range(1 << len(sites))])
            assert not np.any(C.gram(fib)[pc[:, None] != pc[None, :]])                     # exact zeros off the popcount diagonal


def test_full_fibres_are_those_of_the_dense_generator():
    for n_sites, sites in ((12, [11]), (12, [0, 11]), (13, [12, 1, 5, 3, 0]), (12, [9, 1, 11, 5, 3, 7])):
        psi = C.integer_state(1 << n_sites, np.complex64, 4)
        rho, dense = G.reduced_density_matrix_np(n_sites, sites, psi)
        assert np.array_equal(C.full_fibres(n_sites, sites, psi), dense) and np.array_equal(C.gram(dense), rho)
