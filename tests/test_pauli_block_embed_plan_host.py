"""lambda-lanczos_amd/csrc/pauli_block_embed_plan.hpp — the host planning of ll_pauli_block_expand / ll_pauli_block_project — on the
CPU: the program tests/cpp/pauli_block_embed_plan_test.cpp checks the block / target compatibility rule over every combination,
the factor tables and the launch geometry (plain and with the address and undefined-behaviour sanitizers, as ordinary child
processes), and answers questions, through which this file compares the header with numpy (1 / np.sqrt(R), np.sqrt(R) / |G|) and
with the Python restatement of the launch rule in tests/pauli_block_embed_large_cases.py.  Also: the tabulated (units, grid) of
the large cases and their trip counts, and the host references of the large file against the dense embeddings on small rings."""
import math
import os
import subprocess

import numpy as np
import pytest

import pauli_block_embed_large_cases as C
import pauli_measure_large_cases as M
from lambda_lanczos_amd import generators as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pauli_block_embed_plan_test.cpp")
ROLES = {"other": 0, "full": 1, "sector": 2, "momentum": 3, "momentum_full": 4, "symmetric": 5}   # PauliEmbedRole


def _build(tmp_path, extra=()):
    exe = str(tmp_path / "pauli_block_embed_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "lambda-lanczos_amd", "csrc")] + list(extra) +
                   [SRC, "-o", exe], check=True)
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe, "ask"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_pauli_block_embed_plan_properties(tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    assert " 0 failures" in r.stdout


def test_the_compatibility_rule_over_every_combination(tmp_path):
    """Restated: same n_sites and storage type; a sector target takes a sector block (momentum, or symmetric with n_down >= 0) of
    its own n_down; a full-space target takes every block."""
    exe = _build(tmp_path)
    lines, want = [], []
    blocks = ([("momentum", d) for d in range(0, 5)] + [("momentum_full", -1)] + [("symmetric", d) for d in range(-1, 5)])
    targets = [("full", -1)] + [("sector", d) for d in range(0, 5)]
    for bk, bd in blocks:
        for tk, td in targets:
            for tn in (4, 6):
                for teb, tcx in ((8, 0), (8, 1), (4, 0), (16, 1)):
                    lines.append("fault %d 4 %d 8 0 %d %d %d %d %d" % (ROLES[bk], bd, ROLES[tk], tn, td, teb, tcx))
                    ok = tn == 4 and (teb, tcx) == (8, 0) and (tk == "full" or (bd >= 0 and bd == td))
                    want.append(ok)
    for role in ("other", "full", "sector"):
        lines.append("fault %d 4 -1 8 0 %d 4 -1 8 0" % (ROLES[role], ROLES["full"]))
        want.append(False)
    for role in ("other", "momentum", "momentum_full", "symmetric"):
        lines.append("fault %d 4 -1 8 0 %d 4 -1 8 0" % (ROLES["momentum_full"], ROLES[role]))
        want.append(False)
    got = _ask(exe, lines)
    for ln, g, w in zip(lines, got, want):
        assert (g == "ok") == w, (ln, g)
        assert g == "ok" or len(g) > 10       # a refusal names its cause
    assert sum(want) == 12 + 5 + 5            # full target: all 12 blocks; sector targets: the momentum and the symmetric block of their n_down


def test_the_factor_tables_are_those_of_numpy(tmp_path):
    exe = _build(tmp_path)
    groups = [1, 4, 7, 8, 12, 14, 24, 28, 30, 48, 60, 120]
    out = _ask(exe, ["expand_factors"] + ["project_factors %d" % g for g in groups])
    R = np.arange(1, 121, dtype=np.float64)
    ef = np.array([float.fromhex(v) for v in out[0].split()])
    assert ef.shape == (121,) and ef[0] == 0.0 and np.array_equal(ef[1:], 1.0 / np.sqrt(R))
    for g, line in zip(groups, out[1:]):
        pf = np.array([float.fromhex(v) for v in line.split()])
        assert pf.shape == (121,) and pf[0] == 0.0
        assert np.array_equal(pf[1:g + 1], np.sqrt(R[:g]) / float(g)) and not np.any(pf[g + 1:])


def test_the_restated_launch_rule_is_the_headers_and_the_tabulated_cases_hold(tmp_path):
    exe = _build(tmp_path)
    lines, want = [], []
    for case in C.CASES:
        kind, shape, target, eb, pb, e_launch, p_launch = case
        n, dim = C.target_dim(target), C.block_dim(kind, shape)
        assert C.expand_launch(n, eb) == e_launch and C.project_launch(dim, pb) == p_launch, case
        for count, forced, dflt in ((n, eb, C.EXPAND_BITS), (n, None, C.EXPAND_BITS), (dim, pb, C.PROJECT_BITS), (dim, None, C.PROJECT_BITS)):
            lines.append("launch %d %d %d %d" % (count, -1 if forced is None else forced, dflt, C.MAX_GRID))
            want.append(C.launch(count, forced, dflt))
    for count in (1, 255, 256, 257, 1 << 30):      # the small file's sizes and the largest target
        for forced in (None, 0, 3, 40):
            lines.append("launch %d %d %d %d" % (count, -1 if forced is None else forced, C.PROJECT_BITS, C.MAX_GRID))
            want.append(C.launch(count, forced, C.PROJECT_BITS))
    for ln, g, w in zip(lines, _ask(exe, lines), want):
        bits, units, grid = (int(v) for v in g.split())
        assert (units, grid) == w, (ln, g, w)
    assert C.expand_launch(1 << 30) == (1 << 20, 2048)


def test_every_large_case_wraps():
    """Every case gives both kernels two or more trips; with a sector target expand's last trip is ragged, project's always is
    but where the units happen to be a multiple of the grid; every expand form (three block kinds, two target kinds where valid)
    and both project forms have a ragged case."""
    ragged = set()
    for kind, shape, target, _, _, (eu, eg), (pu, pg) in C.CASES:
        assert eg == pg == C.MAX_GRID and eu > eg and pu > pg, (kind, shape)
        if target[0] == "sector":
            assert eu % eg != 0
        else:
            assert eu % eg == 0 and eu // eg >= 2          # 2^n_sites states: whole trips only
        if eu % eg:
            ragged.add(("expand", kind, target[0]))
        if pu % pg:
            ragged.add(("project", target[0]))
    assert {("expand", "momentum", "sector"), ("expand", "symmetric", "sector"), ("project", "sector"), ("project", "full")} <= ragged
    dims = {(k, s): C.block_dim(k, s) for k, s, *_ in C.CASES}
    assert dims[("momentum", (30, 5, 7))] == 4750 and dims[("symmetric", (22, 0, 1, 1, 11))] == 8359
    assert math.comb(30, 5) == 142506 and max(C.target_dim(c[2]) for c in C.CASES) == 1 << 21
    assert M.exact_condition(120 * (1 << 21))              # project's integer sums stay below 2^53


@pytest.mark.parametrize("kind,shape,target", [
    ("momentum", (8, 4, 0), ("sector", 8, 4)), ("momentum", (8, 4, 4), ("full", 8)), ("momentum", (6, 3, 2), ("sector", 6, 3)),
    ("momentum_full", (8, 4), ("full", 8)), ("momentum_full", (7, 3), ("full", 7)),
    ("symmetric", (8, 0, 1, 1, None), ("full", 8)), ("symmetric", (8, 4, -1, -1, 4), ("full", 8)),
    ("symmetric", (8, 4, -1, -1, 4), ("sector", 8, 4)), ("symmetric", (6, 2, 0, 1, None), ("full", 6)),
])
def test_the_large_files_references_against_the_dense_embeddings(kind, shape, target):
    """embedding(), expand_np, project_np and project_integer_np of the large cases against the dense B of generators.py."""
    if kind == "momentum":
        B = G.momentum_embedding(*shape)
        n_down = shape[1]
    elif kind == "momentum_full":
        B = G.full_momentum_embedding(*shape)
        n_down = None
    else:
        B = G.symmetric_embedding(shape[0], shape[1], shape[2], shape[3], shape[4])
        n_down = shape[4]
    if target[0] == "full" and n_down is not None:
        full = np.zeros((1 << shape[0], B.shape[1]), np.complex128)
        full[G.sector_states(shape[0], n_down).astype(np.int64)] = B
        B = full
    n, dim = B.shape
    assert n == C.target_dim(target)
    col, val, R = C.embedding(kind, shape, target)
    dense = np.zeros_like(B)
    dense[np.flatnonzero(col >= 0), col[col >= 0]] = val[col >= 0]
    assert np.array_equal(dense, B)
    assert np.allclose(np.abs(val[col >= 0]) ** 2 * R[col >= 0], 1.0, rtol=0, atol=1e-15)
    real = C.real_character(kind, shape)
    for tid in C.tids(kind, shape):
        dtype = M.TYPES[tid]
        c = M.integer_state(dim, dtype, 3)
        want = B @ c.astype(np.complex128)
        got = C.expand_np(col, val, c, dtype)
        assert got.dtype == np.dtype(dtype) and np.allclose(got, want, rtol=1e-6 if tid in "sc" else 1e-14, atol=0)
        psi = M.integer_state(n, dtype, 4)
        ref = B.conj().T @ psi.astype(np.complex128)
        out, mag = C.project_np(col, val, psi, dim)
        assert np.allclose(out, ref, rtol=0, atol=1e-12) and np.all(mag >= np.abs(out) - 1e-12)
        if real:
            exact = C.project_integer_np(col, val, R, psi, dim, kind, shape, dtype)
            assert np.allclose(exact, ref, rtol=1e-6 if tid in "sc" else 1e-14, atol=1e-12)   # (an exact 0 against the rounding of B^H psi)
