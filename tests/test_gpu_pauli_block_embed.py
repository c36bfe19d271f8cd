"""A state between a ring's symmetry block and the full space or an S_z sector (ll_pauli_block_expand, ll_pauli_block_project;
csrc/pauli_block_embed.hip, planned by csrc/pauli_block_embed_plan.hpp), on rings of 4, 6, 7, 8 and 12 sites: every admitted
(momentum, parity, inversion, n_down) of the three block kinds, both target kinds where valid, all four storage types where the
block is real (the `_tids` rule of test_gpu_pauli_large.py), z and c otherwise.  References: the one-entry-per-row embeddings
(col, val) of generators.py.

The contract (include/lanczos_hip.h), with eps_d = 2^-52, eps_T the storage type's epsilon, |.| the modulus:
  expand, real character (2 m = 0 mod L)   got == (wide(c[col]) * val).astype(T): tolerance ZERO — one double product c * (+-1/sqrt R)
                                           and the storage rounding on both sides.
  expand, complex phases                   |got - ref| <= 16 eps_d |val c| + eps_T |ref|.  The constant: per component the kernel
                                           carries the factor 1/sqrt(R) (2 u, u = eps_d / 2), the scaling (u), the phase table entry
                                           (2 u), the product (u) and the sum of two (u): 7 u |val c|, sqrt(2) times that for the
                                           modulus, 10 u; numpy's val = phase / sqrt(R) and complex product carry 9 u of their own:
                                           19 u < 32 u = 16 eps_d.  eps_T |ref| covers the two storage roundings.  No n in it.
  project                                  |got - B^H psi| <= (2 (|G| + 8) + 8) eps_d sum_t |val(t) psi[t]| + eps_T |want|: the
                                           form of exact_ref.dot_bound over the |G| terms the kernel adds (their magnitudes sum to
                                           that of the orbit's terms), + 8 for the phase product, the factor sqrt(R) / |G| and its
                                           product and the reference's own double sum.
  empty rows of B                          exactly +0.0 in an output prefilled with NaN; out-of-sector states too.
Inputs and outputs in guarded NaN-padded device buffers at shifts 0 and 1 and on the host: the same bits, the input unchanged."""
import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
import pauli_block_embed_large_cases as C
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from pauli_cases import _cplx, _eps
from pauli_expect_block_cases import Block
from guarded import pattern
from test_gpu_accuracy_contracts import _guarded, _unguard
from test_gpu_pauli_expect import NAN_FILL, _refused

pytestmark = pytest.mark.gpu

RINGS = [4, 6, 7, 8, 12]
TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
EXPAND_CONST = 16.0


def _tids(block):
    return ("d", "z", "s", "c") if block.real_ok() else ("z", "c")


def _blocks(kind, n_sites, m, p=0, z=0):
    """Every admitted, non-empty block of the kind at this ring and momentum (symmetric: at this parity and inversion)."""
    out = []
    if kind == "momentum":
        for nd in range(n_sites + 1):
            if G.momentum_basis(n_sites, nd, m)[0].shape[0]:
                out.append(Block("momentum", n_sites, m, n_down=nd))
    elif kind == "momentum_full":
        out.append(Block("momentum_full", n_sites, m))
    else:
        nds = [None] + ([n_sites // 2] if n_sites % 2 == 0 else []) if z else [None] + list(range(n_sites + 1))
        for nd in nds:
            if G.symmetric_basis(n_sites, m, p, z, nd)[0].shape[0]:
                out.append(Block("symmetric", n_sites, m, p, z, nd))
    return out


def _targets(block):
    return [("full", block.n_sites)] + ([("sector", block.n_sites, block.n_down)] if block.sector else [])


def _kind_shape(block):
    if block.kind == "momentum":
        return "momentum", (block.n_sites, block.n_down, block.m)
    if block.kind == "momentum_full":
        return "momentum_full", (block.n_sites, block.m)
    return "symmetric", (block.n_sites, block.m, block.parity, block.inversion, block.n_down)


_TARGET_OPS = {}
_EMBED = {}


def _embedding(block, target):
    """C.embedding, computed once per block and target and left unchanged."""
    key = (block.id, target)
    if key not in _EMBED:
        _EMBED[key] = C.embedding(*_kind_shape(block), target)
        for a in _EMBED[key]:
            a.setflags(write=False)
    return _EMBED[key]


def _target_op(ctx, target, dtype):
    """One target operator per basis and storage type for the session (its terms play no part)."""
    key = (id(ctx), target, np.dtype(dtype).char)
    if key not in _TARGET_OPS:
        zz = [(0, 3 if target[1] > 1 else 1, 1.0)]
        _TARGET_OPS[key] = (L.PauliOperator(ctx, target[1], zz, dtype) if target[0] == "full" else
                            L.PauliSectorOperator(ctx, target[1], target[2], zz, dtype))
    return _TARGET_OPS[key]


def _everywhere(ctx, call, vec, n_out, what):
    """call(in, out) with `vec` and the output in guarded device buffers at shifts 0 and 1 — the output prefilled with NaN — and on
    the host: the same bits, the guards intact, the input unchanged.  Returns the result."""
    first = None
    for shift in (0, 1):
        ib, iv = _guarded(ctx, vec, shift, NAN_FILL)
        ob, ov = _guarded(ctx, pattern(n_out, vec.dtype, NAN_FILL), shift, NAN_FILL)
        assert call(iv, ov) is ov
        got = _unguard(ob, n_out, shift, NAN_FILL).copy()
        assert np.array_equal(_unguard(ib, vec.shape[0], shift, NAN_FILL), vec), (what, "the call changed its input")
        ib.free()
        ob.free()
        assert not np.any(np.isnan(got)), (what, "an element of the output was not written")
        if first is None:
            first = got
        assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "device", shift)
    host_in = vec.copy()
    got = call(host_in, None)
    assert got.dtype == vec.dtype and got.shape == (n_out,) and np.array_equal(host_in, vec)
    assert np.array_equal(first.view(np.uint8), got.view(np.uint8)), (what, "host buffers")
    return first


def _check_expand(block, got, col, val, c, dtype, what):
    ref = C.expand_np(col, val, c, dtype)
    empty = col < 0
    assert np.array_equal(got[empty].view(np.uint8), np.zeros(int(empty.sum()), got.dtype).view(np.uint8)), (what, "an empty row is not +0.0")
    if block.real_ok():
        assert np.array_equal(got, ref), (what, "expand, real character: not the numpy product bit for bit")
        return 0.0
    scale = np.abs(val) * np.abs(np.asarray(c).astype(np.complex128)[np.maximum(col, 0)])
    bound = EXPAND_CONST * E.EPS_D * scale + _eps(dtype) * np.abs(ref.astype(np.complex128))
    err = np.abs(got.astype(np.complex128) - ref.astype(np.complex128))
    assert np.all(err <= bound), (what, int(np.argmax(err - bound)))
    return float(np.max(err[~empty] / bound[~empty])) if np.any(~empty) else 0.0


def _project_bound(gsize, mag, want, dtype):
    return (2 * (gsize + 8) + 8) * E.EPS_D * mag + _eps(dtype) * np.abs(want) + 1e-300


def _check_block(ctx, block, tid):
    dtype = TYPES[tid]
    kind, shape = _kind_shape(block)
    gsize = C.group_size(kind, shape)
    op = block.create(L, ctx, dtype, block.hamiltonian())
    worst = [0.0, 0.0, 0.0]
    try:
        dim = op.n_local
        c = K.start_x(dim, dtype, seed=11)
        for target in _targets(block):
            top = _target_op(ctx, target, dtype)
            n = top.n_local
            col, val, _ = _embedding(block, target)
            what = (block.id, tid, target)
            assert col.shape[0] == n and int(col.max()) == dim - 1
            psi = _everywhere(ctx, lambda i, o: op.expand(i, top, out=o), c, n, what)
            worst[0] = max(worst[0], _check_expand(block, psi, col, val, c, dtype, what))
            # project: a random state that is NOT in the block
            rnd = K.start_x(n, dtype, seed=5)
            want, mag = C.project_np(col, val, rnd, dim)
            if not _cplx(dtype):
                assert np.all(np.abs(want.imag) <= 1e-12 * (mag + 1.0))
            got = _everywhere(ctx, lambda i, o: op.project(i, top, out=o), rnd, dim, what)
            err = np.abs(got.astype(np.complex128) - want)
            bound = _project_bound(gsize, mag, want, dtype)
            assert np.all(err <= bound), (what, "project", int(np.argmax(err - bound)))
            worst[1] = max(worst[1], float(np.max(err / bound)))
            # the round trip: the expanded state as stored carries (16 eps_d + eps_T) |val c| per element, which |B|^T sums to
            # that multiple of |c| (sum |val|^2 = 1), and the projection its own bound on sum |val| |val c| = |c|
            back = op.project(psi, top)
            cw = np.abs(c.astype(np.complex128))
            rt = (EXPAND_CONST * E.EPS_D + _eps(dtype)) * cw + _project_bound(gsize, cw, cw, dtype)
            err = np.abs(back.astype(np.complex128) - c.astype(np.complex128))
            assert np.all(err <= rt), (what, "round trip", int(np.argmax(err - rt)))
            worst[2] = max(worst[2], float(np.max(err / rt)))
    finally:
        op.close()
    return worst


CASES = ([(kind, n, m, 0, 0) for n in RINGS for kind in ("momentum", "momentum_full") for m in range(n)] +
         [("symmetric", n, m, p, z) for n in RINGS for m in range(n) for p in ((0, 1, -1) if (2 * m) % n == 0 else (0,))
          for z in (0, 1, -1)])


@pytest.mark.parametrize("kind,n_sites,m,p,z", CASES, ids=["%s-L%d-m%d-p%d-z%d" % c for c in CASES])
def test_every_block_of_the_ring(ctx, kind, n_sites, m, p, z):
    """(An empty block is refused at creation and has nothing to embed: a (momentum, parity, inversion) none of whose n_down has
    a representative runs no block.)"""
    blocks = _blocks(kind, n_sites, m, p, z)
    assert blocks or kind == "symmetric", "every momentum of a ring has a non-empty block of the two momentum kinds"
    worst = np.zeros(3)
    for block in blocks:
        for tid in _tids(block):
            worst = np.maximum(worst, _check_block(ctx, block, tid))
    print("worst error / bound (expand, project, round trip)", kind, n_sites, m, p, z, len(blocks), worst)


# ------------------------------------------------------------------ several trips of the grid-stride loops
@pytest.mark.parametrize("tid", list(TYPES))
def test_forced_block_sizes_give_the_same_bits(ctx, tid):
    """One index per workgroup block (the smallest value of the keys): at 12 sites 4096 units for expand against a grid of 2048 —
    two trips —, every other size in between; the results do not depend on it.  (A block of 12 sites holds fewer than 2048
    representatives: project's second trip is the large file's.)"""
    dtype = TYPES[tid]
    block = Block("symmetric", 12, 6 if tid in "ds" else 5, 0 if tid in "zc" else -1, -1)
    op = block.create(L, ctx, dtype, block.hamiltonian())
    top = _target_op(ctx, ("full", 12), dtype)
    try:
        assert C.expand_launch(top.n_local, 0) == (4096, 2048) and C.expand_launch(top.n_local) == (4, 4)
        c = K.start_x(op.n_local, dtype, seed=11)
        rnd = K.start_x(top.n_local, dtype, seed=5)
        base_e, base_p = op.expand(c, top), op.project(rnd, top)
        for bits in (0, 3, 7):
            ctx.set_tuning("pauli_block_expand_block_bits", str(bits))
            ctx.set_tuning("pauli_block_project_block_bits", str(bits))
            assert np.array_equal(op.expand(c, top).view(np.uint8), base_e.view(np.uint8)), bits
            assert np.array_equal(op.project(rnd, top).view(np.uint8), base_p.view(np.uint8)), bits
    finally:
        ctx.set_tuning("pauli_block_expand_block_bits", None)
        ctx.set_tuning("pauli_block_project_block_bits", None)
        op.close()


# ------------------------------------------------------------------ orthogonality of the blocks
def _orthogonal(a, b):
    """Different momenta; or, with both flags in use, different parities or different inversions."""
    return a.m != b.m or a.parity * b.parity == -1 or a.inversion * b.inversion == -1


@pytest.mark.parametrize("tid", ["z", "c"])
def test_a_state_of_one_block_has_no_weight_in_another(ctx, tid):
    """project(expand_A(c)) onto a block B orthogonal to A of the same ring is zero within project's bound (want = 0) plus the
    stored state's own error (16 eps_d + eps_T per element) pushed through |B|^T; and the weights ||project_m(psi)||^2 of a random
    psi over the eight momentum blocks of the full space sum to ||psi||^2 within what project's bound allows each coefficient."""
    dtype = TYPES[tid]
    n_sites = 8
    target = ("full", n_sites)
    top = _target_op(ctx, target, dtype)
    blocks = [Block("momentum_full", n_sites, m) for m in range(n_sites)] + [Block("symmetric", n_sites, 0, 1, 1),
                                                                            Block("symmetric", n_sites, 0, -1, 1),
                                                                            Block("symmetric", n_sites, 0, 1, -1),
                                                                            Block("symmetric", n_sites, 4, 1, -1),
                                                                            Block("momentum", n_sites, 3, n_down=4)]
    ops = [b.create(L, ctx, dtype, b.hamiltonian()) for b in blocks]
    try:
        pairs = 0
        for ba, opa in zip(blocks, ops):
            psi = opa.expand(K.start_x(opa.n_local, dtype, seed=3), top)
            for bb, opb in zip(blocks, ops):
                if not _orthogonal(ba, bb):
                    continue
                col, val, _ = _embedding(bb, target)
                rows = np.flatnonzero(col >= 0)
                mag = np.bincount(col[rows], weights=np.abs(val[rows]) * np.abs(psi.astype(np.complex128)[rows]), minlength=opb.n_local)
                got = opb.project(psi, top)
                gsize = C.group_size(*_kind_shape(bb))
                bound = _project_bound(gsize, mag, 0.0, dtype) + (EXPAND_CONST * E.EPS_D + _eps(dtype)) * mag
                assert np.all(np.abs(got) <= bound), (ba.id, bb.id, float(np.max(np.abs(got))))
                pairs += 1
        assert pairs >= 8 * 7 + 20
        rnd = K.start_x(top.n_local, dtype, seed=5)
        nn = float(np.sum(np.abs(rnd.astype(np.complex128)) ** 2))
        total, slack = 0.0, 4.0 * top.n_local * E.EPS_D * nn          # the host's own sums
        for b, opb in zip(blocks[:n_sites], ops[:n_sites]):
            col, val, _ = _embedding(b, target)
            want, mag = C.project_np(col, val, rnd, opb.n_local)
            cb = opb.project(rnd, top).astype(np.complex128)
            e = _project_bound(n_sites, mag, want, dtype)
            total += float(np.sum(np.abs(cb) ** 2))
            slack += float(np.sum(2.0 * np.abs(want) * e + e * e))
        assert abs(total - nn) <= slack, (total, nn, slack)
    finally:
        for o in ops:
            o.close()


# ------------------------------------------------------------------ no new tolerance: the full-space facilities on an expanded state
NO_NEW = [Block("momentum", 12, 4, n_down=6), Block("momentum_full", 12, 5), Block("symmetric", 12, 0, 1, 1),
          Block("symmetric", 12, 6, -1, -1, n_down=6)]


def _no_new(tids):
    cases = [(b, t) for b in NO_NEW for t in tids if t in _tids(b)]
    return dict(argnames="block,tid", argvalues=cases, ids=["%s-%s" % (b.id, t) for b, t in cases])


@pytest.mark.parametrize(**_no_new(["d", "z"]))
def test_expectation_of_the_expanded_state_is_the_blocks(ctx, block, tid):
    """target.expectation(expand(c), obs) against block.expectation(c, obs) at the sum of the two calls' existing bounds: the
    target's (test_gpu_pauli_expect: |coef| dot_bound(psi, P psi) + eps_d |want|, on the state it is given) and the block's
    (pauli_expect_block_cases.reference).  In d and z: the storage rounding of the expanded state is then one of the double
    roundings "that do not grow with the count" in the block's bound; the float types round Psi to eps_f, which neither covers."""
    from pauli_expect_block_cases import reference as block_reference

    dtype = TYPES[tid]
    op = block.create(L, ctx, dtype, block.hamiltonian())
    try:
        c, obs, _, bbound, _ = block_reference(block, dtype, op.n_local)
        states = block.states()
        for target in _targets(block):
            top = _target_op(ctx, target, dtype)
            psi = op.expand(c, top)
            tstates = states if target[0] == "sector" else None
            tb = np.zeros(len(obs))
            for j, t in enumerate(obs):
                q = G.pauli_string_apply_np(block.n_sites, t, psi, states=tstates)
                tb[j] = abs(t[2]) * E.dot_bound(psi, q) + E.EPS_D * abs(t[2] * E.dot_exact(psi, q).real)
            got_t, got_b = top.expectation(psi, obs), op.expectation(c, obs)
            assert np.all(np.abs(got_t - got_b) <= tb + bbound), (block.id, target, int(np.argmax(np.abs(got_t - got_b) - tb - bbound)))
    finally:
        op.close()


@pytest.mark.parametrize(**_no_new(list(TYPES)))
def test_reduced_density_matrix_of_a_block_state(ctx, block, tid):
    """block.reduced_density_matrix(c, sites, target) against generators.reduced_density_matrix_np of B c as expand stores it (the
    state test_every_block_of_the_ring holds to the expand contract), at test_gpu_pauli_rdm's bound: dot_bound of the two fibres
    plus one double rounding; the entropy follows."""
    from test_gpu_pauli_rdm import check_rho

    dtype = TYPES[tid]
    op = block.create(L, ctx, dtype, block.hamiltonian())
    try:
        c = K.start_x(op.n_local, dtype, seed=11)
        for target in _targets(block):
            top = _target_op(ctx, target, dtype)
            psi = op.expand(c, top)
            n_down = target[2] if target[0] == "sector" else None
            states = G.sector_states(block.n_sites, n_down) if n_down is not None else None
            for sites in ([0], [11, 3, 5], [1, 2, 3, 4, 5, 6]):
                _, fib = G.reduced_density_matrix_np(block.n_sites, sites, psi, states=states)
                dim = 1 << len(sites)
                want, bound = np.zeros((dim, dim), np.complex128), np.zeros((dim, dim))
                for a in range(dim):
                    for ap in range(a, dim):
                        if n_down is not None and bin(a).count("1") != bin(ap).count("1"):
                            continue
                        w = complex(E.dot_exact(fib[ap], fib[a]))
                        want[a, ap], want[ap, a] = w, w.conjugate()
                        bound[a, ap] = bound[ap, a] = E.dot_bound(fib[ap], fib[a]) + E.EPS_D * max(abs(w.real), abs(w.imag))
                got, nsw = op.reduced_density_matrix(c, sites, top, return_sweeps=True)
                assert nsw == 1
                check_rho(got, want, bound, dtype, n_down, (block.id, tid, target, sites))
                s = L.entanglement_entropy(got)
                assert 0.0 <= s <= len(sites) * np.log(2.0) + 1e-12
    finally:
        op.close()


@pytest.mark.parametrize(**_no_new(["z", "c"]))
def test_the_targets_hamiltonian_on_the_expanded_state(ctx, block, tid):
    """H_target expand(c) against expand(H_block c), at the embedding bound of test_gpu_pauli_symmetric section 4, read in the
    target's basis: the big apply's class bound on the stored X with the rounding of its input (4 eps_T sum |a||x|), plus the
    block apply's class bound carried by |val| to the row of its column, plus expand's own contract on val y."""
    from pauli_cases import _apply, _class_bound

    dtype = TYPES[tid]
    eps = _eps(dtype)
    terms = block.hamiltonian()
    kind, shape = _kind_shape(block)
    if kind == "momentum":
        csr = G.pauli_momentum_csr(*shape, terms, np.complex128, merge=False)
    elif kind == "momentum_full":
        csr = G.pauli_momentum_full_csr(*shape, terms, np.complex128, merge=False)
    else:
        csr = G.pauli_symmetric_csr(shape[0], shape[1], shape[2], shape[3], terms, np.complex128, n_down=shape[4], merge=False)
    op = block.create(L, ctx, dtype, terms)
    try:
        x = K.start_x(op.n_local, dtype)
        ex = E.rows_exact(csr, x)
        y, _ = _apply(ctx, op, x, 0, 0.0, False)
        cls, _ = _class_bound(dtype, x, ex, y, 0.0)
        for target in _targets(block):
            if target[0] == "full":
                big = L.PauliOperator(ctx, block.n_sites, terms, dtype)
                big_csr = G.pauli_csr(block.n_sites, terms, np.complex128, merge=False)
            else:
                big = L.PauliSectorOperator(ctx, block.n_sites, target[2], terms, dtype)
                big_csr = G.pauli_sector_csr(block.n_sites, target[2], terms, np.complex128, merge=False)
            try:
                col, val, _ = _embedding(block, target)
                X = op.expand(x, big)
                Y, _ = _apply(ctx, big, X, 0, 0.0, False)
                Z = op.expand(y, big)
            finally:
                big.close()
            big_ex = E.rows_exact(big_csr, X)
            big_cls = E.componentwise_bound(big_ex, eps) + eps * E.abs1(Y) + 4 * eps * big_ex.absrow
            k = np.maximum(col, 0)
            inb = col >= 0
            carried = np.where(inb, E.abs1(val) * cls[k], 0.0)
            own = np.where(inb, (EXPAND_CONST * E.EPS_D + eps) * np.abs(val) * np.abs(y.astype(np.complex128)[k]), 0.0)
            bound = big_cls + carried + own + 1e-300
            ok, r = E.within(E.part_errors(Y, Z), (bound, bound))
            assert ok, (block.id, tid, target, r)
            assert np.any(Y != 0)
            print("H_target expand(c) against expand(H_block c): error / bound", block.id, tid, target, r)
    finally:
        op.close()


# ------------------------------------------------------------------ refusals, each with its message
def test_refusals(ctx):
    n_sites = 6
    ring = G.heisenberg_terms(n_sites, 1.0, 0.8, periodic=True)
    tf = G.tfim_terms(n_sites, 1.0, 0.7, periodic=True)
    one = [(0, 3, 1.0)]
    csr = L.CsrOperator(ctx, *G.laplace2d_np(4))
    full = L.PauliOperator(ctx, n_sites, one, np.float64)
    full8 = L.PauliOperator(ctx, 8, one, np.float64)
    fullz = L.PauliOperator(ctx, n_sites, one, np.complex128)
    fulls = L.PauliOperator(ctx, n_sites, one, np.float32)
    sect3 = L.PauliSectorOperator(ctx, n_sites, 3, one, np.float64)
    sect2 = L.PauliSectorOperator(ctx, n_sites, 2, one, np.float64)
    mom = L.PauliMomentumOperator(ctx, n_sites, 3, 0, ring, np.float64)
    mf = L.PauliMomentumFullOperator(ctx, n_sites, 0, tf, np.float64)
    symf = L.PauliSymmetricOperator(ctx, n_sites, 0, tf, np.float64, parity=1)
    syms = L.PauliSymmetricOperator(ctx, n_sites, 0, ring, np.float64, parity=1, n_down=3)
    ctx2 = L.Context(0)
    ctx2.init_comm(L.Context.unique_id(), 0, 1)
    shard_b = L.PauliMomentumFullOperator(ctx2, n_sites, 0, tf, np.float64)
    shard_t = L.PauliOperator(ctx2, n_sites, one, np.float64)
    c = K.start_x(mf.n_local, np.float64)
    psi = K.start_x(64, np.float64)
    lib = capi.lib()
    try:
        for call in (L.pauli_block_expand, L.pauli_block_project):
            def no(block, target, *needles):
                n_in = block.n_local if call is L.pauli_block_expand else target.n_local
                _refused(lambda: call(block, K.start_x(n_in, block.dtype), target), *needles)

            no(csr, full, "the block operator is a CSR operator")
            no(full, full, "the block operator is a full-space sum of Pauli strings")
            no(sect3, full, "the block operator is a sum of Pauli strings on an S_z sector")
            no(mf, csr, "the target operator is a CSR operator")
            no(mf, mf, "the target operator is a momentum block of the full space")
            no(mf, symf, "the target operator is a momentum / reflection / spin-inversion block")
            no(mom, mom, "the target operator is a momentum block of an S_z sector")
            no(mf, full8, "n_sites")
            no(mf, fullz, "storage type")
            no(mf, fulls, "storage type")
            no(mf, sect3, "a full-space block does not fit an S_z-sector target")
            no(symf, sect3, "a full-space block does not fit an S_z-sector target")
            no(mom, sect2, "n_down")
            no(syms, sect2, "n_down")
            no(shard_b, shard_t, "a context with a communicator")
            no(mf, shard_t, "the target operator belongs to another context")
            no(shard_b, full, "the target operator belongs to another context")
        # the C entry points: null arguments, another context, overlapping buffers
        out = np.zeros(64)
        for fn, a, b in ((lib.ll_pauli_block_expand, c, out), (lib.ll_pauli_block_project, psi, np.zeros(mf.n_local))):
            for args in ((None, mf.handle, full.handle, capi.ptr(a), capi.ptr(b)), (ctx.handle, None, full.handle, capi.ptr(a), capi.ptr(b)),
                         (ctx.handle, mf.handle, None, capi.ptr(a), capi.ptr(b)), (ctx.handle, mf.handle, full.handle, None, capi.ptr(b)),
                         (ctx.handle, mf.handle, full.handle, capi.ptr(a), None)):
                assert fn(*args) == capi.LL_ERR_INVALID and b"null argument" in lib.ll_last_error()
            assert fn(ctx2.handle, mf.handle, full.handle, capi.ptr(a), capi.ptr(b)) == capi.LL_ERR_INVALID
            assert b"the block operator belongs to another context" in lib.ll_last_error()
        both = np.zeros(64 + mf.n_local)
        tail = both[64 - 1:]                                     # its first element is the last of the 64
        assert lib.ll_pauli_block_expand(ctx.handle, mf.handle, full.handle, capi.ptr(tail), capi.ptr(both)) == capi.LL_ERR_INVALID
        assert b"input and output overlap" in lib.ll_last_error()
        assert lib.ll_pauli_block_project(ctx.handle, mf.handle, full.handle, capi.ptr(both), capi.ptr(tail)) == capi.LL_ERR_INVALID
        assert b"input and output overlap" in lib.ll_last_error()
        assert lib.ll_pauli_block_expand(ctx.handle, mf.handle, full.handle, capi.ptr(both), capi.ptr(both)) == capi.LL_ERR_INVALID
        assert b"input and output overlap" in lib.ll_last_error()
        dev = ctx.to_device(np.zeros(64 + mf.n_local))
        import types
        inside = types.SimpleNamespace(ptr=dev.ptr + 8 * 60, dtype=np.dtype(np.float64), shape=(mf.n_local,))
        _refused(lambda: mf.expand(inside, full, out=dev), "input and output overlap")
        dev.free()
        # the wrappers' own checks, and the operators still work after the refusals
        with pytest.raises(ValueError):
            mf.expand(c[:-1], full)
        with pytest.raises(TypeError):
            mf.expand(c, full, out=np.zeros(64, np.float32))
        got = mf.project(mf.expand(c, full), full)
        assert np.max(np.abs(got - c)) <= 64 * E.EPS_D
    finally:
        for o in (csr, full, full8, fullz, fulls, sect3, sect2, mom, mf, symf, syms, shard_b, shard_t):
            o.close()
        ctx2.close()
