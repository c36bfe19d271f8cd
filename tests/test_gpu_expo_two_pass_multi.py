"""Several times from one Krylov space (ll_expo_two_pass_multi, csrc/expo_two_pass_multi_run.cpp; ll_recur_accum_multi,
recur_accum_multi_kernel in csrc/recur.hip).  The acceptance property is bit identity: the replayed step with several accumulators
gives every accumulator the bytes the single step gives it alone, and on a device operator every (output, iteration count) of the
multi-time run is, byte for byte, what run_two_pass returns for that time alone.  The single forms are held to exact arithmetic and
to the oracle by tests/test_gpu_two_pass.py and tests/test_gpu_expo_two_pass.py, so their bounds carry over; one case is checked
against the oracle directly.  Then the buffer conventions, the edges and the refusals."""
import numpy as np
import pytest

import contract_cases as K
import lambda_lanczos_amd as L
from guarded import guarded as _guarded, unguard as _unguard
from lambda_lanczos_amd import _capi as capi
from lambda_lanczos_amd import generators as G
from util import overlap

pytestmark = pytest.mark.gpu

TYPES = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}
EPS = np.finfo(np.float64).eps


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


# ------------------------------------------------------------------ 1. the replayed step with several accumulators: bit identity
@pytest.mark.parametrize("with_p", [True, False], ids=["p", "nop"])
@pytest.mark.parametrize("tid", list(TYPES))
def test_recur_accum_multi_gives_every_accumulator_the_single_step_s_bytes(ctx, tid, with_p):
    """y' and psi_j' from one ll_recur_accum_multi call against, for each j, L.recur_accum on a fresh copy of y with g_j and psi_j:
    equal as bytes; x and p unchanged; every guard intact.  Sizes: one element, less than a lane, a lane short of one, around 2048,
    three strips and a ragged end; 1, 2, 3, 5 and 16 accumulators (every remainder of the kernel's batches of two, and the full
    list); pointer shifts 0 and 1 (the second breaks the 16-byte alignment)."""
    dtype = np.dtype(TYPES[tid])
    cplx = dtype.kind == "c"
    ept = 64 // dtype.itemsize
    elems = 256 * ept
    a, b = -1.7, 0.3
    rng = np.random.default_rng(5)
    gs = [complex(rng.uniform(-1, 1), rng.uniform(-1, 1)) if cplx else float(rng.uniform(-1, 1)) for _ in range(16)]
    for n in [1, 7, ept - 1, 2047, 2048, 2049, 3 * elems + 5]:
        y, x, p = (K.start_x(n, dtype, s) for s in (41, 42, 43))
        psis = [K.start_x(n, dtype, 100 + j) for j in range(16)]
        for shift in (0, 1):
            xb, xv = _guarded(ctx, x, shift)
            pb, pv = _guarded(ctx, p, shift)
            # the single step, once per accumulator (shared by every accumulator count below)
            want_q, want_y = [], None
            for j in range(16):
                yb, yv = _guarded(ctx, y, shift)
                qb, qv = _guarded(ctx, psis[j], shift)
                L.recur_accum(ctx, yv, xv, pv if with_p else None, a, b, gs[j] if cplx else np.float64(gs[j]), qv, n)
                want_q.append(_unguard(qb, n, shift))
                got_y = _unguard(yb, n, shift)
                assert want_y is None or _same(got_y, want_y)
                want_y = got_y
                yb.free()
                qb.free()
            for n_acc in (1, 2, 3, 5, 16):
                yb, yv = _guarded(ctx, y, shift)
                qs = [_guarded(ctx, psis[j], shift) for j in range(n_acc)]
                L.recur_accum_multi(ctx, yv, xv, pv if with_p else None, a, b, gs[:n_acc], [q[1] for q in qs], n)
                assert _same(_unguard(yb, n, shift), want_y), (n, shift, n_acc)
                for j in range(n_acc):
                    assert _same(_unguard(qs[j][0], n, shift), want_q[j]), (n, shift, n_acc, j)
                    assert not np.array_equal(want_q[j], psis[j])
                yb.free()
                for q in qs:
                    q[0].free()
            assert np.array_equal(_unguard(xb, n, shift), x) and np.array_equal(_unguard(pb, n, shift), p)
            xb.free()
            pb.free()


# ------------------------------------------------------------------ 2. the solver: bit identity with the single-time call
TFIM = (10, G.tfim_terms(10, 1.0, 1.5, periodic=True))
SECTOR = (12, 6, G.heisenberg_terms(12))
TFIM_TIMES = [-0.5j, 0j, -1.5j, -0.1j]
TFIM_M = [22, 2, 40, 11]   # the reference's rule (EX:124-158) at eps = 1e2 eps_double on this ring and start vector, in double


def _tfim(ctx, dtype):
    return L.PauliOperator(ctx, TFIM[0], TFIM[1], dtype), 1024, G.start_vector(1024, 1, np.complex128).astype(dtype)


def _sector(ctx, dtype):
    op = L.PauliSectorOperator(ctx, SECTOR[0], SECTOR[1], SECTOR[2], dtype)
    return op, 924, G.start_vector(924, 1, np.complex128).astype(dtype)


def _laplace(ctx, dtype):
    rp, ci, va = G.laplace2d(40)
    return L.CsrOperator(ctx, rp, ci, va.astype(dtype)), 1600, G.start_vector(1600, 1).astype(dtype)


def _multi_and_singles(ctx, make, dtype, times, max_it=None):
    """((outputs, m_j, stats) of one multi call, [(output, m) of run_two_pass(a_j)]) on one operator, host buffers."""
    op, n, inp = make(ctx, dtype)
    try:
        ex = L.Exponentiator(op, n)
        if max_it is not None:
            ex.max_iteration = max_it
        outs, ms = ex.run_two_pass_multi(times, inp)
        stats = ex.last_stats
        singles = [ex.run_two_pass(a, inp) for a in times]
    finally:
        op.close()
    return (outs, ms, stats), singles, ex.eps


def _assert_identical(multi, singles):
    outs, ms, stats = multi
    print("m_j:", ms, " single runs:", [it for _, it in singles], " replay mismatches:", stats["replay_mismatches"])
    assert len(outs) == len(singles) and len(ms) == len(singles)
    for j, (ref, it) in enumerate(singles):
        assert ms[j] == it, (j, ms, it)
        assert _same(outs[j], ref), j
    assert stats["total_iterations"] == max(ms) and stats["n_passes"] == 1
    assert stats["replay_mismatches"] == 0


@pytest.mark.parametrize("tid", ["z", "c"])
def test_tfim_four_unsorted_times_equal_the_single_runs_byte_for_byte(ctx, tid):
    multi, singles, _ = _multi_and_singles(ctx, _tfim, TYPES[tid], TFIM_TIMES)
    ms = multi[1]
    if tid == "z":
        assert all(abs(m - want) <= 1 for m, want in zip(ms, TFIM_M)), ms
        assert len(set(ms)) == 4          # accumulators retire at four different iterations
    else:
        assert len(set(ms)) >= 2
    _assert_identical(multi, singles)


@pytest.mark.parametrize("tid", ["z", "c"])
def test_heisenberg_sector_two_times_equal_the_single_runs_byte_for_byte(ctx, tid):
    multi, singles, _ = _multi_and_singles(ctx, _sector, TYPES[tid], [-0.05j, -0.6j])
    _assert_identical(multi, singles)


@pytest.mark.parametrize("tid", ["d", "s"])
def test_real_times_end_at_max_iteration_and_equal_the_single_runs(ctx, tid):
    """With real a the overlap test never fires: every time runs to max_iteration = 40 and no accumulator retires early."""
    multi, singles, _ = _multi_and_singles(ctx, _laplace, TYPES[tid], [-0.5, -0.1], max_it=40)
    assert multi[1] == [40, 40]
    _assert_identical(multi, singles)


# ------------------------------------------------------------------ 3. against the oracle
def test_tfim_outputs_against_the_oracle(ctx, oracle):
    """Each output against oracle.expo(csr, a_j, input, eps = the run's) by the double rule of tests/test_gpu_expo_two_pass.py:
    max|out - o_out| <= 1e-10 ||o_out||, | ||out|| / ||in|| - 1 | <= 1e-12, 1 - overlap <= 10 eps."""
    csr = G.pauli_csr(TFIM[0], TFIM[1], np.complex128)
    (outs, ms, _), _, eps = _multi_and_singles(ctx, _tfim, np.complex128, TFIM_TIMES)
    inp = G.start_vector(1024, 1, np.complex128)
    in_norm = float(np.linalg.norm(inp))
    for a, out, m in zip(TFIM_TIMES, outs, ms):
        o_out, o_it, _ = oracle.expo(csr, a, inp, eps=eps)
        o_norm = float(np.linalg.norm(o_out))
        err = float(np.max(np.abs(out - o_out)))
        norm_err = abs(float(np.linalg.norm(out)) / in_norm - 1)
        miss = 1 - overlap(out, o_out)
        print("a = %s: m = %d (oracle %d), max|out - oracle| / |oracle| %.3e, | |out| / |in| - 1 | %.3e, 1 - overlap %.3e"
              % (a, m, o_it, err / o_norm, norm_err, miss))
        assert abs(m - o_it) <= 1
        assert err <= 1e-10 * o_norm
        assert norm_err <= 1e-12
        assert miss <= 10 * eps


# ------------------------------------------------------------------ 4. buffers and memory
def _tfim_buffers(ctx, inp, where):
    """One multi run on a fresh TFIM operator with TFIM_TIMES; where: 'host', 'device', 'mixed' (outputs 0 and 2 on the device, 1 and
    3 host arrays) or 'inplace' (device, output 2 is the input's buffer).  Returns ([outputs as host arrays], m_j, stats, the input
    buffer read back or None when it was an output)."""
    op = L.PauliOperator(ctx, TFIM[0], TFIM[1], np.complex128)
    ex = L.Exponentiator(op, 1024)
    try:
        if where == "host":
            outs, ms = ex.run_two_pass_multi(TFIM_TIMES, inp)
            return outs, ms, ex.last_stats, inp
        d_in = ctx.to_device(inp)
        on_device = {"device": (0, 1, 2, 3), "mixed": (0, 2), "inplace": (0, 1, 2, 3)}[where]
        bufs = [ctx.empty(1024, np.complex128) if j in on_device else None for j in range(4)]
        if where == "inplace":
            bufs[2].free()
            bufs[2] = d_in
        got, ms = ex.run_two_pass_multi(TFIM_TIMES, d_in, out=bufs)
        assert all(got[j] is bufs[j] for j in on_device)
        outs = [g.get() if isinstance(g, L.DeviceArray) else g for g in got]
        in_after = None if where == "inplace" else d_in.get()
        for buf in bufs + [d_in]:
            if buf is not None:
                buf.free()   # (freeing the shared buffer of 'inplace' twice is harmless)
        return outs, ms, ex.last_stats, in_after
    finally:
        op.close()


def test_workspace_counts_and_device_buffers_change_no_bit(ctx, llenv):
    inp = G.start_vector(1024, 1, np.complex128)
    keep = inp.copy()
    host, ms, stats, _ = _tfim_buffers(ctx, inp, "host")
    assert stats["workspace_vectors"] == 3 + 4 and stats["replay_mismatches"] == 0 and np.array_equal(inp, keep)
    expect = {"host": 7, "device": 3, "mixed": 3 + 2, "inplace": 3}
    for fill in (None, 0xFF, 0x7F):   # then on poisoned workspace (tests/test_gpu_poisoned_workspace.py): NaN in every type, huge
        if fill is not None:
            llenv.setenv("LL_TEST_WORKSPACE_FILL", str(fill))
        for where in ("host", "device", "mixed", "inplace"):
            outs, ms_w, stats_w, in_after = _tfim_buffers(ctx, inp, where)
            assert stats_w["workspace_vectors"] == expect[where], (fill, where)
            assert ms_w == ms and stats_w["replay_mismatches"] == 0, (fill, where)
            for j in range(4):
                assert _same(outs[j], host[j]), (fill, where, j)
            if in_after is not None:
                assert np.array_equal(_bits(in_after), _bits(keep)), (fill, where)   # a distinct input buffer is unchanged
    llenv.delenv("LL_TEST_WORKSPACE_FILL")


# ------------------------------------------------------------------ 5. edges
def test_input_that_is_an_eigenvector_takes_one_iteration_for_every_time(ctx):
    """||in|| = 2 and lambda = 8: alpha_0 and the update are exact, r_1 = 0, breakdown after one iteration ends every time: all
    m_j = 1, no replay, out_j = exp(a_j lambda) in.  What remains is the exponential in double (2 units of roundoff) and the product
    g_0 r_0 (2 sqrt(2) units): below 4 eps, relative."""
    n = 50
    op = L.CsrOperator(ctx, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.arange(1.0, n + 1.0).astype(np.complex128))
    inp = np.zeros(n, dtype=np.complex128)
    inp[7] = -2j
    times = [-0.25j, -1j, 0.125j]
    ex = L.Exponentiator(op, n)
    outs, ms = ex.run_two_pass_multi(times, inp)
    op.close()
    assert ms == [1, 1, 1] and ex.last_stats["total_iterations"] == 1 and ex.last_stats["replay_mismatches"] == 0
    for a, out in zip(times, outs):
        exact = complex(np.exp(np.clongdouble(8 * a)) * np.clongdouble(inp[7]))
        assert abs(out[7] - exact) <= 4 * EPS * abs(exact)
        assert np.all(np.delete(out, 7) == 0)


def test_one_time_equals_run_two_pass(ctx):
    multi, singles, _ = _multi_and_singles(ctx, _tfim, np.complex128, [-0.5j])
    _assert_identical(multi, singles)
    assert multi[2]["workspace_vectors"] == 4


def test_sixteen_copies_of_one_time_give_sixteen_identical_outputs(ctx):
    multi, singles, _ = _multi_and_singles(ctx, _tfim, np.complex128, [-0.5j] * 16)
    _assert_identical(multi, singles)
    assert len(set(multi[1])) == 1 and all(_same(out, multi[0][0]) for out in multi[0])


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ctx):
    op, n, inp = _tfim(ctx, np.complex128)
    ex = L.Exponentiator(op, n)

    def refused(times, input=inp, out=None, word=None):
        with pytest.raises(capi.LanczosHipError) as e:
            ex.run_two_pass_multi(times, input, out=out)
        assert e.value.code == capi.LL_ERR_INVALID
        assert word is None or word in str(e.value), str(e.value)

    try:
        refused([])
        refused([-0.1j] * 17)
        d_in, d_out = ctx.to_device(inp), ctx.empty(n, np.complex128)
        refused([-0.1j, -0.2j], input=d_in, out=[d_out, d_out], word="overlap")
        d_in.free()
        d_out.free()
        refused([-0.1j], input=np.zeros(n, dtype=np.complex128), word="zero")
        ex.full_orthogonalize = True
        refused([-0.1j], word="full_orthogonalize")
    finally:
        op.close()
    rop, rn, rinp = _laplace(ctx, np.float64)
    try:
        ex = L.Exponentiator(rop, rn)
        refused([-0.5, -0.5j], input=rinp, word="a_im")
    finally:
        rop.close()
