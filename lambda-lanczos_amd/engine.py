"""Host-side mirror of the reference's public interface for the Krylov hot path, on top of the C ABI.

``LambdaLanczos`` / ``Exponentiator`` keep the reference's names, constructor shapes, public fields, defaults and
return conventions (include/lambda_lanczos/lambda_lanczos.hpp:109-415, exponentiator.hpp:24-211) so that the parity
tests read like the reference's own tests; the C++ twin of this file is include/lambda_lanczos_hip/*.hpp.
All numerics run in liblanczos_hip.so on the GPU — there is no CPU path in this package.
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi as capi
from ._capi import check, lib, ptr

_EPS = float(np.finfo(np.float64).eps)


def _suffix(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return "d"
    if dtype == np.complex128:
        return "z"
    if dtype == np.float32:
        return "s"
    if dtype == np.complex64:
        return "c"
    raise TypeError("supported scalar types: float32/64, complex64/128 (got %s)" % dtype)


def _is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def _real_eps(dtype):
    """Machine epsilon of real_t<T> (the reference scales its default tolerances with it, LL:150, EX:58)."""
    return float(np.finfo(np.dtype(dtype)).eps)


class DeviceArray:
    """A device allocation owned by a Context (freed with it or by .free())."""

    def __init__(self, ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().ll_malloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def at(self, elem_offset):
        return C.c_void_p(self.ptr + int(elem_offset) * self.dtype.itemsize)

    def set(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes <= self.nbytes
        check(lib().ll_memcpy_h2d(self.ctx.handle, self.ptr, ptr(host), host.nbytes))
        return self

    def get(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(lib().ll_memcpy_d2h(self.ctx.handle, ptr(out), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            check(lib().ll_free(self.ctx.handle, self.ptr))
            self.ptr = None


_LIVE_CONTEXTS = weakref.WeakSet()


def live_contexts():
    """The Context objects that have not been closed (the test suite reloads their LL_* switches after changing one)."""
    return [c for c in list(_LIVE_CONTEXTS) if c.handle]


# callables(context) run at the end of Context.__init__ (the test harness applies its per-context tuning through them)
CONTEXT_CREATED_HOOKS = []


class Context:
    """Device + HIP stream + workspace (+ RCCL communicator): ll_context."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        if stream is None:
            check(lib().ll_ctx_create(int(device), C.byref(h)))
        else:
            check(lib().ll_ctx_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self.rank, self.n_ranks = 0, 1
        _LIVE_CONTEXTS.add(self)
        for hook in list(CONTEXT_CREATED_HOOKS):
            hook(self)

    # ---- multi-GPU
    @staticmethod
    def unique_id():
        buf = (C.c_char * capi.UNIQUE_ID_BYTES)()
        check(lib().ll_comm_unique_id(buf))
        return bytes(buf)

    def init_comm(self, unique_id, rank, n_ranks):
        buf = (C.c_char * capi.UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().ll_comm_init(self.handle, buf, int(rank), int(n_ranks)))
        self.rank, self.n_ranks = int(rank), int(n_ranks)

    def ranks_seen(self):
        """Rank tags that arrived in the communicator self-check of init_comm (== n_ranks when healthy; 1 without one)."""
        out = C.c_int()
        check(lib().ll_comm_ranks_seen(self.handle, C.byref(out)))
        return out.value

    def transport(self):
        """Which transport answers the collectives: "rccl", "plugin:<path>", "attached" or "none" (ll_comm_transport)."""
        buf = C.create_string_buffer(512)
        check(lib().ll_comm_transport(self.handle, buf, len(buf)))
        return buf.value.decode()

    def partition(self, n):
        return partition(n, self.n_ranks, self.rank)

    # ---- memory
    def empty(self, shape, dtype=np.float64):
        return DeviceArray(self, shape, dtype)

    def to_device(self, host):
        host = np.ascontiguousarray(host)
        return DeviceArray(self, host.shape, host.dtype).set(host)

    def synchronize(self):
        check(lib().ll_ctx_synchronize(self.handle))

    def stream(self):
        p = C.c_void_p()
        check(lib().ll_ctx_stream(self.handle, C.byref(p)))
        return p.value

    def timer_start(self):
        check(lib().ll_timer_start(self.handle))

    def timer_stop(self):
        """Milliseconds of device time on this context's stream since timer_start()."""
        ms = C.c_double()
        check(lib().ll_timer_stop(self.handle, C.byref(ms)))
        return ms.value

    def bandwidth_probe(self, nbytes=2 << 30):
        """(read-only GB/s, copy GB/s) of two plain streaming kernels over nbytes, measured now (ll_bandwidth_probe)."""
        r, c = C.c_double(), C.c_double()
        check(lib().ll_bandwidth_probe(self.handle, int(nbytes), C.byref(r), C.byref(c)))
        return r.value, c.value

    def release_cache(self):
        check(lib().ll_ctx_release_cache(self.handle))

    def reload_env(self):
        """Read the LL_* environment switches again (they are read once, when the context is created)."""
        check(lib().ll_ctx_reload_env(self.handle))

    def set_tuning(self, key, value):
        """ll_ctx_set_tuning (UNSTABLE; tests and probes): one tuning field of this context by key, on top of the environment;
        value None removes the setting again."""
        check(lib().ll_ctx_set_tuning(self.handle, str(key).encode(), None if value is None else str(value).encode()))

    def set_profiling(self, on):
        check(lib().ll_ctx_set_profiling(self.handle, 1 if on else 0))

    def close(self):
        if self.handle:
            check(lib().ll_ctx_destroy(self.handle))
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def partition(n, n_ranks, rank):
    """(row_begin, n_local) of `rank` in the 1-D contiguous row partition (ll_partition)."""
    b, c = C.c_int64(), C.c_int64()
    check(lib().ll_partition(int(n), int(n_ranks), int(rank), C.byref(b), C.byref(c)))
    return b.value, c.value


# ------------------------------------------------------------------ operators (the mv_mul plugin)
class _Operator:
    handle = None

    def info(self):
        n, nl, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().ll_op_info(self.handle, C.byref(n), C.byref(nl), C.byref(nnz)))
        return n.value, nl.value, nnz.value

    def device_bytes(self):
        """Device bytes the operator's images hold (ll_op_device_bytes; the context's caches are not counted)."""
        b = C.c_int64()
        check(lib().ll_op_device_bytes(self.handle, C.byref(b)))
        return b.value

    def close(self):
        if self.handle:
            check(lib().ll_op_destroy(self.handle))
            self.handle = None


class CsrOperator(_Operator):
    """Device-resident CSR matrix (rows [row_begin, row_begin+len(row_ptr)-1) of an n_cols x n_cols operator)."""

    def __init__(self, ctx, row_ptr, col, val, n_cols=None, row_begin=0, accuracy=None, kernel=None):
        """accuracy: None (the environment decides), capi.ACCURACY_NORMWISE or capi.ACCURACY_COMPONENTWISE — the accuracy class
        of y = A x (include/lanczos_hip.h, ll_csr_options); kernel: None (timed at creation), capi.SPMV_CSR_STREAM / SPMV_PB / SPMV_TILED
        (SPMV_TILED: an error for a matrix that is not eligible or has no entries, never a silent fallback)."""
        self.ctx = ctx
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val)
        self.dtype = val.dtype
        sfx = _suffix(val.dtype)
        n_rows = row_ptr.shape[0] - 1
        self.n = int(n_cols if n_cols is not None else n_rows)
        self.n_local, self.row_begin = n_rows, int(row_begin)
        h = C.c_void_p()
        if accuracy is None and kernel is None:
            fn = getattr(lib(), "ll_op_create_csr_" + sfx)
            check(fn(ctx.handle, n_rows, self.n, self.row_begin, ptr(row_ptr), ptr(col), ptr(val), C.byref(h)))
        else:
            opt = capi.CsrOptions()
            check(lib().ll_csr_options_default(C.byref(opt)))
            opt.accuracy = capi.ACCURACY_DEFAULT if accuracy is None else int(accuracy)
            opt.kernel = -1 if kernel is None else int(kernel)
            fn = getattr(lib(), "ll_op_create_csr_opt_" + sfx)
            check(fn(ctx.handle, n_rows, self.n, self.row_begin, ptr(row_ptr), ptr(col), ptr(val), C.byref(opt), C.byref(h)))
        self.handle = h
        self.nnz = int(row_ptr[-1])

    @classmethod
    def from_coo(cls, ctx, n, rows, cols, vals):
        """{row, col, value} triplets (sample2_sparse.cpp:14-47); conversion to CSR happens in the library."""
        self = cls.__new__(cls)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        vals = np.ascontiguousarray(vals)
        self.ctx, self.dtype, self.n, self.n_local, self.row_begin, self.nnz = ctx, vals.dtype, int(n), int(n), 0, len(vals)
        h = C.c_void_p()
        fn = getattr(lib(), "ll_op_create_coo_" + _suffix(vals.dtype))
        check(fn(ctx.handle, int(n), len(vals), ptr(rows), ptr(cols), ptr(vals), C.byref(h)))
        self.handle = h
        return self

    @classmethod
    def from_triangle(cls, ctx, row_ptr, col, val, uplo="U", accuracy=None, kernel=None):
        """A symmetric (real) / Hermitian (complex) n x n matrix given as ONE stored triangle (ll_op_create_csr_sym_*):
        A = T + T^T - diag(T), or T + T^H - diag(T) for complex types.  uplo: "U" (col >= row) or "L" (col <= row).
        kernel: None (capi.SPMV_SYM when the triangle is eligible, else the expanded full matrix, timed), capi.SPMV_SYM (an
        error when not eligible), or another capi.SPMV_* for the expanded matrix; accuracy as for the constructor.
        row_ptr / col / val may also be DeviceArrays (int64 / int32 / values already in HBM)."""
        if uplo not in ("U", "L", capi.UPPER, capi.LOWER):
            raise ValueError("uplo must be 'U' or 'L'")
        self = cls.__new__(cls)
        on_device = isinstance(row_ptr, DeviceArray)
        if on_device:  # device arrays (int64 row_ptr, int32 col, values): ll_csr_options.arrays_on_device = 1
            if not (isinstance(col, DeviceArray) and isinstance(val, DeviceArray)):
                raise TypeError("row_ptr, col and val must all be DeviceArrays, or all host arrays")
            if row_ptr.dtype != np.int64 or col.dtype != np.int32:
                raise TypeError("device row_ptr must be int64 and col int32")
            n = row_ptr.shape[0] - 1
            self.nnz = int(col.shape[0])
            args = (row_ptr.ptr, col.ptr, val.ptr)
        else:
            row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
            col = np.ascontiguousarray(col, dtype=np.int32)
            val = np.ascontiguousarray(val)
            n = row_ptr.shape[0] - 1
            self.nnz = int(row_ptr[-1])
            args = (ptr(row_ptr), ptr(col), ptr(val))
        self.ctx, self.dtype, self.n, self.n_local, self.row_begin = ctx, val.dtype, n, n, 0
        opt = capi.CsrOptions()
        check(lib().ll_csr_options_default(C.byref(opt)))
        opt.accuracy = capi.ACCURACY_DEFAULT if accuracy is None else int(accuracy)
        opt.kernel = -1 if kernel is None else int(kernel)
        opt.arrays_on_device = 1 if on_device else 0
        code = capi.UPPER if uplo in ("U", capi.UPPER) else capi.LOWER
        h = C.c_void_p()
        fn = getattr(lib(), "ll_op_create_csr_sym_" + _suffix(val.dtype))
        check(fn(ctx.handle, n, code, *args, C.byref(opt), C.byref(h)))
        self.handle = h
        return self

    def inf_norm(self):
        """max_i sum_j |a_ij| of the local rows (a safe |eigenvalue_offset|)."""
        v = C.c_double()
        check(lib().ll_op_inf_norm(self.handle, C.byref(v)))
        return v.value

    def select_spmv(self, kind):
        """capi.SPMV_PB or capi.SPMV_CSR_STREAM (default: whichever timed faster at creation)."""
        check(lib().ll_op_select_spmv(self.handle, int(kind)))

    def set_accuracy(self, accuracy):
        """capi.ACCURACY_NORMWISE or capi.ACCURACY_COMPONENTWISE (ll_op_set_accuracy): same image, another summation kernel."""
        check(lib().ll_op_set_accuracy(self.handle, int(accuracy)))

    def accuracy(self):
        """The accuracy class of the kernel selected now (ll_op_accuracy)."""
        a = C.c_int()
        check(lib().ll_op_accuracy(self.handle, C.byref(a)))
        return a.value

    def autotune_ms(self):
        """(csr_stream_ms, pb_ms) measured when the operator was created (-1: not timed)."""
        a, b = C.c_double(), C.c_double()
        check(lib().ll_op_autotune_ms(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def autotune_ms_of(self, kind):
        """Creation-time timing of one kernel (capi.SPMV_*), -1 when it was not a candidate."""
        a = C.c_double()
        check(lib().ll_op_autotune_ms_of(self.handle, int(kind), C.byref(a)))
        return a.value

    def tiled_layout(self):
        """(row blocks of the tiled image, those of them whose tiles all lie inside the rank's own columns) — (0, 0) without a tiled image."""
        a, b = C.c_int(), C.c_int()
        check(lib().ll_op_tiled_layout(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def selected_spmv(self):
        k = C.c_int()
        check(lib().ll_op_selected_spmv(self.handle, C.byref(k)))
        return k.value


class DenseOperator(_Operator):
    """Dense row-major matrix (sample1_simple.cpp:22-28): rows [row_begin, row_begin + a.shape[0]) of an n x n matrix."""

    def __init__(self, ctx, a, row_begin=0):
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float32, np.float64, np.complex64, np.complex128):
            a = a.astype(np.float64)
        self.ctx, self.dtype = ctx, a.dtype
        self.n_local, self.n = int(a.shape[0]), int(a.shape[1])
        self.row_begin, self.nnz = int(row_begin), int(a.size)
        h = C.c_void_p()
        fn = getattr(lib(), "ll_op_create_dense_" + _suffix(a.dtype))
        check(fn(ctx.handle, self.n_local, self.n, self.row_begin, ptr(a), C.byref(h)))
        self.handle = h

    inf_norm = CsrOperator.inf_norm


class StencilOperator(_Operator):
    """Matrix-free lattice operator (sample3_dynamic.cpp:17-22, T1:265-273, T2:113-121):
    (A x)(r) = (diag + onsite[r]) x(r) + sum_d (hop[d] x(r+e_d) + conj(hop[d]) x(r-e_d)) on a row-major lattice
    `dims` (last index fastest), open or periodic per dimension; phase_grad (ndim x ndim, complex types) adds Peierls
    phases exp(i * phase_grad[d] . coords(lower site)) to the hops.  Sharded contexts pass their ll_partition range."""

    def __init__(self, ctx, dims, diag=0.0, hop=-1.0, periodic=False, onsite=None, dtype=np.float64, row_begin=0,
                 n_local=None, phase_grad=None):
        dims = [int(d) for d in np.atleast_1d(dims)]
        nd = len(dims)
        if not 1 <= nd <= 3:
            raise ValueError("the lattice operator supports 1, 2 or 3 dimensions")
        hop = np.broadcast_to(np.asarray(hop, dtype=np.complex128), (nd,))
        periodic = np.broadcast_to(np.asarray(periodic, dtype=bool), (nd,))
        d = capi.StencilDesc()
        d.ndim = nd
        for k in range(nd):
            d.dims[k], d.periodic[k] = dims[k], int(periodic[k])
            d.hop_re[k], d.hop_im[k] = float(hop[k].real), float(hop[k].imag)
        d.diag = float(diag)
        if phase_grad is not None:  # Peierls phases: bond r -> r+e_d carries hop[d] * exp(i * phase_grad[d] . coords(r))
            pg = np.asarray(phase_grad, dtype=np.float64).reshape(nd, nd)
            for k in range(nd):
                for e in range(nd):
                    d.phase_grad[k][e] = float(pg[k, e])
        self.ctx, self.dtype = ctx, np.dtype(dtype)
        self.n = int(np.prod(dims))
        self.n_local = self.n if n_local is None else int(n_local)
        self.row_begin, self.nnz = int(row_begin), 0
        os_ = None if onsite is None else np.ascontiguousarray(onsite, dtype=np.float64)
        if os_ is not None and os_.shape[0] != self.n_local:
            raise ValueError("onsite must hold n_local values")
        h = C.c_void_p()
        fn = getattr(lib(), "ll_op_create_stencil_" + _suffix(self.dtype))
        check(fn(ctx.handle, C.byref(d), self.row_begin, self.n_local, ptr(os_), C.byref(h)))
        self.handle = h

    inf_norm = CsrOperator.inf_norm


class _PauliFamily(_Operator):
    """What the Pauli-sum operators with typed entry points share: the term array and the create call, ll_op_create_pauli<kind>_<suffix>(ctx,
    *args, n_terms, terms, out).  n is what creation counted."""

    def _create(self, ctx, kind, dtype, terms, *args):
        arr, n_terms = _term_array(terms)
        self.ctx, self.dtype = ctx, np.dtype(dtype)
        self.row_begin, self.nnz = 0, n_terms
        h = C.c_void_p()
        fn = getattr(lib(), "ll_op_create_pauli" + kind + "_" + _suffix(self.dtype))
        check(fn(ctx.handle, *args, n_terms, arr, C.byref(h)))
        self.handle = h
        self.n = self.n_local = self.info()[0]


def _term_array(terms):
    """(x_mask, z_mask, coef) tuples as an ll_pauli_term array (one spare element: ctypes has no empty array)."""
    terms = list(terms)
    arr = (capi.PauliTerm * max(len(terms), 1))()
    for k, (xm, zm, c) in enumerate(terms):
        arr[k].x_mask, arr[k].z_mask, arr[k].coef = int(xm), int(zm), float(c)
    return arr, len(terms)


def _vector_arg(vec, n, dtype, type_error, value_error):
    """(keep_alive, void*) of a vector argument of n values of `dtype`: a numpy array (converted to dtype; ValueError unless it
    holds exactly n) or anything with .ptr, .dtype, .shape that names device memory (TypeError unless it holds at least n values
    of dtype).  The two texts are formats of n, dtype and size (what the array holds), filled in only when raised.  The caller
    keeps keep_alive until the library returns."""
    if hasattr(vec, "ptr"):
        if vec.dtype != dtype or int(np.prod(vec.shape)) < n:
            raise TypeError(type_error % {"n": n, "dtype": np.dtype(dtype)})
        return vec, C.c_void_p(vec.ptr)
    keep = np.ascontiguousarray(vec, dtype=dtype)
    if keep.size != n:
        raise ValueError(value_error % {"n": n, "size": keep.size})
    return keep, ptr(keep)


_PSI_ERRORS = ("psi must hold n_local values of the operator's dtype %(dtype)s", "psi holds %(size)d values, the operator's basis %(n)d")
_INPUT_ERRORS = ("the input must hold %(n)d values of the operators' dtype %(dtype)s", "the input holds %(size)d values, its basis %(n)d")


def _pauli_expect_call(entry, op, psi, observables, return_sweeps):
    arr, n_obs = _term_array(observables)
    keep, p = _vector_arg(psi, op.n_local, op.dtype, *_PSI_ERRORS)
    out = np.zeros(n_obs, dtype=np.float64)
    sweeps = C.c_int64(0)
    check(getattr(lib(), entry)(op.ctx.handle, op.handle, n_obs, arr, p, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sweeps)))
    return (out, int(sweeps.value)) if return_sweeps else out


def pauli_expect(op, psi, observables, return_sweeps=False):
    """ll_pauli_expect: coef * Re <psi| P |psi> for every observable (x_mask, z_mask, coef) on the basis of `op`, as a float64
    array — many observables per sweep over psi, no n-sized workspace for a device psi; nothing is divided by <psi|psi>.
    psi: a numpy array (converted to the operator's dtype) or a DeviceArray (anything with .ptr, .dtype, .shape that names
    device memory) of op.n_local values of that dtype.  With return_sweeps also the number of passes over psi that were
    launched.  The library refuses every operator but PauliOperator and PauliSectorOperator."""
    return _pauli_expect_call("ll_pauli_expect", op, psi, observables, return_sweeps)


def pauli_expect_block(op, psi, observables, return_sweeps=False):
    """ll_pauli_expect_block: coef * Re <Psi| P |Psi> for every observable (x_mask, z_mask, coef), Psi = B psi the state that the
    op.n_local coefficients `psi` on the representatives of a symmetry block stand for (B: generators.momentum_embedding,
    full_momentum_embedding or symmetric_embedding) — Psi is never formed: every observable is averaged over the block's group
    (generators.symmetrised_strings) and measured with the gather of the operator's own apply, up to 32 per sweep over psi;
    nothing is divided by <psi|psi>.  psi and return_sweeps as pauli_expect.  A PauliTorusOperator averages over the torus's
    translations (generators.torus_embedding, torus_symmetrised_strings).  The library refuses every operator but
    PauliMomentumOperator, PauliMomentumFullOperator, PauliSymmetricOperator and PauliTorusOperator."""
    return _pauli_expect_call("ll_pauli_expect_block", op, psi, observables, return_sweeps)


def _out_arg(out, n_out, dtype):
    """(out, void*) of an output of n_out values of `dtype`: None (a new numpy array), a contiguous writeable numpy array of
    exactly that, or anything with .ptr, .dtype, .shape that names device memory of at least that (TypeError otherwise)."""
    if out is None:
        out = np.empty(n_out, dtype=dtype)
    if hasattr(out, "ptr"):
        if out.dtype != dtype or int(np.prod(out.shape)) < n_out:
            raise TypeError("out must hold %d values of the operators' dtype %s" % (n_out, dtype))
        return out, C.c_void_p(out.ptr)
    if not (isinstance(out, np.ndarray) and out.dtype == dtype and out.size == n_out and out.flags.c_contiguous and
            out.flags.writeable):
        raise TypeError("out must be a contiguous writeable numpy array of %d values of dtype %s" % (n_out, dtype))
    return out, ptr(out)


def _pauli_embed_call(entry, block, target, vec, n_in, n_out, out):
    dtype = np.dtype(block.dtype)
    keep, p = _vector_arg(vec, n_in, dtype, *_INPUT_ERRORS)
    out, q = _out_arg(out, n_out, dtype)
    check(getattr(lib(), entry)(block.ctx.handle, block.handle, target.handle, p, q))
    del keep
    return out


def pauli_block_expand(block, c, target, out=None):
    """ll_pauli_block_expand: Psi = B c — the block.n_local coefficients c on the representatives of a symmetry block
    (PauliMomentumOperator, PauliMomentumFullOperator, PauliSymmetricOperator) as the target.n_local amplitudes on the basis of
    `target` (a PauliOperator, or the PauliSectorOperator of the block's n_down), B = generators.momentum_embedding,
    full_momentum_embedding or symmetric_embedding.  States whose orbit the block excludes, and for a sector block in the full
    space the states outside the sector, come back exactly +0.0.  c: a numpy array (converted to the operators' dtype) or a
    DeviceArray (anything with .ptr, .dtype, .shape); out: None (a new numpy array), a numpy array or a DeviceArray of the
    operators' dtype — returned filled."""
    return _pauli_embed_call("ll_pauli_block_expand", block, target, c, block.n_local, target.n_local, out)


def pauli_block_project(block, psi, target, out=None):
    """ll_pauli_block_project: c = B^H Psi for ANY Psi on the basis of `target` — the block.n_local coefficients of its part in the
    block; ||c||^2 is the weight of Psi in the block and pauli_block_project(block, pauli_block_expand(block, c, t), t) = c.
    Arguments as pauli_block_expand."""
    return _pauli_embed_call("ll_pauli_block_project", block, target, psi, target.n_local, block.n_local, out)


def pauli_block_transfer(source, target, terms, c, out=None, return_norm2=False):
    """ll_pauli_block_transfer: out = B_t^H (sum_j coef_j P_j) B_s c — a sum of Pauli strings (x_mask, z_mask, coef) applied to
    the source.n_local coefficients c of a state of one momentum block, the result taken as the target.n_local coefficients on
    another (both PauliMomentumOperator of one n_sites and n_down, or both PauliMomentumFullOperator of one n_sites; B =
    generators.momentum_embedding / full_momentum_embedding), without a vector of the full space
    (generators.pauli_block_transfer_np).  The strings need not commute with the translation: the target block selects their
    component of momentum target.momentum - source.momentum.  c: a numpy array (converted to the operators' dtype) or a
    DeviceArray (anything with .ptr, .dtype, .shape); out: None (a new numpy array), a numpy array or a DeviceArray of the
    operators' dtype — returned filled; with return_norm2 also sum |out|^2 as the kernel sums it."""
    dtype = np.dtype(source.dtype)
    arr, n_terms = _term_array(terms)
    keep, p = _vector_arg(c, source.n_local, dtype, *_INPUT_ERRORS)
    out, q = _out_arg(out, target.n_local, dtype)
    norm2 = C.c_double(0.0)
    check(lib().ll_pauli_block_transfer(source.ctx.handle, source.handle, target.handle, n_terms, arr, p, q, C.byref(norm2)))
    del keep
    return (out, float(norm2.value)) if return_norm2 else out


def lanczos_coefficients(op, start, m):
    """(alpha, beta, iterations): the Lanczos tridiagonal of (op, start) after at most m steps without a stored basis — a thin
    wrapper over LambdaLanczos.run_two_pass(want_vector=False) with eps = 0 (the stop test cannot fire; breakdown still ends
    the run) and max_iteration = m.  start: a DeviceArray of op.n_local values of op.dtype, read and never modified; it need not
    be normalised.  alpha and beta hold `iterations` entries each, indexed as ll_lanczos_two_pass_* writes them: beta[k] couples
    alpha[k] and alpha[k + 1], and the last entry, beta[iterations - 1], is the norm of the residual that ended the run — not
    an element of the tridiagonal (continued_fraction leaves it out)."""
    if not isinstance(start, DeviceArray):
        raise TypeError("start must be a DeviceArray of op.n_local values")
    eng = LambdaLanczos(op, op.n, False, 1, dtype=op.dtype, context=op.ctx)
    eng.init_vector = start
    eng.eps = 0.0
    eng.max_iteration = int(m)
    _, _, info = eng.run_two_pass(want_vector=False)
    return eng.last_alpha, eng.last_beta, info["iterations"]


def continued_fraction(alpha, beta, z, norm2=1.0):
    """norm2 / (z - alpha[0] - beta[0]^2 / (z - alpha[1] - beta[1]^2 / (... - alpha[m - 1]))) = norm2 e_1^T (z - T)^-1 e_1 for the
    m x m tridiagonal T of a Lanczos run, vectorised over complex z and evaluated bottom-up (m divisions per z).  Indexing as
    ll_lanczos_two_pass_* writes it (lanczos_coefficients): m = len(alpha), beta[k] couples alpha[k] and alpha[k + 1]; only
    beta[0 .. m - 2] enter, so beta may hold m - 1 entries or m (the residual norm in the last one is not read)."""
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1)
    m = alpha.shape[0]
    if m < 1 or beta.shape[0] < m - 1:
        raise ValueError("need at least one alpha and len(alpha) - 1 betas")
    z = np.asarray(z, dtype=np.complex128)
    d = z - alpha[m - 1]
    for k in range(m - 2, -1, -1):
        d = z - alpha[k] - (beta[k] * beta[k]) / d
    return float(norm2) / d


def spectral_function(alpha, beta, omega, eta, e0=0.0, norm2=1.0):
    """-Im G(omega + e0 + i eta) / pi with G = continued_fraction(alpha, beta, ., norm2): the spectral function of the start
    vector of the Lanczos run, Lorentz-broadened by eta > 0, on the real frequencies omega measured from e0 (the ground-state
    energy).  It integrates to norm2 over omega."""
    z = np.asarray(omega, dtype=np.float64) + float(e0) + 1j * float(eta)
    return -continued_fraction(alpha, beta, z, norm2).imag / np.pi


def _block_rdm(block, c, sites, target, return_sweeps=False):
    buf = block.ctx.empty(target.n_local, block.dtype)   # the expanded state: a context-owned device buffer, freed below
    try:
        pauli_block_expand(block, c, target, out=buf)
        return pauli_rdm(target, buf, sites, return_sweeps)
    finally:
        buf.free()


def pauli_rdm(op, psi, sites, return_sweeps=False):
    """ll_pauli_rdm: the reduced density matrix rho[a][a'] = sum_e psi(a, e) conj psi(a', e) of the sites `sites` (1 to 6 distinct
    sites; bit k of a is sites[k]) of a state on the basis of `op`, as a complex128 array of shape (2^m, 2^m) — one sweep over
    psi, no n-sized workspace for a device psi; nothing is divided by <psi|psi>: the trace is ||psi||^2.  psi as for pauli_expect:
    a numpy array (converted to the operator's dtype) or anything with .ptr, .dtype, .shape that names device memory.  With
    return_sweeps also the number of passes over psi (1).  The library refuses every operator but PauliOperator and
    PauliSectorOperator."""
    sites = [int(s) for s in sites]
    m = len(sites)
    arr = (C.c_int32 * max(m, 1))(*sites)
    keep, p = _vector_arg(psi, op.n_local, op.dtype, *_PSI_ERRORS)
    dim = 1 << min(max(m, 0), 6)   # (a count the library refuses still gets a buffer)
    out = np.zeros((dim, dim), dtype=np.complex128)
    sweeps = C.c_int64(0)
    check(lib().ll_pauli_rdm(op.ctx.handle, op.handle, m, arr, p, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(sweeps)))
    return (out, int(sweeps.value)) if return_sweeps else out


def pauli_rdm_tiled(op, psi, sites, out=None, return_sweeps=False):
    """ll_pauli_rdm_tiled: the reduced density matrix of pauli_rdm for 4 to 13 distinct sites (bit k of a is sites[k]), formed as
    the rank-K update rho = F F^H on the f64 matrix cores — the half chain of a ring of 20 to 26 sites.  Returns a complex128
    array of shape (2^m, 2^m); or fills `out`, a DeviceArray (anything with .ptr, .dtype, .shape that names device memory) of
    4^m complex128 values or a contiguous writeable complex128 numpy array of that size, and returns it.  Exactly Hermitian, not
    divided by <psi|psi>.  psi as for pauli_rdm.  With return_sweeps also the number of passes (1).  The library refuses every
    operator but PauliOperator and PauliSectorOperator, and a count outside 4 .. 13."""
    sites = [int(s) for s in sites]
    m = len(sites)
    arr = (C.c_int32 * max(m, 1))(*sites)
    keep, p = _vector_arg(psi, op.n_local, op.dtype, *_PSI_ERRORS)
    dim = 1 << (m if 4 <= m <= 13 else 4)   # (a count the library refuses still gets a buffer, a small one)
    if out is None:
        out = np.zeros((dim, dim), dtype=np.complex128)
    out, q = _out_arg(out, dim * dim, np.dtype(np.complex128))
    sweeps = C.c_int64(0)
    check(lib().ll_pauli_rdm_tiled(op.ctx.handle, op.handle, m, arr, p, q, C.byref(sweeps)))
    del keep
    return (out, int(sweeps.value)) if return_sweeps else out


def _block_rdm_tiled(block, c, sites, target, return_sweeps=False):
    buf = block.ctx.empty(target.n_local, block.dtype)   # the expanded state: a context-owned device buffer, freed below
    try:
        pauli_block_expand(block, c, target, out=buf)
        return pauli_rdm_tiled(target, buf, sites, None, return_sweeps)
    finally:
        buf.free()


def entanglement_entropy(rho):
    """The von Neumann entropy -sum lambda ln lambda of rho / tr rho (host numpy: numpy.linalg.eigvalsh of the Hermitian
    matrix; eigenvalues <= 0 contribute 0)."""
    rho = np.asarray(rho, dtype=np.complex128)
    lam = np.linalg.eigvalsh(rho / np.trace(rho).real)
    lam = lam[lam > 0.0]
    return float(-np.sum(lam * np.log(lam))) + 0.0   # (never -0.0)


class PauliOperator(_PauliFamily):
    """Matrix-free spin-1/2 Hamiltonian H = sum_t coef_t P_t (ll_op_create_pauli_*): `terms` is a sequence of
    (x_mask, z_mask, coef); bit j of a basis state is site j, a site carries X (x bit only), Z (z bit only) or Y (both).
    n = 2^n_sites; single-GPU contexts; the real dtypes take terms with an even number of Y only."""

    def __init__(self, ctx, n_sites, terms, dtype=np.float64):
        self.n_sites = int(n_sites)
        self._create(ctx, "", dtype, terms, self.n_sites)

    def inf_norm(self):
        """sum_t |coef_t|: an upper bound of every absolute row sum (a safe |eigenvalue_offset|)."""
        return CsrOperator.inf_norm(self)

    def expectation(self, psi, observables, return_sweeps=False):
        """coef * Re <psi| P |psi> for every (x_mask, z_mask, coef) of `observables`, as a float64 array (pauli_expect)."""
        return pauli_expect(self, psi, observables, return_sweeps)

    def reduced_density_matrix(self, psi, sites, return_sweeps=False):
        """rho_A = Tr_env |psi><psi| of the sites `sites` (at most 6), complex128 of shape (2^m, 2^m), not normalised (pauli_rdm)."""
        return pauli_rdm(self, psi, sites, return_sweeps)

    def reduced_density_matrix_tiled(self, psi, sites, out=None, return_sweeps=False):
        """rho_A of 4 to 13 sites on the f64 matrix cores, complex128 of shape (2^m, 2^m) or `out` filled (pauli_rdm_tiled)."""
        return pauli_rdm_tiled(self, psi, sites, out, return_sweeps)


class PauliSectorOperator(_PauliFamily):
    """The same Hamiltonian on one magnetisation sector (ll_op_create_pauli_sector_*): the basis is the comb(n_sites, n_down)
    states with n_down set bits (a set bit is sigma_z = -1) in ascending integer order (generators.sector_states), and H must
    conserve total S_z — creation refuses one that does not, naming the x mask at fault.  Terms, dtypes and limits as
    PauliOperator; 0 <= n_down <= n_sites."""

    def __init__(self, ctx, n_sites, n_down, terms, dtype=np.float64):
        self.n_sites, self.n_down = int(n_sites), int(n_down)
        self._create(ctx, "_sector", dtype, terms, self.n_sites, self.n_down)

    inf_norm = PauliOperator.inf_norm
    expectation = PauliOperator.expectation  # psi on the sector's basis; a partner outside the sector contributes nothing
    reduced_density_matrix = PauliOperator.reduced_density_matrix  # popcount(a) != popcount(a') is exactly +0.0
    reduced_density_matrix_tiled = PauliOperator.reduced_density_matrix_tiled


class PauliMomentumOperator(_PauliFamily):
    """One momentum block of one magnetisation sector of a ring (ll_op_create_pauli_momentum_*): the operator B^H H_sector B with
    B = generators.momentum_embedding(n_sites, n_down, momentum); the basis is the orbit representatives of
    generators.momentum_basis, ascending.  H must conserve total S_z and commute with the one-site translation — creation
    refuses one that does not, naming the term at fault.  0 <= momentum < n_sites; the real dtypes take momentum 0 and
    n_sites / 2 only.  Holds 4 comb(n_sites, n_down) bytes of look-up table on the device (device_bytes)."""

    def __init__(self, ctx, n_sites, n_down, momentum, terms, dtype=np.float64):
        self.n_sites, self.n_down, self.momentum = int(n_sites), int(n_down), int(momentum)
        self._create(ctx, "_momentum", dtype, terms, self.n_sites, self.n_down, self.momentum)  # n = D_m

    def inf_norm(self):
        """sum_t |coef_t|: an upper bound of every |eigenvalue| of the block (a safe |eigenvalue_offset|)."""
        return CsrOperator.inf_norm(self)

    def expectation(self, psi, observables, return_sweeps=False):
        """coef * Re <B psi| P |B psi> for every (x_mask, z_mask, coef) of `observables`, psi the coefficients on the block's
        representatives, as a float64 array (pauli_expect_block)."""
        return pauli_expect_block(self, psi, observables, return_sweeps)

    def expand(self, c, target, out=None):
        """Psi = B c on the basis of `target`: the PauliOperator of the ring, or the PauliSectorOperator of this block's n_down
        (pauli_block_expand)."""
        return pauli_block_expand(self, c, target, out)

    def project(self, psi, target, out=None):
        """c = B^H Psi, the part of ANY state on the basis of `target` that lies in this block (pauli_block_project)."""
        return pauli_block_project(self, psi, target, out)

    def transfer(self, terms, c, target, out=None, return_norm2=False):
        """B_t^H (sum of `terms`) B c: the strings applied to the state c of this block, taken on the momentum block `target` of
        the same kind, n_sites and n_down (pauli_block_transfer).  The library refuses a momentum / reflection / spin-inversion
        block."""
        return pauli_block_transfer(self, target, terms, c, out, return_norm2)

    def reduced_density_matrix(self, c, sites, target, return_sweeps=False):
        """rho_A = Tr_env |Psi><Psi| of Psi = B c: c is expanded into a device buffer of target.n_local values, measured with
        target.reduced_density_matrix (pauli_rdm) and the buffer freed.  entanglement_entropy takes the result."""
        return _block_rdm(self, c, sites, target, return_sweeps)

    def reduced_density_matrix_tiled(self, c, sites, target, return_sweeps=False):
        """The same for 4 to 13 sites: expand, target.reduced_density_matrix_tiled (pauli_rdm_tiled), free."""
        return _block_rdm_tiled(self, c, sites, target, return_sweeps)


class PauliMomentumFullOperator(_PauliFamily):
    """One momentum block of the full 2^n_sites space of a ring (ll_op_create_pauli_momentum_full_*): the operator B^H H B with
    B = generators.full_momentum_embedding(n_sites, momentum) and H the PauliOperator of the same terms; the basis is the orbit
    representatives of generators.full_momentum_basis, ascending.  H must commute with the one-site translation — creation
    refuses one that does not, naming the term at fault — and need not conserve S_z (transverse-field Ising, XYZ rings).
    0 <= momentum < n_sites; the real dtypes take momentum 0 and n_sites / 2 only.  The image is O(n): no table over the
    2^n_sites states (device_bytes <= 8 n + 64 KiB)."""

    def __init__(self, ctx, n_sites, momentum, terms, dtype=np.float64):
        self.n_sites, self.momentum = int(n_sites), int(momentum)
        self._create(ctx, "_momentum_full", dtype, terms, self.n_sites, self.momentum)  # n = D_m

    inf_norm = PauliMomentumOperator.inf_norm
    expectation = PauliMomentumOperator.expectation
    expand = PauliMomentumOperator.expand
    project = PauliMomentumOperator.project
    transfer = PauliMomentumOperator.transfer
    reduced_density_matrix = PauliMomentumOperator.reduced_density_matrix
    reduced_density_matrix_tiled = PauliMomentumOperator.reduced_density_matrix_tiled


class PauliSymmetricOperator(_PauliFamily):
    """One block of a ring under momentum, reflection and spin inversion (ll_op_create_pauli_symmetric_*): the operator B^H H B
    with B = generators.symmetric_embedding(n_sites, momentum, parity, inversion, n_down) and H the PauliOperator (n_down None)
    or the PauliSectorOperator (n_down) of the same terms; the basis is generators.symmetric_basis, ascending.  parity and
    inversion are 0 (the symmetry is not used), +1 or -1; parity != 0 and the real dtypes take momentum 0 and n_sites / 2 only.
    H must commute with the translation and with every symmetry in use — creation refuses one that does not, naming the term
    at fault — and an empty block is refused.  The image is O(n): no table over the states (device_bytes <= 8 n + 192 KiB)."""

    def __init__(self, ctx, n_sites, momentum, terms, dtype=np.float64, parity=0, inversion=0, n_down=None):
        self.n_sites, self.momentum = int(n_sites), int(momentum)
        self.parity, self.inversion = int(parity), int(inversion)
        self.n_down = None if n_down is None else int(n_down)
        self._create(ctx, "_symmetric", dtype, terms, self.n_sites, -1 if self.n_down is None else self.n_down, self.momentum,
                     self.parity, self.inversion)  # n = D

    inf_norm = PauliMomentumOperator.inf_norm
    expectation = PauliMomentumOperator.expectation
    expand = PauliMomentumOperator.expand
    project = PauliMomentumOperator.project
    transfer = PauliMomentumOperator.transfer  # exists to surface the library's refusal: semi-momentum states are not built
    reduced_density_matrix = PauliMomentumOperator.reduced_density_matrix
    reduced_density_matrix_tiled = PauliMomentumOperator.reduced_density_matrix_tiled


class PauliTorusOperator(_PauliFamily):
    """One translation block of an lx x ly torus (ll_op_create_pauli_torus): the operator B^H H B with
    B = generators.torus_embedding(lx, ly, mx, my, n_down) and H the PauliOperator (n_down None) or the PauliSectorOperator (n_down)
    of the same terms; the basis is generators.torus_basis, ascending.  Site (x, y) is bit x + lx y; 0 <= mx < lx, 0 <= my < ly;
    the real dtypes take mx = 0 or lx / 2 and my = 0 or ly / 2 only.  H must commute with both one-site translations — creation
    refuses one that does not, naming the direction and the term at fault — and an empty block is refused.  The image is O(n):
    no table over the states (device_bytes <= 8 n + 192 KiB).  The library refuses expand, project, transfer and the block
    density matrices for this kind; `expectation` measures on the block."""

    def __init__(self, ctx, lx, ly, mx, my, terms, dtype=np.float64, n_down=None):
        self.lx, self.ly, self.mx, self.my = int(lx), int(ly), int(mx), int(my)
        self.n_sites = self.lx * self.ly
        self.n_down = None if n_down is None else int(n_down)
        arr, n_terms = _term_array(terms)
        self.ctx, self.dtype = ctx, np.dtype(dtype)
        self.row_begin, self.nnz = 0, n_terms
        h = C.c_void_p()
        check(lib().ll_op_create_pauli_torus(ctx.handle, ord(_suffix(self.dtype)), self.lx, self.ly,
                                             -1 if self.n_down is None else self.n_down, self.mx, self.my, n_terms, arr, C.byref(h)))
        self.handle = h
        self.n = self.n_local = self.info()[0]  # n = D

    inf_norm = PauliMomentumOperator.inf_norm
    expectation = PauliMomentumOperator.expectation


class HostOperator(_Operator):
    """Unmodified user code: mv_mul(in, out) on numpy arrays, `out` zero-filled on entry (LL:120-126)."""

    def __init__(self, ctx, mv_mul, n, dtype=np.float64):
        self.ctx, self.n, self.n_local, self.row_begin = ctx, int(n), int(n), 0
        self.dtype = np.dtype(dtype)
        self.nnz = 0
        self.calls = 0
        sfx = _suffix(dtype)
        dt = self.dtype

        def tramp(in_p, out_p, nn, _user):
            try:
                a = np.frombuffer((C.c_char * (nn * dt.itemsize)).from_address(in_p), dtype=dt)
                b = np.frombuffer((C.c_char * (nn * dt.itemsize)).from_address(out_p), dtype=dt)
                self.calls += 1
                mv_mul(a, b)
                return 0
            except Exception:  # noqa: BLE001 - reported through the C ABI as LL_ERR_CALLBACK
                import traceback

                traceback.print_exc()
                return 1

        self._cb = capi.HOST_MV_FN(tramp)  # keep alive
        h = C.c_void_p()
        check(getattr(lib(), "ll_op_create_host_" + sfx)(ctx.handle, self.n, self._cb, None, C.byref(h)))
        self.handle = h


# ------------------------------------------------------------------ primitives (one call per kernel family)
def spmv(op, x_dev, y_dev, offset=0.0, want_dot=False):
    d = C.c_double()
    fn = getattr(lib(), "ll_spmv_" + _suffix(op.dtype))
    check(fn(op.ctx.handle, op.handle, x_dev.ptr, y_dev.ptr, float(offset), C.byref(d) if want_dot else None))
    return d.value if want_dot else None


def dot(ctx, a_dev, b_dev, n=None):
    sfx = _suffix(a_dev.dtype)
    n = int(n if n is not None else a_dev.shape[-1])
    out = (C.c_double * 2)()
    check(getattr(lib(), "ll_dot_" + sfx)(ctx.handle, n, a_dev.ptr, b_dev.ptr, out))
    return out[0] if sfx in "ds" else complex(out[0], out[1])


def nrm2(ctx, v_dev, n=None):
    n = int(n if n is not None else v_dev.shape[-1])
    out = C.c_double()
    check(getattr(lib(), "ll_nrm2_" + _suffix(v_dev.dtype))(ctx.handle, n, v_dev.ptr, C.byref(out)))
    return out.value


def scal(ctx, a, v_dev, n=None):
    n = int(n if n is not None else v_dev.shape[-1])
    check(getattr(lib(), "ll_scal_" + _suffix(v_dev.dtype))(ctx.handle, n, float(a), v_dev.ptr))


def normalize(ctx, v_dev, n=None):
    n = int(n if n is not None else v_dev.shape[-1])
    out = C.c_double()
    check(getattr(lib(), "ll_normalize_" + _suffix(v_dev.dtype))(ctx.handle, n, v_dev.ptr, C.byref(out)))
    return out.value


def three_term(ctx, w_dev, u_prev_dev, u_cur_dev, beta, alpha, n=None):
    n = int(n if n is not None else w_dev.shape[-1])
    fn = getattr(lib(), "ll_three_term_" + _suffix(w_dev.dtype))
    check(fn(ctx.handle, n, w_dev.ptr, None if u_prev_dev is None else u_prev_dev.ptr, u_cur_dev.ptr, float(beta),
             float(alpha)))


def recur_accum(ctx, y_dev, x_dev, p_dev, a, b, g, psi_dev, n=None):
    """One replayed step of the two-pass recurrence: y -= a x + b p (p_dev may be None), then psi += g y, in one sweep.  g is real,
    or complex on complex arrays (the Exponentiator's replay, ll_recur_accum_scaled)."""
    n = int(n if n is not None else y_dev.shape[-1])
    sfx = _suffix(y_dev.dtype)
    if isinstance(g, (complex, np.complexfloating)):
        assert sfx in "zc", "a complex g needs complex arrays"
        check(lib().ll_recur_accum_scaled(ctx.handle, ord(sfx), n, y_dev.ptr, x_dev.ptr, None if p_dev is None else p_dev.ptr,
                                          float(a), float(b), float(g.real), float(g.imag), psi_dev.ptr))
        return
    fn = getattr(lib(), "ll_recur_accum_" + sfx)
    check(fn(ctx.handle, n, y_dev.ptr, x_dev.ptr, None if p_dev is None else p_dev.ptr, float(a), float(b), float(g),
             psi_dev.ptr))


def recur_accum_multi(ctx, y_dev, x_dev, p_dev, a, b, g_list, psi_list, n=None):
    """recur_accum with several accumulators in one sweep (ll_recur_accum_multi): y -= a x + b p once (p_dev may be None), then
    psi_list[j] += g_list[j] y for every j.  Every accumulator receives the bits recur_accum gives it on its own."""
    n = int(n if n is not None else y_dev.shape[-1])
    g = np.ascontiguousarray(g_list, dtype=np.complex128).view(np.float64)
    psi = (C.c_void_p * len(psi_list))(*[q.ptr for q in psi_list])
    assert g.shape[0] == 2 * len(psi_list), "one coefficient per accumulator"
    check(lib().ll_recur_accum_multi(ctx.handle, ord(_suffix(y_dev.dtype)), n, y_dev.ptr, x_dev.ptr,
                                     None if p_dev is None else p_dev.ptr, float(a), float(b), len(psi_list),
                                     g.ctypes.data_as(C.POINTER(C.c_double)), psi))


def orth_block(ctx, basis_dev, nb, ld, w_dev, n, mode=capi.ORTH_CGS_DGKS, want_h=False):
    sfx = _suffix(w_dev.dtype)
    norm = C.c_double()
    cplx = sfx in "zc"
    h = np.zeros(max(nb, 1) * (2 if cplx else 1), dtype=np.float64) if want_h else None
    fn = getattr(lib(), "ll_orth_block_" + sfx)
    check(fn(ctx.handle, int(n), int(nb), None if basis_dev is None else basis_dev.ptr, int(ld), w_dev.ptr, int(mode),
             C.byref(norm), ptr(h)))
    if want_h:
        hh = h[: nb * (2 if cplx else 1)]
        return norm.value, (hh.view(np.complex128) if cplx else hh)
    return norm.value


def gemv_basis(ctx, basis_dev, m, ld, coeff, out_dev, ld_out, n):
    sfx = _suffix(out_dev.dtype)
    if sfx in "sc":   # the float entry points take their coefficients as doubles, like every scalar
        coeff = np.ascontiguousarray(coeff, dtype=np.complex128 if sfx == "c" else np.float64)
    else:
        coeff = np.ascontiguousarray(coeff, dtype=out_dev.dtype)
    nout = coeff.shape[0] if coeff.ndim == 2 else 1
    fn = getattr(lib(), "ll_gemv_basis_" + sfx)
    check(fn(ctx.handle, int(n), int(m), basis_dev.ptr, int(ld), int(nout), ptr(coeff), out_dev.ptr, int(ld_out)))


def tridiag_eig(alpha, beta, want_vectors=True):
    """Host tridiagonal eigen-solver of the library (a11): ascending eigenvalues, rows of q = eigenvectors."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    m = alpha.shape[0]
    beta = np.ascontiguousarray(np.concatenate([np.asarray(beta, dtype=np.float64), np.zeros(1)]))
    ev = np.empty(m)
    q = np.empty((m, m)) if want_vectors else None
    unc = C.c_int64()
    check(lib().ll_tridiag_eig(m, ptr(alpha), ptr(beta), ptr(ev), ptr(q), C.byref(unc)))
    return (ev, q, unc.value) if want_vectors else (ev, unc.value)


def tridiag_eigvecs(alpha, beta, lambdas):
    """Eigenvectors (rows) of T(alpha, beta) for the given eigenvalues by inverse iteration."""
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    beta = np.ascontiguousarray(np.concatenate([np.asarray(beta, dtype=np.float64), np.zeros(1)]))
    lam = np.ascontiguousarray(np.atleast_1d(lambdas), dtype=np.float64)
    out = np.empty((lam.shape[0], alpha.shape[0]))
    check(lib().ll_tridiag_eigvecs(alpha.shape[0], ptr(alpha), ptr(beta), lam.shape[0], ptr(lam), ptr(out)))
    return out


def tridiag_bisect(alpha, beta, k):
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    beta = np.ascontiguousarray(np.concatenate([np.asarray(beta, dtype=np.float64), np.zeros(1)]))
    out = C.c_double()
    check(lib().ll_tridiag_bisect(alpha.shape[0], ptr(alpha), ptr(beta), int(k), C.byref(out)))
    return out.value


# ------------------------------------------------------------------ the engines
_default_context = None


def default_context():
    global _default_context
    if _default_context is None:
        _default_context = Context(0)
    return _default_context


def _as_operator(mv_mul, n, dtype, ctx):
    if isinstance(mv_mul, _Operator):
        return mv_mul, False
    if callable(mv_mul):
        return HostOperator(ctx, mv_mul, n, dtype), True
    raise TypeError("mv_mul must be a CsrOperator/HostOperator or a callable mv_mul(in, out)")


class LambdaLanczos:
    """lambda_lanczos::LambdaLanczos<T> (LL:109-415) with device-resident Krylov vectors.

    ``mv_mul`` is a device operator (``CsrOperator``) or — for unmodified user code — a callable
    ``mv_mul(in_array, out_array)`` with the reference's contract (out zero-filled, accumulate or overwrite).
    Public fields and defaults are the reference's (LL:126-181)."""

    def __init__(self, mv_mul, matrix_size, find_maximum, num_eigs, dtype=None, context=None):
        self.context = context or (mv_mul.ctx if isinstance(mv_mul, _Operator) else default_context())
        self.dtype = np.dtype(dtype if dtype is not None else getattr(mv_mul, "dtype", np.float64))
        self.mv_mul = mv_mul                                     # LL:126
        self.init_vector = None                                  # LL:133 (None = random default, LL:70-104)
        self.matrix_size = int(matrix_size)                      # LL:136
        self.max_iteration = int(matrix_size)                    # LL:138,206
        self.eps = _real_eps(self.dtype) * 1e3                   # LL:150 (epsilon of real_t<T>)
        self.find_maximum = bool(find_maximum)                   # LL:153
        self.num_eigs = int(num_eigs)                            # LL:156
        self.eigenvalue_offset = 0.0                             # LL:165
        self.num_eigs_per_iteration = 5                          # LL:173
        self.initial_vector_size = 200                           # LL:181
        # additions (0 = reference-faithful)
        self.tridiag_mode = capi.TRIDIAG_AUTO  # decision- and value-identical to the reference's QR, O(k) per iteration
        self.orth_mode = capi.ORTH_CGS_DGKS
        # device-resident I/O (additions): init_vector may be a DeviceArray (start vector already in HBM), and a
        # DeviceArray of shape (num_eigs, n_local) here receives the eigenvectors instead of a host array
        self.eigenvectors_out = None
        self._iter_counts = []
        self.last_stats = None
        self.last_alpha = self.last_beta = None

    def _params(self, num_eigs):
        p = capi.LanczosParams()
        check(lib().ll_lanczos_params_default(C.byref(p), self.matrix_size, int(self.find_maximum), int(num_eigs)))
        p.max_iteration = int(self.max_iteration)
        p.eps = float(self.eps)
        p.eigenvalue_offset = float(self.eigenvalue_offset)
        p.num_eigs_per_iteration = int(self.num_eigs_per_iteration)
        p.initial_vector_size = int(self.initial_vector_size)
        p.tridiag_mode = int(self.tridiag_mode)
        p.orth_mode = int(self.orth_mode)
        return p

    def run(self, num_eigs=None):
        """Returns (eigenvalues, eigenvectors): eigenvectors[k] is the k-th eigenvector (LL:330-386).
        For sharded contexts each rank receives its row shard of every eigenvector."""
        k = int(self.num_eigs if num_eigs is None else num_eigs)
        vals, vecs, _ = self._drive(k, None, None)
        return vals, vecs

    def run_iteration(self, nroot, orthogonalize_to=None):
        """LambdaLanczos<T>::run_iteration(eigvalues, eigvecs, nroot, orthogonalizeTo) (LL:216-322): ONE pass tracking
        nroot Ritz pairs, every Lanczos vector orthogonalised against the rows of orthogonalize_to first.
        Returns (eigenvalues, eigenvectors, iteration_count); no restart loop, no EigenPairManager filtering."""
        return self._drive(int(nroot), int(nroot), orthogonalize_to)

    def _set_start_vector(self, p, op):
        """Point the params at self.init_vector (DeviceArray or hook); returns what must stay alive during the call."""
        keep = None
        if isinstance(self.init_vector, DeviceArray):  # start vector already in HBM
            assert self.init_vector.dtype == self.dtype and self.init_vector.nbytes >= op.n_local * self.dtype.itemsize
            p.init_vector_dev = self.init_vector.ptr
        elif self.init_vector is not None:
            dt, user_fn = self.dtype, self.init_vector

            def tramp(vec_p, n_local, row_begin, _user):
                v = np.frombuffer((C.c_char * (n_local * dt.itemsize)).from_address(vec_p), dtype=dt)
                try:
                    user_fn(v, row_begin)
                except TypeError:
                    user_fn(v)  # reference signature init_vector(vec) (LL:133)

            keep = capi.INIT_FN(tramp)
            p.init_vector = keep
        return keep

    def _drive(self, k, nroot, orth):
        op, owned = _as_operator(self.mv_mul, self.matrix_size, self.dtype, self.context)
        sfx = _suffix(self.dtype)
        p = self._params(1 if nroot is not None else k)
        keep = self._set_start_vector(p, op)
        n_local = op.n_local
        vals = np.zeros(k, dtype=np.float64)
        dev_out = self.eigenvectors_out
        if dev_out is not None:  # Ritz vectors stay in HBM: rows of the caller's DeviceArray
            assert dev_out.dtype == self.dtype and dev_out.nbytes >= k * n_local * self.dtype.itemsize
            vecs, vecs_p = dev_out, C.c_void_p(dev_out.ptr)
        else:
            vecs = np.empty((k, n_local), dtype=self.dtype)
            vecs_p = ptr(vecs)
        n_found = C.c_int64()
        cap = 4 * k + 64
        counts = np.zeros(cap, dtype=np.int64)
        trace_cap = int(min(self.max_iteration, 1 << 24))
        alpha = np.zeros(trace_cap)
        beta = np.zeros(trace_cap)
        stats = capi.RunStats()
        itern = C.c_int64()
        try:
            if nroot is None:
                fn = getattr(lib(), "ll_lanczos_run_" + sfx)
                check(fn(self.context.handle, op.handle, C.byref(p), ptr(vals), vecs_p, C.byref(n_found), ptr(counts),
                         cap, ptr(alpha), ptr(beta), C.byref(stats)))
            else:
                lock = None
                n_orth = 0
                lock_p = None
                if isinstance(orth, DeviceArray):  # orthogonalizeTo vectors already in HBM: rows of a (n_orth, n_local) array
                    assert orth.dtype == self.dtype and orth.shape[-1] == n_local
                    n_orth = int(np.prod(orth.shape[:-1])) if len(orth.shape) > 1 else 1
                    lock_p = C.c_void_p(orth.ptr)
                elif orth is not None and len(orth):
                    lock = np.ascontiguousarray(orth, dtype=self.dtype).reshape(-1, n_local)
                    n_orth = lock.shape[0]
                    lock_p = ptr(lock)
                fn = getattr(lib(), "ll_lanczos_run_iteration_" + sfx)
                check(fn(self.context.handle, op.handle, C.byref(p), nroot, n_orth, lock_p, ptr(vals), vecs_p,
                         C.byref(n_found), C.byref(itern), ptr(alpha), ptr(beta), C.byref(stats)))
                counts[0] = itern.value
        finally:
            if owned:
                op.close()
        del keep
        nf = n_found.value
        self._iter_counts = [int(c) for c in counts[: min(stats.n_passes, cap)]]
        self.last_stats = stats.as_dict()
        self.last_alpha, self.last_beta = alpha[: stats.last_alpha_len].copy(), beta[: stats.last_alpha_len].copy()
        return vals[:nf], (vecs if dev_out is not None else vecs[:nf]), int(itern.value)

    def run_two_pass(self, want_vector=True):
        """The extreme eigenpair WITHOUT a stored Krylov basis (two-pass Lanczos, ll_lanczos_two_pass_*): three or four
        n-sized device vectors whatever the iteration count, every operator application twice, no re-orthogonalisation
        (one pair only; num_eigs is not consulted).  Returns (eigenvalue, eigenvector or None, info) with info =
        {"iterations", "residual" (None without the vector), "stats"}.  init_vector and eigenvectors_out act as in run():
        with a DeviceArray in eigenvectors_out the Ritz vector is accumulated there and that array is returned."""
        op, owned = _as_operator(self.mv_mul, self.matrix_size, self.dtype, self.context)
        p = self._params(1)
        keep = self._set_start_vector(p, op)
        vec, vec_p = None, None
        if want_vector:
            dev_out = self.eigenvectors_out
            if dev_out is not None:
                assert dev_out.dtype == self.dtype and dev_out.nbytes >= op.n_local * self.dtype.itemsize
                vec, vec_p = dev_out, C.c_void_p(dev_out.ptr)
            else:
                vec = np.empty(op.n_local, dtype=self.dtype)
                vec_p = ptr(vec)
        trace_cap = int(min(self.max_iteration, 1 << 24))
        alpha, beta = np.zeros(trace_cap), np.zeros(trace_cap)
        val, res, itern, stats = C.c_double(), C.c_double(), C.c_int64(), capi.RunStats()
        try:
            fn = getattr(lib(), "ll_lanczos_two_pass_" + _suffix(self.dtype))
            check(fn(self.context.handle, op.handle, C.byref(p), C.byref(val), vec_p, C.byref(itern), C.byref(res),
                     ptr(alpha), ptr(beta), C.byref(stats)))
        finally:
            if owned:
                op.close()
        del keep
        self._iter_counts = [int(itern.value)]
        self.last_stats = stats.as_dict()
        self.last_alpha, self.last_beta = alpha[: stats.last_alpha_len].copy(), beta[: stats.last_alpha_len].copy()
        info = {"iterations": int(itern.value), "residual": res.value if want_vector else None, "stats": self.last_stats}
        return val.value, vec, info

    def run_single(self):
        """run(eigenvalue, eigenvector): one pair regardless of num_eigs (LL:394-407)."""
        vals, vecs = self.run(num_eigs=1)
        return vals[0], vecs[0]

    def getIterationCounts(self):  # noqa: N802 - reference name (LL:412-414)
        return list(self._iter_counts)


class Exponentiator:
    """lambda_lanczos::Exponentiator<T> (EX:24-211): output = exp(a*A) input by Krylov projection."""

    def __init__(self, mv_mul, matrix_size, dtype=None, context=None):
        self.context = context or (mv_mul.ctx if isinstance(mv_mul, _Operator) else default_context())
        self.dtype = np.dtype(dtype if dtype is not None else getattr(mv_mul, "dtype", np.float64))
        self.mv_mul = mv_mul                                     # EX:41
        self.matrix_size = int(matrix_size)                      # EX:44
        self.max_iteration = int(matrix_size)                    # EX:46,81
        self.eps = _real_eps(self.dtype) * 1e2                   # EX:58
        self.full_orthogonalize = False                          # EX:63
        self.initial_vector_size = 200                           # EX:71
        self.orth_mode = capi.ORTH_CGS_DGKS
        self.last_stats = None

    def _params(self):
        p = capi.ExpoParams()
        check(lib().ll_expo_params_default(C.byref(p), self.matrix_size))
        p.max_iteration = int(self.max_iteration)
        p.eps = float(self.eps)
        p.full_orthogonalize = int(bool(self.full_orthogonalize))
        p.orth_mode = int(self.orth_mode)
        p.initial_vector_size = int(self.initial_vector_size)
        return p

    def _call(self, name, a, input, want_stats, out=None, typed=True):
        op, owned = _as_operator(self.mv_mul, self.matrix_size, self.dtype, self.context)
        sfx = _suffix(self.dtype)
        if isinstance(input, DeviceArray):  # psi stays in HBM: device input, device output (out= or a new DeviceArray)
            assert input.dtype == self.dtype and input.nbytes >= op.n_local * self.dtype.itemsize
            out = out if out is not None else DeviceArray(self.context, (op.n_local,), self.dtype)
            in_p, out_p = C.c_void_p(input.ptr), C.c_void_p(out.ptr)
        else:
            inp = np.ascontiguousarray(input, dtype=self.dtype)
            assert inp.shape[0] == op.n_local, "input size differs from the (local) matrix size (EX:88)"
            out = np.zeros_like(inp)
            in_p, out_p = ptr(inp), ptr(out)
        it = C.c_int64()
        p = self._params()
        stats = capi.RunStats()
        try:
            fn = getattr(lib(), name + sfx if typed else name)
            args = [self.context.handle, op.handle, C.byref(p)]
            args += [float(a)] if typed and sfx in "ds" else [float(np.real(a)), float(np.imag(a))]
            args += [in_p, out_p, C.byref(it)]
            if want_stats:
                args.append(C.byref(stats))
            check(fn(*args))
        finally:
            if owned:
                op.close()
        if want_stats:
            self.last_stats = stats.as_dict()
        return out, it.value

    def run(self, a, input, out=None):
        """Returns (output, iteration_count) (EX:87-173).  A DeviceArray input keeps the vector in HBM (output: `out`,
        which may be `input` itself, or a new DeviceArray)."""
        return self._call("ll_expo_run_", a, input, True, out)

    def run_two_pass(self, a, input, out=None):
        """run() WITHOUT a stored Krylov basis (ll_expo_two_pass): three n-sized device vectors whatever the iteration count (four
        when the output is a host array), every operator application twice; full_orthogonalize must be False.  Same buffer
        conventions and return value as run(); last_stats carries workspace_vectors and replay_mismatches."""
        return self._call("ll_expo_two_pass", a, input, True, out, typed=False)

    def run_two_pass_multi(self, a, input, out=None):
        """run_two_pass for a sequence of times `a` from ONE Krylov space (ll_expo_two_pass_multi, at most 16 per call): pass 1 runs
        once with the stop rule applied to every a[j] on its own, pass 2 once with one accumulator per output.  Returns
        (list of outputs, list of iteration counts m_j); on a device operator each pair is bit for bit what run_two_pass(a[j], input)
        returns, for 2 max(m_j) - 1 operator applications instead of sum(2 m_j - 1).  out: None (host arrays are returned) or a
        sequence with one entry per time, each a DeviceArray (one of them may be `input`), a host array of the run's type, or None
        for a new host array.  last_stats as run_two_pass: total_iterations = max(m_j), workspace_vectors = 3 + host outputs."""
        a = [complex(v) for v in a]
        op, owned = _as_operator(self.mv_mul, self.matrix_size, self.dtype, self.context)
        try:
            if isinstance(input, DeviceArray):
                assert input.dtype == self.dtype and input.nbytes >= op.n_local * self.dtype.itemsize
                keep_in, in_p = input, C.c_void_p(input.ptr)
            else:
                keep_in = np.ascontiguousarray(input, dtype=self.dtype)
                assert keep_in.shape[0] == op.n_local, "input size differs from the (local) matrix size (EX:88)"
                in_p = ptr(keep_in)
            out = [None] * len(a) if out is None else list(out)
            assert len(out) == len(a), "one output per time"
            ptrs = []
            for j, o in enumerate(out):
                if o is None:
                    o = out[j] = np.zeros(op.n_local, dtype=self.dtype)
                if isinstance(o, DeviceArray):
                    assert o.dtype == self.dtype and o.nbytes >= op.n_local * self.dtype.itemsize
                    ptrs.append(o.ptr)
                else:
                    assert o.dtype == self.dtype and o.flags.c_contiguous and o.shape == (op.n_local,)
                    ptrs.append(o.ctypes.data)
            a_reim = np.array([[v.real, v.imag] for v in a], dtype=np.float64).reshape(-1)
            its = (C.c_int64 * max(len(a), 1))()
            p = self._params()
            stats = capi.RunStats()
            check(lib().ll_expo_two_pass_multi(self.context.handle, op.handle, C.byref(p), len(a),
                                               a_reim.ctypes.data_as(C.POINTER(C.c_double)), in_p,
                                               (C.c_void_p * max(len(a), 1))(*ptrs), its, C.byref(stats)))
        finally:
            if owned:
                op.close()
        del keep_in
        self.last_stats = stats.as_dict()
        return out, [int(v) for v in its[: len(a)]]

    def taylor_run(self, a, input, out=None):
        """Returns (output, number_of_terms) (EX:175-210)."""
        return self._call("ll_expo_taylor_run_", a, input, False, out)
