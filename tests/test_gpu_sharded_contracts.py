"""The accuracy contracts of include/lanczos_hip.h on SHARDED contexts, against the exact host reference (tests/exact_ref.py):
every operator form that runs other code with more than one rank — the column-split CSR-stream and dense operators, the PB
kernel's own / remote column blocks and chunked gather, the tiled kernel's two passes, the lattice kernels' halos, the padded
all-gather — in all four storage types, on matrices built to break kernels (contract_cases.sharded_edge_matrix: rows on every
shard cut, empty rows, duplicates, rows of more than 1024 entries spread over every rank) and on sizes that leave shards short
or empty.  2, 3 and 4 rank processes share the one GPU through the host-staged test transport (tests/shm_contract_worker.py);
each launch runs once per module and the parametrised tests read its records.

Per form, type and world: the bound of the accuracy class against the correctly rounded A x; for float / complex float the
sharper storage contract (split forms: two partial sums, each rounded to T once, added in T — exact_ref.split_storage_bound);
alpha identical on every rank and within dot_bound of the exact Re<x, y>; the fixed-point forms bit for bit the single-context
product in every world and gather / block geometry; overlapped and serial issue order bit for bit.

tiled_layout at n = 5003: every rank has row blocks that wait for the gather (own < nrb); a rank has row blocks that do not
(own > 0) exactly where a row block's entries all fall into column tiles that lie whole inside the rank's columns.  A tile is
16 KiB of x — 4096 columns in float, 2048 in double and complex float, 1024 in complex double — so a shard of 1668 columns
holds a whole tile only in complex double or at the ragged end of the matrix; _expected_own_blocks works it out per type and
rank from the matrix."""
import json
import os
import re
import subprocess
import sys
import time
import uuid

import numpy as np
import pytest

import contract_cases as K
import exact_ref as E
import lambda_lanczos_amd as L
import shm_contract_worker as W
from conftest import SHM_TRANSPORT
from lambda_lanczos_amd import _capi as capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_IDS = list(W.TYPES)
OFFSETS = W.OFFSETS
LAUNCHES = {"w2": (2, {}), "w3": (3, {}), "w4": (4, {}), "w2_serial": (2, {"LL_COMM_OVERLAP": "0"})}
_RECORDS, _REF, RATIOS = {}, {}, {}


# ------------------------------------------------------------------ the launches (once per module)
def _launch(tag, tmp_root):
    """Start the rank processes of one launch and load their records.  No retries: a rank that exits non-zero fails the caller
    with its output; every communicate has the time limit of test_gpu_multirank.run_ranks."""
    world, extra = LAUNCHES[tag]
    out_dir = os.path.join(tmp_root, tag)
    os.makedirs(out_dir, exist_ok=True)
    name = "/ll_shm_test_" + uuid.uuid4().hex[:12]
    env = dict(os.environ, LL_COMM_PLUGIN=SHM_TRANSPORT, OMP_NUM_THREADS="2", **extra)
    for k in W.MANAGED:
        env.pop(k, None)
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "shm_contract_worker.py"), str(r), str(world), name,
                               out_dir], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-4000:]
    ranks = []
    for r in range(world):
        with np.load(os.path.join(out_dir, "rank%d.npz" % r)) as z:
            ranks.append({k: z[k] for k in z.files})
        ranks[-1]["meta"] = json.loads(str(ranks[-1]["meta"]))
    print("launch %s: %d ranks, %.1f s wall (%.1f s inside rank 0)" % (tag, world, time.time() - t0, ranks[0]["meta"]["seconds"]))
    return ranks


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("sharded_contracts"))

    def get(tag):
        if tag not in _RECORDS:
            _RECORDS[tag] = None           # a launch that failed is not started again by the next test
            _RECORDS[tag] = _launch(tag, root)
        assert _RECORDS[tag] is not None, "the %s launch failed in an earlier test" % tag
        return _RECORDS[tag]

    return get


def _meta(ranks, key, t):
    return [r["meta"][key + ":" + t] for r in ranks]


def _stitch(ranks, key, t, si, oi):
    return np.concatenate([r[key + ":" + t + ":y"][si, oi] for r in ranks])


def _alpha(ranks, key, t):
    """alpha (shift, offset) — after asserting that every rank holds the same bits (one all-reduce, replicated)."""
    a = ranks[0][key + ":" + t + ":alpha"]
    for r in ranks[1:]:
        assert np.array_equal(a.view(np.uint8), r[key + ":" + t + ":alpha"].view(np.uint8)), (key, t, "alpha differs between ranks")
    return a


def _expected_shards(n, world):
    stride = -(-n // world)
    return [min(n, stride * (r + 1)) - min(n, stride * r) for r in range(world)]


# ------------------------------------------------------------------ references (computed once, shared, never changed)
def _ref(kind, name, size, t):
    key = (kind, name if kind == "lattice" else None, size, t)
    if key not in _REF:
        inp = W.inputs(kind, name, size, t)
        ex = E.rows_exact(inp["csr"], inp["x"])
        sp = E.rows_storage_products(inp["csr"], inp["x"], W.TYPES[t]) if W._single(W.TYPES[t]) and kind == "csr" else None
        _REF[key] = (inp, ex, sp)
    return _REF[key]


def _split_ref(kind, size, t, world):
    """exact_ref.split_rows of the case on `world` ranks: CSR-stream goes by the > 1024 rule per part, dense forms every product exactly."""
    key = ("split", kind, size, t, world)
    if key not in _REF:
        inp = W.inputs(kind, None, size, t)
        _REF[key] = E.split_rows(inp["csr"], inp["x"], W.TYPES[t], world, 1024 if kind == "csr" else -1)
    return _REF[key]


def _eps(dtype):
    return E.EPS_F if W._single(dtype) else E.EPS_D


def _check(label, t, world, inp, ex, y, alpha, offset, fixed, storage):
    """Class bound, storage contract (s / c; storage = (target Rows, per-row split mask or None, (own, rem) or None)) and alpha.
    Returns the error / bound ratios (class, storage, alpha)."""
    dtype = W.TYPES[t]
    x = inp["x"]
    xw = x.astype(np.complex128 if np.dtype(dtype).kind == "c" else np.float64)
    cls = E.class_bound(ex, x, y, offset, _eps(dtype), fixed)
    errs = E.part_errors(y, ex.y + offset * xw)
    ok, r_cls = E.within(errs, (cls, cls))
    print("  %s %s world %d offset %g: class ratio %.3g" % (label, t, world, offset, r_cls))
    assert ok, "%s: class bound violated (ratio %.3g)" % (label, r_cls)
    r_sto = 0.0
    if W._single(dtype):
        rows, split_mask, parts = storage
        xmax = float(np.max(E.abs1(x))) if x.size else 0.0
        sb = E.storage_bound(y, x, offset, dtype, E.double_sum_error(rows, fixed_point=fixed, xmax=xmax))
        target = rows.y
        if parts is not None:
            own, rem = parts
            ssb = E.split_storage_bound(y, x, offset, dtype, own, rem, E.double_sum_error(own), E.double_sum_error(rem))
            sb = tuple(None if a is None else np.where(split_mask, b, a) for a, b in zip(sb, ssb))
            target = np.where(split_mask, own.y + rem.y, target)
        ok, r_sto = E.within(E.part_errors(y, target + offset * xw), sb)
        print("  %s %s world %d offset %g: storage ratio %.3g" % (label, t, world, offset, r_sto))
        assert ok, "%s: storage-product contract violated (ratio %.3g)" % (label, r_sto)
    # alpha = Re<x, y> of the RETURNED y over the whole vector, the ranks' partial sums joined by one all-reduce.  Inside a rank
    # the sum is what dot_bound describes, over n_local <= n products.  The all-reduce adds P - 1 times; every one of these
    # additions rounds a partial sum that is bounded by sum |x_i||y_i|, so each costs at most eps_d sum |x_i||y_i|.  The + 8 of
    # dot_bound allows 2 * 8 eps_d = 16 eps_d sum |x_i||y_i|: room for P - 1 <= 3 here (and up to 16) on top of the
    # single-context sum, whose n term is not used up by a shard of n_local < n products.  An empty shard adds an exact zero.
    d = E.dot_exact(x, y)
    db = E.dot_bound(x, y)
    print("  %s %s world %d offset %g: alpha ratio %.3g" % (label, t, world, offset, abs(alpha - np.real(d)) / db))
    assert abs(alpha - np.real(d)) <= db, (label, alpha, d, db)
    return r_cls, r_sto, abs(alpha - np.real(d)) / db


def _expected_own_blocks(csr, row_begin, n_local, dtype, rb_rows):
    """(row blocks, those whose entries all fall into column tiles lying whole inside the rank's columns) of the tiled image of
    one rank: tiles of 16 KiB of x from column 0, the last one ragged; a row block without entries needs no other rank either."""
    rp, ci, _ = csr
    n = rp.shape[0] - 1
    width = 16384 // np.dtype(dtype).itemsize
    lo, hi = row_begin, row_begin + n_local
    nrb, own = -(-n_local // rb_rows), 0
    for b in range(nrb):
        r0 = lo + b * rb_rows
        tiles = np.unique(ci[rp[r0]:rp[min(hi, r0 + rb_rows)]].astype(np.int64) // width)
        own += bool(np.all((tiles * width >= lo) & (np.minimum(tiles * width + width, n) <= hi)))
    return nrb, own


def _note(family, t, r):
    RATIOS[(family, t)] = tuple(max(a, b) for a, b in zip(RATIOS.get((family, t), (0.0, 0.0, 0.0)), r))


def _family(name):
    return re.sub(r"(_g\d+)?(_b37)?(_rp64)?$", "", name)


# ------------------------------------------------------------------ CSR operators: CSR-stream (split / gather), PB, tiled
CSR_FORMS = W.csr_forms()


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("t", TYPE_IDS)
@pytest.mark.parametrize("form", list(CSR_FORMS))
def test_sharded_csr_operator_meets_its_contract(records, form, t, world):
    ranks = records("w%d" % world)
    kernel, _, _, fixed, split = CSR_FORMS[form]
    dtype = W.TYPES[t]
    for n in ([W.CSR_N] if world in (2, 3) else []) + W.TINY:
        key = "csr:%s:%d" % (form, n)
        meta = _meta(ranks, key, t)
        inp, ex, sp = _ref("csr", None, n, t)
        assert [m["n_local"] for m in meta] == _expected_shards(n, world)      # sums to n; the expected shards are short / empty
        local_nnz = [int(inp["csr"][0][m["row_begin"] + m["n_local"]] - inp["csr"][0][m["row_begin"]]) for m in meta]
        if kernel == capi.SPMV_TILED and min(local_nnz) == 0:
            # asked for by name, the tiled kernel is an error where a rank has no entries to tile — on every rank, never a fallback
            assert all("tiled" in m.get("refused", "") for m in meta), (key, meta)
            continue
        assert all("refused" not in m for m in meta), (key, meta)
        assert all(m["selected"] == kernel for m in meta), (key, [m["selected"] for m in meta])
        if kernel == capi.SPMV_TILED and n == W.CSR_N:
            # row blocks: 16 rows for shards this small, LL_PB_ROW_BLOCK=37 rounded up to an even 38
            want = [_expected_own_blocks(inp["csr"], m["row_begin"], m["n_local"], dtype, 38 if form.endswith("_b37") else 16) for m in meta]
            print("  %s %s world %d: tiled_layout %s, from the matrix %s" % (key, t, world, [m["layout"] for m in meta], want))
            assert all(0 <= m["layout"][1] < m["layout"][0] for m in meta), (key, [m["layout"] for m in meta])
            assert [m["layout"][1] > 0 for m in meta] == [w[1] > 0 for w in want], (key, [m["layout"] for m in meta], want)
            assert any(w[1] > 0 for w in want)
        if kernel == capi.SPMV_PB:
            # the phase-2 form that was asked for is the one that runs: fixed point is the norm-wise class, ordered / atomic are not
            want_acc = capi.ACCURACY_NORMWISE if fixed else capi.ACCURACY_COMPONENTWISE
            assert all(m["accuracy"] == want_acc for m in meta), (key, [m["accuracy"] for m in meta])
            if n == W.CSR_N and form.endswith("_b37"):
                # ... and the block hook took effect: blocks of 37 columns and rows need other tables than the default geometry
                other = _meta(ranks, "csr:%s:%d" % (form[:-4], n), t)
                assert all(a["device_bytes"] != b["device_bytes"] for a, b in zip(meta, other)), (meta, other)
        if form == "csr_split" and n == W.CSR_N:
            # the column-split image is a second copy of the rank's matrix next to the kept CSR arrays; LL_CSR_SPLIT=0 builds none
            other = _meta(ranks, "csr:csr_gather:%d" % n, t)
            assert all(a["device_bytes"] > b["device_bytes"] for a, b in zip(meta, other)), (meta, other)
        storage = None
        if W._single(dtype):
            long_rows = ex.nnz > 1024 if kernel == capi.SPMV_CSR_STREAM else np.zeros(n, dtype=bool)
            rows = E.Rows(np.where(long_rows, ex.y, sp.y), ex.absrow, ex.rowsum, ex.nnz)
            storage = (rows, np.ones(n, dtype=bool), _split_ref("csr", n, t, world)) if split else (rows, None, None)
        alpha = _alpha(ranks, key, t)
        first = {}
        for si, shift in enumerate(W.SHIFTS):
            for oi, offset in enumerate(OFFSETS):
                y = _stitch(ranks, key, t, si, oi)
                _note(_family(form), t, _check(key, t, world, inp, ex, y, alpha[si, oi], offset, fixed, storage))
                if "atomic" not in form:   # a fixed order: the same bits for any placement of x / y
                    assert np.array_equal(first.setdefault(oi, y).view(np.uint8), y.view(np.uint8)), (key, shift, offset)
                if split:
                    # column split and gather-then-multiply round differently (two partial sums against one): they agree to
                    # within the class bound, not bit for bit
                    g = _stitch(ranks, key.replace("csr_split", "csr_gather"), t, si, oi)
                    cls = E.class_bound(ex, inp["x"], y, offset, _eps(dtype), False)
                    assert E.within(E.part_errors(y, g), (cls, cls))[0], (key, offset)


@pytest.mark.parametrize("t", TYPE_IDS)
def test_fixed_point_forms_stitch_to_the_bits_of_the_single_context_product(records, ctx, llenv, t):
    """PB `fixed` and tiled `fixed`: the same bits on 2, 3 and 4 ranks, for every LL_GATHER_CHUNKS / block setting, as ONE context
    applying the whole matrix (the grid's scale is max |x| over the whole vector, the sums are integers)."""
    dtype = W.TYPES[t]
    llenv.setenv("LL_TL_FORCE", "1")
    compared = 0
    for n in [W.CSR_N] + W.TINY:
        inp, _, _ = _ref("csr", None, n, t)
        x = inp["x"]
        single = {}
        for kernel in (capi.SPMV_PB, capi.SPMV_TILED):
            op = L.CsrOperator(ctx, *inp["csr"], accuracy=capi.ACCURACY_NORMWISE, kernel=kernel)
            assert op.selected_spmv() == kernel
            xd, yd = ctx.to_device(x), ctx.empty(n, dtype)
            for oi, offset in enumerate(OFFSETS):
                L.spmv(op, xd, yd, offset=offset)
                single[(kernel, oi)] = yd.get()
            xd.free()
            yd.free()
            op.close()
        for oi in range(len(OFFSETS)):
            assert np.array_equal(single[(capi.SPMV_PB, oi)].view(np.uint8), single[(capi.SPMV_TILED, oi)].view(np.uint8))
        for world in (2, 3, 4):
            if n == W.CSR_N and world == 4:
                continue
            ranks = records("w%d" % world)
            for form, spec in CSR_FORMS.items():
                key = "csr:%s:%d" % (form, n)
                if not spec[3] or "refused" in _meta(ranks, key, t)[0]:
                    continue
                for si in range(len(W.SHIFTS)):
                    for oi in range(len(OFFSETS)):
                        y = _stitch(ranks, key, t, si, oi)
                        assert np.array_equal(y.view(np.uint8), single[(capi.SPMV_PB, oi)].view(np.uint8)), (key, world, si, oi)
                        compared += 1
    assert compared >= 2 * 6 * 6   # n = 5003: six fixed-point forms on two worlds, at least


def test_overlapped_and_serial_issue_order_give_the_same_bits(records):
    """LL_COMM_OVERLAP=0 issues the same kernels behind the exchange on one stream: every y and every alpha of the 2-rank launch
    bit for bit, for every form except PB's atomic one (floating-point adds in arrival order)."""
    a, b = records("w2"), records("w2_serial")
    compared = 0
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for k in ra:
            if k == "meta" or "atomic" in k:
                continue
            assert np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), k
            compared += 1
        for k, m in ra["meta"].items():
            if k != "seconds":
                assert {f: v for f, v in m.items() if f != "device_bytes"} == {f: v for f, v in rb["meta"][k].items() if f != "device_bytes"}, k
    assert compared > 500


# ------------------------------------------------------------------ dense row blocks
def _dense_split_mask(n, world, dtype, variant):
    """Rows whose rank takes the column-split form: the shard's column range must start and end on 16-byte pieces of the rows
    (Engine::apply: otherwise both parts would take the scalar loads, and gather-then-multiply is used).  Decided per rank."""
    v = max(1, 16 // np.dtype(dtype).itemsize)
    col0, col1 = E.owner_ranges(n, world)
    return (n % v == 0) & (col0 % v == 0) & (col1 % v == 0) & (variant == "split")


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("t", TYPE_IDS)
@pytest.mark.parametrize("variant", ["split", "gather"])
def test_sharded_dense_operator_meets_its_contract(records, variant, t, world):
    ranks = records("w%d" % world)
    dtype = W.TYPES[t]
    for n in {2: [1027, 1040], 3: [1027, 1040, 3]}[world]:
        key = "dense:%s:%d" % (variant, n)
        meta = _meta(ranks, key, t)
        assert [m["n_local"] for m in meta] == _expected_shards(n, world)
        inp, ex, _ = _ref("dense", None, n, t)
        mask = _dense_split_mask(n, world, dtype, variant)
        if n == 1040 and world == 2:
            assert variant != "split" or mask.all()       # cut at 520: the split form with vector loads, for every type
        if n == 1027 and np.dtype(dtype).itemsize < 16:
            assert not mask.any()                          # odd n: gather-then-multiply
        storage = (ex, mask, _split_ref("dense", n, t, world) if mask.any() else None) if W._single(dtype) else None
        if storage is not None and storage[2] is None:
            storage = (ex, None, None)
        alpha = _alpha(ranks, key, t)
        differ = 0
        for si in range(len(W.SHIFTS)):
            for oi, offset in enumerate(OFFSETS):
                y = _stitch(ranks, key, t, si, oi)
                _note("dense_" + variant, t, _check(key, t, world, inp, ex, y, alpha[si, oi], offset, False, storage))
                if variant == "split":
                    g = _stitch(ranks, key.replace("split", "gather"), t, si, oi)
                    cls = E.class_bound(ex, inp["x"], y, offset, _eps(dtype), False)
                    assert E.within(E.part_errors(y, g), (cls, cls))[0], (key, offset)
                    differ += int(np.count_nonzero(y != g))
        if variant == "split" and n == 1040 and world == 2 and W._single(dtype):
            # the split path really ran: two partial sums rounded to float and added in float cannot give the bits of one sum
            # rounded once on all 1040 rows x 6 applies (a dense operator that quietly gathered first would)
            print("  %s %s: %d elements differ between the column-split and the gather-then-multiply form" % (key, t, differ))
            assert differ > 0, key


# ------------------------------------------------------------------ lattice operators (halo exchange)
LATTICE_CASES = [(name, world) for world, names in ((2, ["37x64_periodic", "37x64_open", "5x8x8_mixed", "2x8x8_periodic"]),
                                                    (3, ["37x64_periodic", "37x64_open", "5x8x8_mixed"]), (4, ["4x8x8_periodic"]))
                 for name in names]


@pytest.mark.parametrize("t", TYPE_IDS)
@pytest.mark.parametrize("vec", ["1", "0"], ids=["vec", "scalar"])
@pytest.mark.parametrize("name,world", LATTICE_CASES)
def test_sharded_lattice_operator_meets_its_contract(records, name, world, vec, t):
    ranks = records("w%d" % world)
    dtype = W.TYPES[t]
    dims = W.LATTICES[name][0]
    n = int(np.prod(dims))
    key = "lattice:%s:vec%s" % (name, vec)
    meta = _meta(ranks, key, t)
    assert [m["n_local"] for m in meta] == _expected_shards(n, world)
    if name in ("2x8x8_periodic", "4x8x8_periodic"):
        assert all(m["n_local"] == 64 for m in meta)       # one hyperplane per rank: the halo is the whole neighbouring shard
    inp, ex, _ = _ref("lattice", name, dims, t)
    storage = (ex, None, None) if W._single(dtype) else None   # every product exact in double
    alpha = _alpha(ranks, key, t)
    other = "lattice:%s:vec%s" % (name, "0" if vec == "1" else "1")
    for si in range(len(W.SHIFTS)):
        for oi, offset in enumerate(OFFSETS):
            y = _stitch(ranks, key, t, si, oi)
            _note("lattice_" + ("vec" if vec == "1" else "scalar"), t, _check(key, t, world, inp, ex, y, alpha[si, oi], offset, False, storage))
            # the vectorised and the scalar kernel add a site's terms in the same order: identical bits
            assert np.array_equal(y.view(np.uint8), _stitch(ranks, other, t, si, oi).view(np.uint8)), (key, si, oi)


def test_report_the_worst_ratios(records):
    """The largest error / bound ratio per form and type over every world, size, offset and pointer shift (the bounds are
    derived in exact_ref.py, the ratios are what this run measured)."""
    for tag in LAUNCHES:
        records(tag)
    print("worst error / bound ratios: form type class storage alpha")
    for (family, t), r in sorted(RATIOS.items()):
        print("RATIO %-14s %s %.3g %.3g %.3g" % ((family, t) + r))
