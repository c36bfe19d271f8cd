"""Bits of the propagation-blocked and the 2-D tiled SpMV for two builds of the library: every layout-sensitive form on the
smallest shapes at which each branch of the image planning (csrc/spmv_plan.hpp) runs.

  python tools/spmv_image_ab_bits.py --write DIR        one process = one build (LL_LIB_PATH selects the library): one file of raw
                                                        bytes per case under DIR
  python tools/spmv_image_ab_bits.py --compare A B      byte comparison of two such directories on the host, one line per case

Forms: PB with phase 2 `ordered` (floating-point sums in stream order: an entry that moves changes bits) and `fixed`; the tiled
kernel in both classes.  `atomic` is left out (not reproducible by design).  Matrices: random symmetric, n = 1031, and a band
matrix, n = 2049, in the four storage types.  Plans: automatic blocks, pb_block = 5, pb_row_block = 40 / pb_col_block = 7; pb_pad 4
and 16; pb_diag 0 and 1; tl_force with tl_walk 0 and 1; force_rp64; sharded plans through the stand-in transport
(tests/transport/solo_transport.cpp: ranks 0 and 2 of 3) and through the hook pb_test_all_remote with three gather chunks on one rank.
Per case: two applies (offset 0; offset 0.37 with the fused dot), each as the whole y buffer with one element of slack on either
side (zero-filled before the apply) and the dot as a double."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLO = os.path.join(ROOT, "tests", "transport", "_build", "libll_solo_transport.so")


def cases():
    """(name, matrix, dtype letter, kernel, ordered?, tuning keys, (rank, ranks) or None)"""
    out = []
    for mat in ("rand1031", "band2049"):
        for t in "dzsc":
            for ordered in (False, True):
                form = "ordered" if ordered else "fixed"
                for bname, blocks in (("auto", {}), ("blk5", {"pb_block": 5}), ("r40c7", {"pb_row_block": 40, "pb_col_block": 7})):
                    for pad in (4, 16):
                        for diag in (0, 1):
                            out.append(("%s_%s_pb_%s_%s_pad%d_diag%d" % (mat, t, form, bname, pad, diag), mat, t, "pb", ordered,
                                        dict(blocks, pb_pad=pad, pb_diag=diag), None))
                out.append(("%s_%s_pb_%s_blk5_rp64" % (mat, t, form), mat, t, "pb", ordered, {"pb_block": 5, "force_rp64": 1}, None))
                for bname, blocks in (("auto", {}), ("r40", {"pb_row_block": 40})):
                    for walk in (0, 1):
                        out.append(("%s_%s_tiled_%s_%s_walk%d" % (mat, t, form, bname, walk), mat, t, "tiled", ordered,
                                    dict(blocks, tl_force=1, tl_walk=walk), None))
                out.append(("%s_%s_tiled_%s_r40_rp64" % (mat, t, form), mat, t, "tiled", ordered,
                            {"pb_row_block": 40, "tl_force": 1, "force_rp64": 1}, None))
                # sharded plans
                for rank in (0, 2):
                    for bname, blocks in (("auto", {}), ("blk5", {"pb_block": 5})):
                        out.append(("%s_%s_pb_%s_%s_rank%dof3" % (mat, t, form, bname, rank), mat, t, "pb", ordered, dict(blocks), (rank, 3)))
                    out.append(("%s_%s_tiled_%s_r40_rank%dof3" % (mat, t, form, rank), mat, t, "tiled", ordered,
                                {"pb_row_block": 40, "tl_force": 1}, (rank, 3)))
                for bname, blocks in (("auto", {}), ("blk5", {"pb_block": 5})):
                    out.append(("%s_%s_pb_%s_%s_allremote_chunks3" % (mat, t, form, bname), mat, t, "pb", ordered,
                                dict(blocks, pb_test_all_remote=1, gather_chunks=3), (0, 1)))
    return out


def write(out_dir):
    os.environ.setdefault("LL_COMM_PLUGIN", SOLO)
    sys.path.insert(0, ROOT)
    import numpy as np

    import lambda_lanczos_amd as L
    from lambda_lanczos_amd import capi
    from lambda_lanczos_amd import generators as G

    os.makedirs(out_dir, exist_ok=True)
    dtypes = {"d": np.float64, "z": np.complex128, "s": np.float32, "c": np.complex64}

    class At:  # a device array seen from an element offset
        def __init__(self, arr, off):
            self.ptr = arr.at(off).value

    def matrix(mat, dtype, rb, nl):
        n = 1031 if mat == "rand1031" else 2049
        rp, ci, va = G.randsym_np(n, band=0 if mat == "rand1031" else 60, row_begin=rb, n_local=nl)
        if np.dtype(dtype).kind == "c":
            va = va * (0.8 + 0.6j)
        return rp, ci, va.astype(dtype)

    for name, mat, t, kernel, ordered, keys, shard in cases():
        dtype = dtypes[t]
        n = 1031 if mat == "rand1031" else 2049
        ctx = L.Context(0)
        if shard is not None:
            ctx.init_comm(L.Context.unique_id(), shard[0], shard[1])
        for k, v in keys.items():
            ctx.set_tuning(k, str(v))
        rb, nl = ctx.partition(n) if shard is not None else (0, n)
        op = L.CsrOperator(ctx, *matrix(mat, dtype, rb, nl), n_cols=n, row_begin=rb,
                           accuracy=capi.ACCURACY_COMPONENTWISE if ordered else capi.ACCURACY_NORMWISE,
                           kernel=capi.SPMV_PB if kernel == "pb" else capi.SPMV_TILED)
        assert op.selected_spmv() == (capi.SPMV_PB if kernel == "pb" else capi.SPMV_TILED), name
        x = G.start_vector(nl, 3, np.complex128 if np.dtype(dtype).kind == "c" else np.float64, rb).astype(dtype)
        xd = ctx.to_device(x)
        blob = []
        for offset, want_dot in ((0.0, False), (0.37, True)):
            yd = ctx.to_device(np.zeros(nl + 2, dtype=dtype))
            dot = L.spmv(op, xd, At(yd, 1), offset=offset, want_dot=want_dot)
            blob.append(yd.get().tobytes())
            blob.append(np.float64(dot if want_dot else 0.0).tobytes())
        with open(os.path.join(out_dir, name), "wb") as f:
            f.write(b"".join(blob))
        op.close()
        ctx.close()
    print("%d cases written to %s with %s" % (len(cases()), out_dir, capi.LIB_PATH))


def compare(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)), "the two directories hold different cases"
    total = differ = 0
    for name in names:
        with open(os.path.join(a, name), "rb") as f:
            da = f.read()
        with open(os.path.join(b, name), "rb") as f:
            db = f.read()
        total += len(da)
        differ += da != db
        print("%-48s %7d bytes  sha256 %s  %s" % (name, len(da), hashlib.sha256(da).hexdigest()[:16], "equal" if da == db else "DIFFERENT"))
    print("\n%d case files, %d bytes compared per build, %d files differ%s" % (
        len(names), total, differ, ": every compared byte is equal." if differ == 0 else "."))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        write(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
