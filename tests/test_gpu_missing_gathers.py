"""The missing-call index lists and gather kernels of the exact-integer mode (csrc/missing_kernels.hip: k_count_missing, k_fill_missing,
k_sparse_rows_sum, k_sparse_rows_sum_batched, k_sparse_rows_sum_short; dispatch in csrc/missing_routes.hip) at the shapes where they can
go wrong, every comparison exact or with a derived bound.

What makes exact comparison possible:
 * a gather of integer-valued rows is exact whatever the order of summation: fp64 values are held to |v| <= 2^20, fp32 values to 2^12
   and widened before they are added, colw is a power of two and x 32 is exact -- the kernels are compared bit for bit with int64 numpy;
 * X'B (K2) on an integer block in [-4, 4] is a function of exact integers on every route (k_i8_combine forms (g - mean (1'B - E'B)) / sd,
   and E'B is the same integer whether it comes from the E partials, from the gathered plane or from the hybrid route's small GEMM), so
   routes 4 (hybrid), 3 (gathers), 1 (block skipping) and 0 (both matrices) return the same bits, under every forced gather kernel and
   at 4 slices, where the gathers read fp32 rows.  X T (K3) has no such identity (the gathers read the unsliced mean T / sd, the
   two-matrix kernels its slices): it is held to the tolerance of test_i8_mode_operator_parity, and the exactness of its kernels comes
   from the direct hook.

Checks:
 a. fpca_debug_gather (the very kern::sparse_rows_sum / sparse_rows_sum_f32 the operator calls, reached through short_lists / avg_len
    as the operator reaches them; each case asserts the kernel that ran): 16 / 32 / 64 columns, fp64 and fp32 rows, with and without
    init, all three kernels, on lists of 0, 1, EPW - 1, EPW, 4 EPW - 1, 4 EPW, 4 EPW + 1, 8 EPW +- 1, 63, 64, 65, 128, 129 and 1000
    entries (EPW = 64 / b: the unroll of the plain kernel, the 8-deep batches of the batched one, its 64-entry index reads), indices
    0 and v_rows - 1, repeats across lists, every residue of the 4 EPW unroll; the short kernel on 0, 1, 3, 4, 5, B - 1, B, B + 1, 2 B + 3
    (and 2, 6, B + 2, 2 B + 2: the batch sizes 2 mod 4 the list leaves out) entries with the groups of a wave
    all different, the longest list in the last group and a wave of empty groups; nrec no multiple of 4 or 4 (64 / B), nrec = 1, rows_out >
    nrec (pad rows = init or 0); the grid-stride pass behind the 65,536-block cap; a different power-of-two colw per column; fp64 rowscale
    (kernels 1 and 2); 64 columns never take kernel 3.  The output buffer is NaN before every launch.
 b. fpca_debug_missing_lists == np.nonzero of the decoded matrix, entry for entry, by SNP and by sample, on records of 16,450 codes (two
    steps of k_fill_missing and a ragged last piece) in the band-tiled layout and with FPCA_I8_TILED=0; on the hybrid view the dense
    SNPs -- those of the CPU port of the cost model -- have empty lists and appear in no sample's list.
 c. K2 across routes 4, 3, 1, 0 x b 16 / 32 / 64 x S 7 / 4 x FPCA_GATHER unset / 1 / 2 / 3 on both matrices: all bit-identical, within 4 u
    (|g| + |mean m|) / sd of the longdouble value of int64 g, m (the bound test_gpu_i8_plan.py derives), exactly 0 where sd <= 1e-9.
 d. K3 and the full apply on routes 4 and 3 against the dense matrix at 10 x 1e-12 (S = 7) / 10 x 3e-6 (S = 4); K3 takes the short
    kernel on the tall matrix (1.2 listed calls per sample) and the batched one on the wide one; with FPCA_SPARSE_SIDE_BYTES=1 (both
    stages gather on the side stream), also in three row chunks behind a one-rank communicator, the same bits as inline.
Every product is called with A, A2, A: the third result equals the first and differs from the second.  The matrices, the routes and the
kernels of every case are checked without a device in tests/test_missing_gathers_cpu.py.

Measured on the MI355X (profiles/missing_gather_test_figures.txt): every gather case bit-identical with the kernel it asks for (64 columns
asking for kernel 3 run kernel 2); the lists equal entry for entry, 5 / 7 dense SNPs on the tall matrix at 7 / 4 slices, 125 / 2141 on the
wide one; K2 one bit pattern per matrix and width, at most 0.49 of the bound; K3 and the apply at most 1.4e-15 (S = 7) and 1.9e-8 (S = 4);
the side stream bit-identical.  74 tests in 25 s."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_missing_gathers_cpu as M  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- a. the gather kernels on caller data -------------------------------------------------------------------
REACH = {1: (False, 0.0), 2: (True, 0.0), 3: (True, 12.0)}  # (short_lists, avg_len) as K2 / K3 / K3 on short lists pass them


def _lists(lengths, v_rows, rng):
    """Lists of the given lengths: ascending indices below v_rows, 0 and v_rows - 1 among them, rows shared between lists."""
    lengths = np.asarray(lengths, dtype=np.int64)
    ptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=ptr[1:])
    idx = np.zeros(ptr[-1], dtype=np.int64)
    for r in np.nonzero(lengths)[0]:
        n = int(lengths[r])
        pick = np.sort(rng.choice(v_rows, size=n, replace=n > v_rows))
        if n >= 2:
            pick[0], pick[-1] = 0, v_rows - 1
        elif n == 1:
            pick[0] = (0, v_rows - 1)[r % 2]
        idx[ptr[r]:ptr[r + 1]] = pick
    return ptr, idx


def _operand(v_rows, b, f32, rng):
    lim = 2 ** 12 if f32 else 2 ** 20
    Vi = rng.integers(-lim, lim + 1, size=(v_rows, b))
    Vi[0], Vi[-1] = lim, -lim
    return Vi, Vi.astype(np.float32 if f32 else np.float64)


def _gather_case(fp, b, f32, lengths, kernel, rows_out=None, with_init=False, rowscale=False, v_rows=301, seed=0, label=""):
    rng = np.random.default_rng(seed * 1000 + b)
    nrec = len(lengths)
    rows_out = nrec if rows_out is None else rows_out
    ptr, idx = _lists(lengths, v_rows, rng)
    Vi, V = _operand(v_rows, b, f32, rng)
    assert np.array_equal(V.astype(np.int64), Vi)
    rs_exp = rng.integers(-3, 4, size=v_rows) if rowscale else None
    rs = None if rs_exp is None else 2.0 ** rs_exp
    colw = 2.0 ** (np.arange(b) % 23 - 11.0) if f32 else None  # a different power of two per column (the same for c and c + 23)
    init_i = rng.integers(-2 ** 20, 2 ** 20 + 1, size=(rows_out, b)) if with_init else None
    short_lists, avg_len = REACH[kernel]
    want_kernel = M.gather_variant(b, rowscale, short_lists, avg_len)
    out, variant = fp.api.debug_gather(ptr, idx, V, b, rows_out=rows_out, rowscale=rs, colw=colw, init=None if init_i is None else init_i.astype(np.float64),
                                       short_lists=short_lists, avg_len=avg_len)
    # int64 reference; a per-row factor 2^k, k >= -3, is applied as an integer after scaling everything by 8
    rows = np.repeat(np.arange(nrec), np.diff(ptr))
    acc = np.zeros((rows_out, b), dtype=np.int64)
    np.add.at(acc, rows, Vi[idx] * (2 ** (rs_exp[idx] + 3))[:, None] if rowscale else Vi[idx])
    assert np.max(np.abs(acc)) < 2 ** 52
    ref = acc.astype(np.float64)
    if rowscale:
        ref /= 8.0
    if f32:
        ref *= (colw * 32.0)[None, :]
    if with_init:
        ref += init_i.astype(np.float64)  # (an integer below 2^21 plus a multiple of 2^-6 below 2^53: exact)
    assert float(np.max(np.abs(ref))) < 2 ** 46
    ok = bool(np.array_equal(out, ref))
    print("gather %-14s b %2d %s init %d rowscale %d rows %d / %d calls %d kernel %d (asked %d) bit-identical %s"
          % (label, b, "fp32" if f32 else "fp64", with_init, rowscale, nrec, rows_out, idx.size, variant, kernel, ok))
    assert variant == want_kernel and (variant == kernel or (b == 64 and kernel == 3 and variant == 2)), (variant, kernel)
    assert np.isfinite(out).all(), "rows the kernel did not write: %s" % np.nonzero(~np.isfinite(out).all(axis=1))[0][:8]
    bad = np.nonzero((out != ref).any(axis=1))[0]
    assert ok, (label, b, kernel, "rows", bad[:8], "lengths", [lengths[r] if r < nrec else -1 for r in bad[:8]])
    return variant


def _edge_lengths(b):
    """The lengths around every batch size of the three kernels, and every residue of the plain kernel's unroll (4 EPW entries per step:
    each of its three tail predicates decides for one residue class only); the count is no multiple of 4."""
    e = 64 // b
    L = [0, 1, e - 1, e, 4 * e - 1, 4 * e, 4 * e + 1, 8 * e - 1, 8 * e + 1, 63, 64, 65, 128, 129, 1000] + list(range(4 * e + 2, 8 * e - 1))
    while len(L) % 4 != 3:
        L.append(2)
    return L


@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("b", [16, 32, 64])
def test_gather_edge_lengths(built_lib, b, f32, with_init, kernel):
    """Lists around every batch size of the three kernels (their number no multiple of 4, 8 or 16), six output rows behind the last
    list: the pad rows are init or 0."""
    import flashpca_amd as fp

    lengths = _edge_lengths(b)
    assert len(lengths) % 4 and {r % (256 // b) for r in lengths} == set(range(256 // b))
    v = _gather_case(fp, b, f32, lengths, kernel, rows_out=len(lengths) + 6, with_init=with_init, seed=1, label="edges")
    if b == 64:
        assert v != 3  # no several-rows-per-wave kernel for 64 columns: avg_len <= 24 lands on the batched one


def _short_lengths(B):
    L = 2 * B + 3
    if B == 16:  # four groups per wave
        return [1, 0, 5, L, 0, 0, 0, 0, B - 1, B, 3, B + 1, 4, B + 1, 0, L, 2, 6, B + 2, L - 1, 3, 1, L]
    return [1, L, 0, 0, 5, B + 1, B - 1, B, 3, 4, 0, L, B, 1, 2, 6, B + 2, L - 1, L]  # two groups per wave


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("b", [16, 32])
def test_gather_short_kernel_groups(built_lib, b, f32, with_init):
    """The several-rows-per-wave kernel: the groups of a wave run different numbers of B-entry batches (the shuffles are executed by all
    lanes), the longest list sits in the last group of its wave, one wave has only empty groups, and the last wave is partly behind nrec."""
    import flashpca_amd as fp

    lengths = _short_lengths(b)
    G = 64 // b
    waves = [lengths[i:i + G] for i in range(0, len(lengths), G)]
    assert any(len(set(w)) == G for w in waves if len(w) == G) and any(not any(w) for w in waves) and len(waves[-1]) < G
    assert any(len(w) == G and w[-1] == max(lengths) for w in waves) and len(lengths) % 4 and len(lengths) % (4 * G)
    assert {0, 1, 3, 4, 5, b - 1, b, b + 1, 2 * b + 3} <= set(lengths) and {n % b % 4 for n in lengths} == {0, 1, 2, 3}  # (every tail predicate)
    assert _gather_case(fp, b, f32, lengths, 3, rows_out=len(lengths) + 3, with_init=with_init, seed=2, label="short groups") == 3
    for k in (1, 2):  # the same lists through the other two kernels
        _gather_case(fp, b, f32, lengths, k, rows_out=len(lengths) + 3, with_init=with_init, seed=2, label="short groups")


@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("b", [16, 32, 64])
def test_gather_one_record(built_lib, b, kernel):
    """nrec = 1, alone and in front of eight pad rows."""
    import flashpca_amd as fp

    for rows_out, with_init in ((1, False), (9, True), (9, False)):
        for f32 in (False, True):
            _gather_case(fp, b, f32, [2 * b + 3], kernel, rows_out=rows_out, with_init=with_init, seed=3, label="one record")


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("b", [16, 32, 64])
def test_gather_rowscale(built_lib, b, kernel):
    """The per-row factor of the fp64 gathers (powers of two).  A factor selects the batched kernel on its own; the plain kernel takes one
    only when it is forced (FPCA_GATHER=1, read once per process): that case runs on the test build in a process of its own."""
    import flashpca_amd as fp

    if kernel == 2:
        for short_lists, avg_len in ((False, 0.0), (True, 12.0)):  # (asking for the short kernel with a factor gives the batched one too)
            assert M.gather_variant(b, True, short_lists, avg_len) == 2
        _gather_case(fp, b, False, _edge_lengths(b), 2, rows_out=len(_edge_lengths(b)) + 2, with_init=True, rowscale=True, seed=4, label="rowscale")
        return
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    env["FPCA_GATHER"] = "1"
    r = subprocess.run([sys.executable, "-c", _ROWSCALE_CHILD, ROOT, str(b)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    print(r.stdout.strip())
    assert "ROWSCALE-OK kernel 1" in r.stdout


_ROWSCALE_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import flashpca_amd as fp
import test_gpu_missing_gathers as G
b = int(sys.argv[2])
with fp.test_hooks():
    for with_init in (False, True):
        rng = np.random.default_rng(b)
        lengths = G._edge_lengths(b)
        ptr, idx = G._lists(lengths, 301, rng)
        Vi, V = G._operand(301, b, False, rng)
        e = rng.integers(-3, 4, size=301)
        rows_out = len(lengths) + 2
        init = rng.integers(-2 ** 20, 2 ** 20, size=(rows_out, b)) if with_init else None
        out, variant = fp.api.debug_gather(ptr, idx, V, b, rows_out=rows_out, rowscale=2.0 ** e, init=None if init is None else init.astype(np.float64))
        acc = np.zeros((rows_out, b), dtype=np.int64)
        np.add.at(acc, np.repeat(np.arange(len(lengths)), np.diff(ptr)), Vi[idx] * (2 ** (e[idx] + 3))[:, None])
        ref = acc.astype(np.float64) / 8.0 + (0.0 if init is None else init.astype(np.float64))
        assert variant == 1, variant
        assert np.array_equal(out, ref), np.nonzero((out != ref).any(axis=1))[0]
print("ROWSCALE-OK kernel 1 b %d" % b)
"""


@pytest.mark.parametrize("kernel", [1, 2, 3])
def test_gather_grid_stride(built_lib, kernel):
    """More output rows than the 65,536-block grid covers in one pass (4 rows per block; 16 for the short kernel at 16 columns): most
    lists are empty, a few sit at both ends of the first pass and in the second."""
    import flashpca_amd as fp

    per_block = 16 if kernel == 3 else 4
    rows_out = per_block * 65536 + (37 if kernel == 3 else 5)
    nrec = rows_out - 1
    first = per_block * 65536
    lengths = np.zeros(nrec, dtype=np.int64)
    for r, n in ((0, 3), (7, 65), (first - 1, 17), (first, 9), (first + 1, 64), (first + 3, 1), (nrec - 1, 33)):
        lengths[r] = n
    _gather_case(fp, 16, False, list(lengths), kernel, rows_out=rows_out, with_init=kernel != 3, seed=5, label="grid stride")


# ---- b. the lists ------------------------------------------------------------------------------------------------
def _check_lists(ctx, b, mask, what):
    """Both list sets of the context against np.nonzero of the mask [P][N]."""
    n = 0
    for by_sample, m in ((False, mask), (True, mask.T)):
        ptr, idx = ctx.missing_lists(b, by_sample)
        rptr, ridx = M.csr_of(m)
        same = bool(np.array_equal(ptr.astype(np.int64), rptr) and np.array_equal(idx.astype(np.int64), ridx))
        print("lists %s by %s: %d records, %d calls, longest %d, entry for entry %s" % (what, "sample" if by_sample else "SNP", m.shape[0], ridx.size,
                                                                                        int(np.max(np.diff(rptr))), same))
        if not np.array_equal(ptr.astype(np.int64), rptr):
            bad = np.nonzero(np.diff(ptr.astype(np.int64)) != np.diff(rptr))[0]
            raise AssertionError((what, by_sample, "list lengths differ at records", bad[:8]))
        if not same:
            t = int(np.nonzero(idx.astype(np.int64) != ridx)[0][0])
            r = int(np.searchsorted(rptr, t, side="right") - 1)
            raise AssertionError((what, by_sample, "record", r, "entry", t - int(rptr[r]), "is", int(idx[t]), "expected", int(ridx[t])))
        n = ridx.size
    return n


@pytest.mark.parametrize("tiled", [None, "0"])
@pytest.mark.parametrize("shape", [M.TALL, M.WIDE], ids=["tall", "wide"])
def test_lists_equal_nonzero(built_lib, shape, tiled):
    import flashpca_amd as fp

    N, P = shape
    codes, info = M.missing_pattern(shape)
    miss = codes == 1
    saved = {k: os.environ.pop(k, None) for k in ("FPCA_I8_MODE", "FPCA_I8_TILED")}
    try:
        with fp.test_hooks():
            if tiled is not None:
                os.environ["FPCA_I8_TILED"] = tiled
            for S in ((7, 4) if tiled is None else (7,)):
                os.environ.pop("FPCA_I8_MODE", None)
                with fp.Context.from_packed(M.pack_codes(codes), N, P, accum="i8x%d" % S) as ctx:
                    assert np.array_equal(M.unpack_codes(ctx.download_packed(), N, P), codes)
                    assert np.array_equal(ctx.snp_missing(), miss.sum(axis=1))
                    view, dense = M.hybrid_view(miss, N, S)
                    what = "%dx%d S %d %s" % (N, P, S, "row-major" if tiled == "0" else "band-tiled")
                    for b in (16, 64):
                        assert ctx.missing_mode(b) == 4, what
                        listed = _check_lists(ctx, b, view, what + " hybrid view b %d" % b)
                    ptr, _ = ctx.missing_lists(16, False)
                    empty = np.nonzero((np.diff(ptr.astype(np.int64)) == 0) & (miss.sum(axis=1) > 0))[0]
                    print("lists %s: %d dense SNPs, %d listed calls of %d" % (what, empty.size, listed, int(miss.sum())))
                    assert np.array_equal(empty, dense) and dense.size > 0 and 0 < listed < miss.sum()
                    os.environ["FPCA_I8_MODE"] = "3"  # (gives up the hybrid view: the lists are made again from the plain copies)
                    assert ctx.missing_mode(32) == 3, what
                    _check_lists(ctx, 32, miss, what + " plain b 32")
                    os.environ["FPCA_I8_MODE"] = "0"
                    with pytest.raises(fp.FpcaError):  # not a list route
                        ctx.missing_lists(16, False)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- c / d. the operator, in child processes on the test build -------------------------------------------------------
_CHILD = r"""
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import flashpca_amd as fp
import test_missing_gathers_cpu as M
groups = json.loads(sys.argv[2])
out, info, dense = {}, {}, {}

def thrice(f, A, A2):
    R1 = f(A)
    R2 = f(A2)
    R3 = f(A)
    return R1, bool(np.isfinite(R1).all() and np.isfinite(R2).all() and np.max(np.abs(R2)) > 0), bool(np.array_equal(R1, R3) and not np.array_equal(R1, R2))

with fp.test_hooks():
    for g in groups:  # one context each
        N, P = g["shape"]
        S = g["S"]
        codes, _ = M.missing_pattern((N, P))
        for k in ("FPCA_I8_MODE", "FPCA_AR_CHUNKS", "FPCA_I8_TILED"):  # (read per call / per context)
            os.environ.pop(k, None)
        if g.get("ar_chunks"):
            os.environ["FPCA_AR_CHUNKS"] = str(g["ar_chunks"])
        with fp.Context.from_packed(M.pack_codes(codes), N, P, accum="i8x%d" % S) as ctx:
            if g.get("comm"):
                ctx.comm_init_rank(1, 0, fp.Context.comm_unique_id())
            if g.get("save"):
                out["meansd.%d.%d" % (N, P)] = ctx.stats()[0]
            if g.get("ref") and (N, P) not in dense:  # the oracle's dense standardised matrix, once per data set
                from oracle import oracle as O
                dense[N, P] = O.OracleData(packed=M.pack_codes(codes).ravel(), N=N, P=P, stand="binom2").dense()
            for route in g["routes"]:  # 4 first: any other route gives up the hybrid view for good
                if route == 4:
                    os.environ.pop("FPCA_I8_MODE", None)
                else:
                    os.environ["FPCA_I8_MODE"] = str(route)
                for b in g["bs"]:
                    key = "%s.S%d.b%d.r%d" % (g["name"], S, b, route)
                    i = {"mode": ctx.missing_mode(b), "chunks": ctx.allreduce_chunks() if g.get("comm") else 1}
                    if route in (3, 4):
                        i["listed"] = int(ctx.missing_lists(b, True)[1].size)
                    ops = M.operands(N, P, b)
                    for op in g["ops"]:
                        R, fin, rep = thrice({"xt": ctx.apply_xt, "x": ctx.apply_x, "xxt": ctx.apply_xxt}[op], *ops[op])
                        i[op] = {"hash": hashlib.sha1(np.ascontiguousarray(R).tobytes()).hexdigest(), "finite": fin, "repeat": rep}
                        if route in g.get("save", []):
                            out[key + "." + op] = R
                        if g.get("ref"):
                            if (N, P, b, op) not in dense:  # (the operands depend on the data set and the width alone)
                                X = dense[N, P]
                                dense[N, P, b, op] = X @ ops[op][0] if op == "x" else X @ (X.T @ ops[op][0])
                            ref = dense[N, P, b, op]
                            i[op]["err"] = float(np.max(np.abs(R - ref) / np.max(np.abs(ref), axis=0)))
                    info[key] = i
np.savez(sys.argv[3], **out)
print("CHILD " + json.dumps(info))
"""


def _run(groups, env_extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    env.update(env_extra)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "res.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(groups), out], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        info = json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
        return dict(np.load(out)), info


_NAME = {M.TALL: "tall", M.WIDE: "wide"}
_KERNELS = {(tuple(c["shape"]), c["S"], c["b"], c["route"], c["forced"]): c for c in M.route_cases()}


def _k2_groups(save):
    return [dict(name=_NAME[shape], shape=list(shape), S=S, routes=[4, 3, 1, 0], bs=[16, 32, 64], ops=["xt"], save=[4] if save and S == 7 else [])
            for shape in (M.TALL, M.WIDE) for S in (7, 4)]


def _check_info(groups, info, forced, what):
    """Route, finiteness and the A, A2, A repeat of every case; prints what the case is about (route, gather kernels, listed calls)."""
    for g in groups:
        for route in g["routes"]:
            for b in g["bs"]:
                key = "%s.S%d.b%d.r%d" % (g["name"], g["S"], b, route)
                i, c = info[key], _KERNELS[(tuple(g["shape"]), g["S"], b, route, forced)]
                assert i["mode"] == route, (key, i)
                if route in (3, 4):
                    assert i["listed"] == c["listed"], (key, i, c)
                for op in g["ops"]:
                    assert i[op]["finite"] and i[op]["repeat"], (key, op, i)
                print("%s %s %dx%d route %d: K2 gather kernel %d, K3 gather kernel %d, %d listed calls; %s" % (
                    what, key, g["shape"][0], g["shape"][1], route, c["k2"], c["k3"], c["listed"], " ".join("%s %s" % (op, i[op]["hash"][:12]) for op in g["ops"])))


@pytest.fixture(scope="module")
def k2_default(built_lib):
    """X'B of every case under the gather kernels the dispatch chooses (no FPCA_GATHER)."""
    groups = _k2_groups(True)
    res, info = _run(groups, {})
    return groups, res, info


@pytest.mark.parametrize("gather", ["", "1", "2", "3"])
def test_k2_routes_bit_identical(k2_default, gather):
    """Integer block: routes 4, 3, 1, 0, 16 / 32 / 64 columns, 7 and 4 slices -- one result per matrix and width, under every gather kernel."""
    groups, res, info = k2_default
    if gather:
        groups = _k2_groups(False)
        _, info_g = _run(groups, {"FPCA_GATHER": gather})
    else:
        info_g = info
    _check_info(groups, info_g, int(gather or 0), "K2 FPCA_GATHER=%s" % (gather or "unset"))
    for g in groups:
        for b in g["bs"]:
            want = hashlib.sha1(np.ascontiguousarray(res["%s.S7.b%d.r4.xt" % (g["name"], b)]).tobytes()).hexdigest()
            assert info["%s.S7.b%d.r4" % (g["name"], b)]["xt"]["hash"] == want
            for route in g["routes"]:
                key = "%s.S%d.b%d.r%d" % (g["name"], g["S"], b, route)
                assert info_g[key]["xt"]["hash"] == want, (key, gather, "differs from route 4 at 7 slices without FPCA_GATHER")


@pytest.mark.parametrize("shape", [M.TALL, M.WIDE], ids=["tall", "wide"])
def test_k2_integer_block_within_bound(k2_default, shape):
    """The one result of each matrix and width against (g - mean m) / sd in longdouble, g = (G.M)'B and m = M'B exact integers."""
    _, res, _ = k2_default
    N, P = shape
    codes, _ = M.missing_pattern(shape)
    GM = np.where(codes == 0, 2, np.where(codes == 2, 1, 0)).astype(np.float64)
    Mk = (codes != 1).astype(np.float64)
    meansd = res["meansd.%d.%d" % (N, P)]
    mean, sd = meansd[:, 0].astype(np.longdouble)[:, None], meansd[:, 1].astype(np.longdouble)[:, None]
    live = (meansd[:, 1] > 1e-9)[:, None]
    assert not live[M.J_ALL]  # the SNP that is missing everywhere
    for b in (16, 32, 64):
        Bi = M.operands(N, P, b)["xt"][0]
        assert np.array_equal(Bi.astype(np.int64), Bi)
        # (fp64 products of integers whose every partial sum stays below 2^53: exact in any order, so these ARE the int64 values)
        g, m = (GM @ Bi).astype(np.int64), (Mk @ Bi).astype(np.int64)
        assert np.max(np.abs(g)) <= 8 * N and np.max(np.abs(m)) <= 4 * N
        rows = np.arange(0, P, max(P // 40, 1))  # ... checked in int64 on a sample of the rows
        assert np.array_equal(g[rows], GM[rows].astype(np.int64) @ Bi.astype(np.int64)) and np.array_equal(m[rows], Mk[rows].astype(np.int64) @ Bi.astype(np.int64))
        gl, ml = g.astype(np.longdouble), m.astype(np.longdouble)
        sd1 = np.where(live, sd, 1)
        want = np.where(live, (gl - mean * ml) / sd1, 0)
        bound = np.where(live, 4 * np.longdouble(2.0) ** -53 * (np.abs(gl) + np.abs(mean * ml)) / sd1, 0)
        T = res["%s.S7.b%d.r4.xt" % (_NAME[shape], b)]
        err = np.abs(T.astype(np.longdouble) - want)
        print("K2 %dx%d b %d: max error / bound %.3f, monomorphic SNPs %d" % (N, P, b, float(np.max(err / np.where(bound > 0, bound, 1))), int((~live).sum())))
        assert np.all(err <= bound), (shape, b, float(np.max(err - bound)))
        assert np.all(T[~live[:, 0]] == 0.0)


_TOL = {7: 1e-12, 4: 3e-6}  # test_i8_mode_operator_parity, per S


def _k3_groups(ref):
    """ref: the child also measures every result against the oracle's dense matrix, max |R - ref| over the column maximum of |ref|."""
    gs = []
    for shape in (M.TALL, M.WIDE):
        for S, bs in ((7, [16, 64]), (4, [32])):
            gs.append(dict(name=_NAME[shape], shape=list(shape), S=S, routes=[4, 3], bs=bs, ops=["x", "xxt"], ref=ref))
    # K3 in three row chunks of the sample-major copy behind a one-rank communicator
    gs.append(dict(name="tallchunks", shape=list(M.TALL), S=7, routes=[4, 3], bs=[16], ops=["xxt"], comm=True, ar_chunks=3, ref=ref))
    return gs


@pytest.fixture(scope="module")
def k3_inline(built_lib):
    groups = _k3_groups(True)
    res, info = _run(groups, {})
    return groups, res, info


def test_k3_and_apply_against_dense(k3_inline):
    """X T and X X'B on the list routes against the oracle's dense matrix; the short kernel on the tall matrix, the batched one on the wide."""
    groups, _, info = k3_inline
    _check_info(groups, info, 0, "K3 inline")
    for g in groups:
        N, P = g["shape"]
        for route in g["routes"]:
            for b in g["bs"]:
                c = _KERNELS[((N, P), g["S"], b, route, 0)]
                assert c["k2"] == 1 and c["k3"] == ((3 if b <= 32 else 2) if (N, P) == M.TALL else 2)
                key = "%s.S%d.b%d.r%d" % (g["name"], g["S"], b, route)
                if g.get("comm"):
                    assert info[key]["chunks"] == 3, info[key]
                for op in g["ops"]:
                    e, tol = info[key][op]["err"], 10 * _TOL[g["S"]]
                    print("K3 %s %s: error %.3g tolerance %.3g" % (key, op, e, tol))
                    assert e <= tol, (key, op, e)


def test_side_stream_changes_no_bits(k3_inline):
    """FPCA_SPARSE_SIDE_BYTES=1: both stages gather on the low-priority side stream, two event hand-offs each -- the same bits."""
    groups, _, info = k3_inline
    _, info_s = _run(_k3_groups(False), {"FPCA_SPARSE_SIDE_BYTES": "1"})
    _check_info(groups, info_s, 0, "K3 side stream")
    for key, i in info.items():
        for op in ("x", "xxt"):
            if op in i:
                same = i[op]["hash"] == info_s[key][op]["hash"]
                print("side stream %s %s bit-identical to inline: %s" % (key, op, same))
                assert same, (key, op)
