"""The host-pointer entries fpca_apply_xxt / fpca_apply_xt / fpca_apply_x (csrc/cabi.cpp), which every Python and R caller goes through,
where no other test takes them: past 64 columns, with leading dimensions above the row count, and through the pipelined download.

Contexts, 513 x 300 each: packed fp64, packed "auto" (the int8 path) on the same generated codes (about 2 % missing), dense "sd".

More than 64 columns (b = 1, 64, 65, 130): the entries cut the columns into chunks of 64, so the wide call must equal, array_equal, the
separate calls on [0, 64), [64, 128), [128, b) -- it is specified to be exactly those launches -- and lie within 1e-11 of numpy on the
oracle's matrix, relative to the largest entry per column (the bound of tests/test_gpu_kernels.py for these calls).

Leading dimensions (b = 3, 130): ldb = N + 5, ldy = N + 2, ldt = P + 7 through lib() directly.  Inputs are the leading rows of taller
Fortran arrays whose spare rows hold NaN, outputs taller arrays prefilled with -7.25: the leading rows equal the contiguous call's result
bit for bit and every spare row is still -7.25.

Refusals: a leading dimension one short of the row count, b = 0 and a NULL pointer return -1 with "bad argument", and the context serves
a correct call afterwards.

Pipelined download: staged_download (csrc/download.hip) cuts results above 1,048,576 doubles into pieces that cycle through four pinned
slots and are scattered by helper threads.  N = 8, P = 70,000 packed (8.96 MB of device records) and 64 columns give T = 4,480,000 doubles:
five pieces, the fifth reusing slot 0.  With ldt = P + 7 the piece boundaries fall at (row, column) = (68576, 14), (67152, 29),
(65728, 44), (64304, 59), all inside a column.  B = e_0 .. e_7 in columns 0..7: those columns are single products, equal bit for bit to
the single-column calls (70,000 doubles, the one-piece path), columns 8..63 exactly zero, the seven spare rows of every column still
-7.25, and columns 0..7 within 1e-11 of the oracle's rows.  A second call with e_{c mod 8} in EVERY column puts values on both sides of
every piece boundary and of every helper thread's share.

Records (printed by every case, pytest -s; profiles/dense_edges_test_figures.txt).  Measured on the MI355X:
    wide calls: equal to the chunked calls bit for bit in all 36 cases; worst error against numpy 1.9e-15 (fp64), 2.0e-15 (int8),
        2.6e-15 (dense), bound 1e-11; no call above 0.01 s
    leading dimensions: leading rows bit-equal and spare rows untouched in all 18 cases; all 45 refusals -1 "bad argument"
    pipelined download: columns bit-equal to the single-column calls in both calls, zero columns zero, spare rows untouched,
        1.2e-16 from the oracle; 0.72 s
Tried by hand: with N for ld in staged_download's scatter, test_leading_dimensions and test_pipelined_download fail (19 cases of the two
files); a dropped `c0 * ldb` / `c0 * ldy` in cabi.cpp fails the wide calls and, first, the read-backs of tests/test_gpu_dense_edges.py."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P = 513, 300
SENTINEL = -7.25
REL = 1e-11
KINDS = ["fp64", "auto", "dense"]
OPS = ["apply_xxt", "apply_xt", "apply_x"]


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as O

    O.build()
    return O


def pack_codes(codes):
    """codes: P x N raw .bed codes (0 hom A1, 1 missing, 2 het, 3 hom A2) -> P x ceil(N / 4) bytes, SNP-major, pad bits 0."""
    Pn, Nn = codes.shape
    full = np.zeros((Pn, (Nn + 3) // 4 * 4), dtype=np.uint8)
    full[:, :Nn] = codes
    return np.ascontiguousarray(full[:, 0::4] | (full[:, 1::4] << 2) | (full[:, 2::4] << 4) | (full[:, 3::4] << 6))


def random_codes(rng, Pn, Nn, missing):
    codes = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=(Pn, Nn), p=[0.2, 0.4, 0.4])
    codes[rng.random((Pn, Nn)) < missing] = 1
    return codes


@pytest.fixture(scope="module")
def contexts(fp, orc):
    """kind -> (context, the oracle's N x P matrix, read-only)."""
    rng = np.random.default_rng(513300)
    packed = pack_codes(random_codes(rng, P, N, 0.02))
    Xp = orc.OracleData(packed=packed, N=N, P=P, stand="binom2").dense()
    Xd = rng.standard_normal((N, P)) * 2 + 0.5
    Xd[rng.random((N, P)) < 0.02] = np.nan
    Xds, _ = orc.standardise(Xd, "sd")
    for a in (Xp, Xds):
        a.flags.writeable = False
    out = {"fp64": (fp.Context.from_packed(packed, N, P, accum="fp64"), Xp), "auto": (fp.Context.from_packed(packed, N, P, accum="auto"), Xp),
           "dense": (fp.Context.from_dense(Xd, stand="sd"), Xds)}
    assert out["fp64"][0].accum == "fp64" and out["auto"][0].accum.startswith("i8"), out["auto"][0].accum
    yield out
    for ctx, _ in out.values():
        ctx.close()


def rows_in(ctx, op):
    return ctx.P if op == "apply_x" else ctx.N


def rows_out(ctx, op):
    return ctx.P if op == "apply_xt" else ctx.N


def numpy_ref(X, op, A):
    return X @ (X.T @ A) if op == "apply_xxt" else (X.T @ A if op == "apply_xt" else X @ A)


def col_err(got, ref):
    """Largest error relative to the largest entry of its column."""
    scale = np.maximum(np.max(np.abs(ref), axis=0), np.finfo(float).tiny)
    return float(np.max(np.max(np.abs(got - ref), axis=0) / scale))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def raw_call(fp, ctx, op, src, ld_in, b, dst, ld_out):
    return getattr(fp.lib(), "fpca_" + op)(ctx.h, ptr(src) if src is not None else None, ld_in, b, ptr(dst) if dst is not None else None, ld_out)


@pytest.mark.parametrize("b", [1, 64, 65, 130])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kind", KINDS)
def test_more_than_64_columns(kind, op, b, contexts):
    ctx, X = contexts[kind]
    A = np.random.default_rng(1000 + b).standard_normal((rows_in(ctx, op), b))
    call = getattr(ctx, op)
    t0 = time.perf_counter()
    wide = call(A)
    dt = time.perf_counter() - t0
    assert wide.shape == (rows_out(ctx, op), b)
    parts = np.concatenate([call(np.asfortranarray(A[:, c0:min(c0 + 64, b)])) for c0 in range(0, b, 64)], axis=1)
    equal, err = bool(np.array_equal(wide, parts)), col_err(wide, numpy_ref(X, op, A))
    print("%s %s, %d columns: equal to the calls on chunks of 64 bit for bit: %s; %.2e from numpy on the oracle's matrix; %.3f s" % (
        kind, op, b, equal, err, dt))
    assert equal
    assert err <= REL


def tall(rows, spare, b, fill, top=None):
    a = np.full((rows + spare, b), fill, order="F")
    if top is not None:
        a[:rows] = top
    return a


@pytest.mark.parametrize("b", [3, 130])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kind", KINDS)
def test_leading_dimensions(kind, op, b, fp, contexts):
    ctx, _ = contexts[kind]
    spare_in = 7 if op == "apply_x" else 5    # ldt = P + 7, ldb = N + 5
    spare_out = 7 if op == "apply_xt" else 2  # ldt = P + 7, ldy = N + 2
    ri, ro = rows_in(ctx, op), rows_out(ctx, op)
    A = np.random.default_rng(2000 + b).standard_normal((ri, b))
    want = getattr(ctx, op)(A)
    src, dst = tall(ri, spare_in, b, np.nan, A), tall(ro, spare_out, b, SENTINEL)
    rc = raw_call(fp, ctx, op, src, ri + spare_in, b, dst, ro + spare_out)
    assert rc == 0, fp.lib().fpca_last_error()
    equal, kept = bool(np.array_equal(dst[:ro], want)), bool(np.all(dst[ro:] == SENTINEL))
    print("%s %s, %d columns, leading dimensions %d in / %d out: leading rows equal to the contiguous call bit for bit: %s; spare rows "
          "untouched: %s" % (kind, op, b, ri + spare_in, ro + spare_out, equal, kept))
    assert not np.any(np.isnan(want))
    assert equal and kept


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind, op, fp, contexts):
    ctx, _ = contexts[kind]
    ri, ro, b = rows_in(ctx, op), rows_out(ctx, op), 3
    A = np.random.default_rng(3000).standard_normal((ri, b))
    want = getattr(ctx, op)(A)
    src, dst = np.asfortranarray(A), tall(ro, 0, b, SENTINEL)
    bad = {"input leading dimension one short": (src, ri - 1, b, dst, ro), "output leading dimension one short": (src, ri, b, dst, ro - 1),
           "b = 0": (src, ri, 0, dst, ro), "NULL input": (None, ri, b, dst, ro), "NULL output": (src, ri, b, None, ro)}
    for what, (s, ldi, nb, d, ldo) in bad.items():
        rc = raw_call(fp, ctx, op, s, ldi, nb, d, ldo)
        msg = fp.lib().fpca_last_error().decode()
        print("%s %s, %s: %d, %s" % (kind, op, what, rc, msg))
        assert rc == -1 and "bad argument" in msg, what
        assert np.all(dst == SENTINEL), what
    rc = getattr(fp.lib(), "fpca_" + op)(None, ptr(src), ri, b, ptr(dst), ro)
    assert rc == -1 and "bad argument" in fp.lib().fpca_last_error().decode()
    assert raw_call(fp, ctx, op, src, ri, b, dst, ro) == 0
    assert np.array_equal(dst, want)  # the context still serves


def test_pipelined_download(fp, orc):
    """Five pieces through four slots, boundaries inside columns 14, 29, 44 and 59 at rows 68576, 67152, 65728 and 64304 (module docstring)."""
    n, p, b, spare = 8, 70000, 64, 7
    piece = 1 << 20
    assert -(-p * b // piece) == 5 and [divmod(k * piece, p) for k in range(1, 5)] == [(14, 68576), (29, 67152), (44, 65728), (59, 64304)]
    rng = np.random.default_rng(870000)
    packed = pack_codes(random_codes(rng, p, n, 0.001))
    X = orc.OracleData(packed=packed, N=n, P=p, stand="binom2").dense()
    t0 = time.perf_counter()
    with fp.Context.from_packed(packed, n, p, accum="fp64") as ctx:
        singles = [ctx.apply_xt(np.eye(n)[:, c])[:, 0] for c in range(n)]  # 70,000 doubles each: the one-piece path
        for name, hot in (("e_c in columns 0..7", [c if c < n else None for c in range(b)]), ("e_(c mod 8) in every column", [c % n for c in range(b)])):
            B = np.zeros((n, b), order="F")
            for c, s in enumerate(hot):
                if s is not None:
                    B[s, c] = 1.0
            T = tall(p, spare, b, SENTINEL)
            rc = raw_call(fp, ctx, "apply_xt", B, n, b, T, p + spare)
            assert rc == 0, fp.lib().fpca_last_error()
            equal = all(np.array_equal(T[:p, c], singles[s]) for c, s in enumerate(hot) if s is not None)
            zero = all(np.all(T[:p, c] == 0.0) for c, s in enumerate(hot) if s is None)
            kept = bool(np.all(T[p:] == SENTINEL))
            err = max(float(np.max(np.abs(T[:p, c] - X[s])) / np.max(np.abs(X[s]))) for c, s in enumerate(hot) if s is not None)
            print("8 x 70000, 64 columns, ldt = P + 7, %s: columns equal to the single-column calls bit for bit: %s; other columns zero: %s; "
                  "spare rows untouched: %s; %.2e from the oracle's rows" % (name, equal, zero, kept, err))
            assert equal and zero and kept
            assert err <= REL
    print("pipelined download test: %.3f s after the oracle" % (time.perf_counter() - t0))
