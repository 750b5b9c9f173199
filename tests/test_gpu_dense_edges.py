"""The in-memory matrix path at its edges: k_dense_standardise (util.cpp:24-192) and the dense pair K2d / K3d behind fpca_create_dense,
at the shapes where a row loop, a workgroup or a column chunk ends, on columns a careless kernel mishandles.

Read-back without rounding.  On a dense context apply_x(eye(P)) is the standardised matrix Xs and apply_xt(eye(N)) is Xs': every output
entry is one product x * 1.0 plus zeros, so every split plan of both kernels must hand the stored matrix back bit for bit.  With P or N
above 64 the two calls also run the 64-column chunk loops of the host-pointer entries (tests/test_gpu_host_pointers.py).

Shapes (N x P): 1 x 1, 2 x 3, 63 x 5, then one short of, on and one past 256 x 128 and 512 x 256 -- N_pad is a multiple of 512, a K3d
workgroup takes 256 rows, a K2d workgroup 128 matrix columns, the standardise workgroup strides the rows by 256.  All five methods.

Exact data: entries from {0, 1, 2}, so every sum and sum of squares is an integer below 2^53, exact in any order, and mean, sd and every
standardised entry are the same correctly rounded operations on the device as in orc_standardise: array_equal (NaN equal to NaN) on
stats()[0] and on both read-backs.  The trace is a sum of squares in another order: 1e-11 relative, the bound of tests/test_gpu_dense.py.

Planted columns, as many as the shape has room for beside one ordinary column, in this order: all NaN (last column; not under "none",
where 0 * NaN poisons every product in the reference as well -- that column is tested alone on a 5 x 1 matrix); one value 2.0 in row N / 2,
NaN elsewhere (column 0); constant 1.0; constant 0.0; only NaN in the first row; only NaN in the last row (these two from N = 3).  About
2 % NaN in the ordinary columns.  What the rules of util.cpp make of them is asserted on the oracle's output first, then on the device's.

Records (printed by every case, pytest -s; profiles/dense_edges_test_figures.txt).  Measured on the MI355X:
    exact data, 9 shapes x 5 methods: mean / sd, apply_x(eye) and apply_xt(eye) equal to the oracle bit for bit in all 45 cases; trace
        within 1.22e-15 relative (bound 1e-11); 5 x 1 all-NaN "none": mean NaN, sd 1, trace NaN
    real-valued 257 x 129: mean / sd within 7.8e-16 (bound 1e-12), read-backs within 5.1e-16 and trace within 3.6e-16 (bound 1e-11)
    ldx = N + 3 at 63 x 5 and 513 x 257: stats, trace and both read-backs bit-equal to the contiguous context's
    513 x 257 "sd", widths 1 / 16 / 17 / 48 / 64: apply_xt within 1.6e-15, apply_xxt within 1.2e-15 of numpy on the oracle's Xs, apply_x
        within 1.1e-15 at one column and equal to numpy's product at the others (bound 1e-11)
    no case above 0.26 s (the first, which initialises the device); both files, 120 cases, in 2.7 s
Each of these, tried by hand, fails cases here: `i < N_pad` in the first pass of k_dense_standardise (from 1 x 1 on), `: 0.0` for
`: mean` in its second pass (the planted single-value column under sd / binom / binom2), a dropped `c0 * ldb` or `c0 * ldy` in cabi.cpp
(the read-backs from 255 x 127 on)."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (63, 5), (255, 127), (256, 128), (257, 129), (511, 255), (512, 256), (513, 257)]
METHODS = ["none", "sd", "binom", "binom2", "center"]
KINDS = ("all_nan", "single", "const1", "const0", "nan_first", "nan_last")
REL = 1e-11  # products and trace (tests/test_gpu_dense.py)


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as O

    O.build()
    return O


def planted_columns(N, P, stand):
    """kind -> column, as many kinds as leave one ordinary column."""
    where = dict(all_nan=P - 1, single=0, const1=P // 2, const0=1, nan_first=P - 2, nan_last=2)
    kinds = [k for k in KINDS if not (k == "all_nan" and stand == "none") and not (k.startswith("nan_") and N < 3)]
    cols = {k: where[k] for k in kinds[:max(0, min(len(kinds), P - 1))]}
    if len(set(cols.values())) != len(cols):  # (a shape too narrow for these places: plant them from the left)
        cols = {k: j for j, k in enumerate(cols)}
    return cols


def make_matrix(N, P, stand, exact):
    rng = np.random.default_rng(100003 * N + 101 * P + (7 if exact else 0))
    X = rng.integers(0, 3, size=(N, P)).astype(np.float64) if exact else rng.standard_normal((N, P)) * 2 + 0.5
    X[rng.random((N, P)) < 0.02] = np.nan
    for j in range(P):  # (an ordinary column keeps a value: under "none" an all-NaN column would poison the products)
        if np.all(np.isnan(X[:, j])):
            X[0, j] = 1.0
    cols = planted_columns(N, P, stand)
    for kind, j in cols.items():
        if kind == "all_nan":
            X[:, j] = np.nan
        elif kind == "single":
            X[:, j] = np.nan
            X[N // 2, j] = 2.0
        elif kind == "const1":
            X[:, j] = 1.0
        elif kind == "const0":
            X[:, j] = 0.0
        else:
            X[:, j] = rng.integers(0, 3, size=N).astype(np.float64) if exact else rng.standard_normal(N) * 2 + 0.5
            X[0 if kind == "nan_first" else N - 1, j] = np.nan
    return np.asfortranarray(X), cols


def check_planted(Xs, ms, cols, stand, N, who):
    """What util.cpp:24-192 makes of the planted columns (confirmed on the CPU at N = 9), on the oracle's output and on the device's."""
    for kind, j in cols.items():
        col, mean, sd, msg = Xs[:, j], ms[j, 0], ms[j, 1], "%s: %s column under %s" % (who, kind, stand)
        if kind == "all_nan":  # 0 / 0: no mean; nothing to standardise, NaN -> 0
            assert np.isnan(mean), msg
            if stand == "sd":
                assert np.isnan(sd), msg
            assert np.all(col == 0.0), msg
        elif kind == "single":  # nj - 1 == 0: the variance is 0 / 0, and `sd > 1e-9` is false for NaN as for 0 -> the mean
            assert mean == 2.0, msg
            if stand == "sd":
                assert np.isnan(sd), msg
            if stand in ("binom", "binom2"):
                assert sd == 0.0, msg
            want = np.zeros(N)
            want[N // 2] = 0.0 if stand == "center" else 2.0
            if stand == "none":
                want[:] = 2.0
            assert np.array_equal(col, want), msg
        elif kind == "const1":
            assert mean == 1.0, msg
            if stand == "binom":
                assert sd == 0.5, msg
            if stand == "sd":
                assert sd == 0.0, msg
            assert np.all(col == (1.0 if stand in ("none", "sd") else 0.0)), msg  # (sd: zero variance -> the mean)
        elif kind == "const0":
            assert mean == 0.0 and np.all(col == 0.0), msg
            if stand != "none" and stand != "center":
                assert sd == 0.0, msg
        else:
            row = 0 if kind == "nan_first" else N - 1
            assert not np.isnan(mean), msg
            assert col[row] == (mean if stand == "none" else 0.0), msg


_REF = {}


def reference(orc, N, P, stand, exact=True):
    """(X, planted columns, oracle's Xs, oracle's meansd), computed once, read-only, the oracle's own output checked."""
    key = (N, P, stand, exact)
    if key not in _REF:
        X, cols = make_matrix(N, P, stand, exact)
        Xs, ms = orc.standardise(X, stand)
        check_planted(Xs, ms, cols, stand, N, "oracle")
        for a in (X, Xs, ms):
            a.flags.writeable = False
        _REF[key] = (X, cols, Xs, ms)
    return _REF[key]


def same(a, b):
    return bool(np.array_equal(a, b, equal_nan=True))


def read_back(ctx):
    """(Xs through K3d, Xs through K2d): one product x * 1.0 per entry."""
    return ctx.apply_x(np.eye(ctx.P)), ctx.apply_xt(np.eye(ctx.N)).T


def rel_err(a, ref):
    return float(np.max(np.abs(a - ref)) / max(np.max(np.abs(ref)), np.finfo(float).tiny))


def bits(v):
    return "0x%016x" % np.float64(v).view(np.uint64)


def report_unequal(name, got, ref, stand):
    """The first entries that differ, with both bit patterns (a last-place difference is a finding about the device's arithmetic)."""
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    return "%s under %s: %d entries differ; " % (name, stand, len(bad)) + "; ".join(
        "%s device %s (%r) oracle %s (%r)" % (tuple(i), bits(got[tuple(i)]), float(got[tuple(i)]), bits(ref[tuple(i)]), float(ref[tuple(i)]))
        for i in bad[:4])


@pytest.mark.parametrize("stand", METHODS)
@pytest.mark.parametrize("N,P", SHAPES)
def test_exact_data_bit_for_bit(N, P, stand, fp, orc):
    X, cols, Xs, ms = reference(orc, N, P, stand)
    assert not np.any(np.isnan(Xs))
    t0 = time.perf_counter()
    with fp.Context.from_dense(X, stand=stand) as ctx:
        assert (ctx.N, ctx.P) == (N, P)
        gms, trace = ctx.stats()
        via_x, via_xt = read_back(ctx)
    dt = time.perf_counter() - t0
    tr_ref = float((Xs * Xs).sum())
    tr_err = abs(trace - tr_ref) / tr_ref if tr_ref > 0 else abs(trace)
    eq = same(gms, ms), same(via_x, Xs), same(via_xt, Xs)
    print("%d x %d %s (planted %s): mean/sd equal to the oracle bit for bit: %s, apply_x(eye): %s, apply_xt(eye): %s; trace relative error %.2e; "
          "%.3f s" % (N, P, stand, ",".join(cols) or "none", eq[0], eq[1], eq[2], tr_err, dt))
    check_planted(via_x, gms, cols, stand, N, "device")
    assert eq[0], report_unequal("mean/sd", gms, ms, stand)
    assert eq[1], report_unequal("apply_x(eye(P))", via_x, Xs, stand)
    assert eq[2], report_unequal("apply_xt(eye(N))'", via_xt, Xs, stand)
    assert tr_err <= REL


def test_all_nan_column_alone_under_none(fp, orc):
    """Under "none" an all-NaN column stays NaN: the mean and the trace are NaN, as in the reference."""
    X = np.full((5, 1), np.nan, order="F")
    Xs, ms = orc.standardise(X, "none")
    assert np.all(np.isnan(Xs)) and np.isnan(ms[0, 0]) and ms[0, 1] == 1.0
    with fp.Context.from_dense(X, stand="none") as ctx:
        gms, trace = ctx.stats()
    print("5 x 1 all NaN, none: mean %r sd %r trace %r" % (float(gms[0, 0]), float(gms[0, 1]), trace))
    assert same(gms, ms) and np.isnan(trace)


@pytest.mark.parametrize("stand", ["none", "sd", "center"])
def test_real_valued_data(stand, fp, orc):
    N, P = 257, 129
    X, cols, Xs, ms = reference(orc, N, P, stand, exact=False)
    assert len(cols) == (5 if stand == "none" else 6)
    with fp.Context.from_dense(X, stand=stand) as ctx:
        gms, trace = ctx.stats()
        via_x, via_xt = read_back(ctx)
    fin = ~np.isnan(ms)
    e_ms = float(np.max(np.abs(gms[fin] - ms[fin]) / np.maximum(np.abs(ms[fin]), 1.0)))
    tr_ref = float((Xs * Xs).sum())
    print("257 x 129 %s, rnorm * 2 + 0.5: mean/sd error %.2e; apply_x(eye) %.2e, apply_xt(eye) %.2e, trace %.2e relative" % (
        stand, e_ms, rel_err(via_x, Xs), rel_err(via_xt, Xs), abs(trace - tr_ref) / tr_ref))
    check_planted(via_x, gms, cols, stand, N, "device")
    assert np.allclose(gms, ms, rtol=1e-12, atol=1e-12, equal_nan=True)
    assert rel_err(via_x, Xs) <= REL and rel_err(via_xt, Xs) <= REL
    assert abs(trace - tr_ref) <= REL * tr_ref


@pytest.mark.parametrize("N,P", [(63, 5), (513, 257)])
def test_leading_dimension_of_the_input(N, P, fp, orc):
    """fpca_create_dense with ldx = N + 3: the first N rows of a taller Fortran array whose spare rows are NaN."""
    X = reference(orc, N, P, "sd")[0]
    big = np.full((N + 3, P), np.nan, order="F")
    big[:N] = X
    with fp.Context.from_dense(X, stand="sd") as ctx:
        ms0, tr0 = ctx.stats()
        x0, xt0 = read_back(ctx)
    h = C.c_void_p()
    rc = fp.lib().fpca_create_dense(C.byref(h), big.ctypes.data_as(C.c_void_p), N + 3, N, P, 1, 0)  # (1: "sd")
    assert rc == 0, fp.lib().fpca_last_error()
    with fp.Context(h) as ctx:
        assert (ctx.N, ctx.P) == (N, P)
        ms1, tr1 = ctx.stats()
        x1, xt1 = read_back(ctx)
    eq = same(ms1, ms0), tr1 == tr0, same(x1, x0), same(xt1, xt0)
    print("%d x %d sd, ldx = N + 3: stats equal to the contiguous context's bit for bit: %s, trace: %s, apply_x(eye): %s, apply_xt(eye): %s" % (
        (N, P) + eq))
    assert all(eq)


@pytest.fixture(scope="module")
def sd_context(fp, orc):
    X, _, Xs, _ = reference(orc, 513, 257, "sd")
    with fp.Context.from_dense(X, stand="sd") as ctx:
        yield ctx, Xs


@pytest.mark.parametrize("b", [1, 16, 17, 48, 64])
def test_every_width_on_the_standardised_matrix(b, sd_context):
    """tests/test_gpu_fp_splits.py covers the split plans under "none" only; here they multiply a matrix that went through "sd"."""
    ctx, Xs = sd_context
    rng = np.random.default_rng(b)
    B, Tin = rng.standard_normal((ctx.N, b)), rng.standard_normal((ctx.P, b))
    e = rel_err(ctx.apply_xt(B), Xs.T @ B), rel_err(ctx.apply_x(Tin), Xs @ Tin), rel_err(ctx.apply_xxt(B), Xs @ (Xs.T @ B))
    print("513 x 257 sd, %d columns: apply_xt %.2e, apply_x %.2e, apply_xxt %.2e of numpy on the oracle's matrix" % ((b,) + e))
    assert max(e) <= REL
