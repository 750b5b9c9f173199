"""fpca_scca_prepare / fpca_scca_fit on the GPU against the reference's loop restated in numpy AS WRITTEN -- two products per
iteration, u = invdiv X'(Yh v), v = invdiv Yh'(X u), never via C = X'Y (RandomPCA::scca, randompca.cpp:387-528) -- on the CPU oracle's
dense standardised X and standardised Y, from the same V0.

Bounds.  The restatement run on C instead of the two products (CPU, numpy, the 30 parity cases below) differs from itself by
r = 1.5e-15 in U, 3.4e-15 in V, 8.8e-16 relative in d, with the same iteration counts and supports everywhere; the device sums its
P-term reductions in another order (about sqrt(P) eps = 3e-14 relative on a norm), so for EQUAL iteration counts the bound is 1e-12 on
max |dU| and max |dV| and 1e-11 relative on d.  The stopping rule lets two correct implementations stop one iteration apart (they then
differ by less than tol per entry): unequal counts must differ by exactly one, the bound becomes tol + 1e-12 (d: 2 sqrt(P) tol
relative), and at most ONE parametrised parity case may take that branch.
Measured on the MI355X (hapmap3_data, the 30 parity cases): max |dU| 1.6e-15, max |dV| 4.7e-15, d 1.3e-15 relative; every case stopped
on the restatement's own iteration.  Every case prints what it measured (pytest -s)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
STANDS = ("sd", "binom2", "binom", "center", "none")
LAMBDAS = ((1e-6, 1e-6), (5e-3, 1e-3), (2e-2, 1e-2))
B_EQ, B_D = 1e-12, 1e-11


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def norm_thresh(x, lam):
    """randompca.cpp:225-245."""
    s = np.linalg.norm(x)
    if s > 0:
        x = x / s
        x = np.sign(x) * np.maximum(np.abs(x) - lam, 0.0)
        s = np.linalg.norm(x)
        if s > 0:
            x = x / s
    return x


def reference_scca(X, Ys, divisor, l1, l2, V0, maxiter=1000, tol=1e-4, use_c=False):
    """randompca.cpp:402-528 on the standardised X (missing = 0) and the standardised Ys, with this project's edge rules where the
    reference has none: u or v below tol -> stop, this and the later columns U = 0, V = V0, d = 0; maxiter reached ->
    current u, v kept, d = 0; Px, Py from what is there.  use_c: the same loop on C = invdiv X'Yh (for the CPU cross-check)."""
    n, p = X.shape
    invdiv = 1.0 / np.sqrt(n - 1.0) if divisor == "n1" else 1.0
    Yh = Ys * invdiv
    ndim = V0.shape[1]
    U, V, d = np.zeros((p, ndim)), np.array(V0, dtype=np.float64), np.zeros(ndim)
    iters = np.zeros(ndim, dtype=int)
    Cm = (X.T @ Yh) * invdiv if use_c else None
    status = "ok"
    for j in range(ndim):
        it = 0
        while it < maxiter:
            u_old, v_old = U[:, j].copy(), V[:, j].copy()
            u = Cm @ V[:, j] if use_c else (X.T @ (Yh @ V[:, j])) * invdiv
            for q in range(j):
                u = u - (u @ U[:, q]) * U[:, q] / (U[:, q] @ U[:, q])
            u = norm_thresh(u, l1)
            if np.abs(u).max() < tol:
                status = "lambda1 too large"
                break
            U[:, j] = u
            v = Cm.T @ u if use_c else (Yh.T @ (X @ u)) * invdiv
            for q in range(j):
                v = v - (v @ V[:, q]) * V[:, q] / (V[:, q] @ V[:, q])
            v = norm_thresh(v, l2)
            if np.abs(v).max() < tol:
                status = "lambda2 too large"
                break
            V[:, j] = v
            if it > 0 and np.abs(v_old - v).max() < tol and np.abs(u_old - u).max() < tol:
                break
            it += 1
        iters[j] = it
        if status != "ok":
            U[:, j:] = 0
            V[:, j:] = V0[:, j:]
            break
        if it >= maxiter:
            status = "maxiter reached"
            break
        d[j] = ((X @ U[:, j]) * invdiv) @ (Yh @ V[:, j])
    return dict(U=U, V=V, d=d, Px=(X @ U) * invdiv, Py=Yh @ V, iters=iters, converged=status == "ok", status=status,
                nzero_x=(U != 0).sum(axis=0), nzero_y=(V != 0).sum(axis=0), invdiv=invdiv, Yh=Yh)


ONE_APART = []  # the parity cases whose iteration counts differed by one


def compare(got, ref, tol, label):
    """got: Context.scca_fit's result; ref: reference_scca's.  Prints what it measured, then asserts the module's bounds."""
    p = ref["U"].shape[0]
    assert got["status"] == ref["status"] and got["converged"] == ref["converged"], (label, got["status"], ref["status"])
    gi, ri = np.asarray(got["iters"], dtype=int), ref["iters"]
    dU, dV = np.abs(got["U"] - ref["U"]).max(), np.abs(got["V"] - ref["V"]).max()
    dmax = max(np.abs(ref["d"]).max(), 1e-300)
    dd = np.abs(got["d"] - ref["d"]).max() / dmax
    print("%s: iters %s / %s  max|dU| %.3g  max|dV| %.3g  d rel %.3g  nzero_x %s  d %s" % (label, gi.tolist(), ri.tolist(), dU, dV, dd,
                                                                                    got["nzero_x"].tolist(), ref["d"].tolist()))
    assert not np.isnan(got["U"]).any() and not np.isnan(got["V"]).any() and not np.isnan(got["d"]).any(), label
    if np.array_equal(gi, ri):
        bU, bD = B_EQ, B_D
    else:
        assert np.abs(gi - ri).max() == 1, (label, gi, ri)
        ONE_APART.append(label)
        bU, bD = tol + B_EQ, 2 * np.sqrt(p) * tol
    assert dU < bU and dV < bU and dd < bD, (label, dU, dV, dd, bU, bD)
    big = (np.abs(got["U"]) > bU) | (np.abs(ref["U"]) > bU)
    assert np.array_equal((got["U"] != 0) & big, (ref["U"] != 0) & big), label
    if np.array_equal(gi, ri):
        assert np.array_equal(got["nzero_y"], ref["nzero_y"]), (label, got["nzero_y"], ref["nzero_y"])
    check_projections(got, ref["X"], ref["Yh"], ref["invdiv"], label)


def check_projections(got, X, Yh, invdiv, label=""):
    """Px, Py against invdiv X U and Yh V formed from the RETURNED U and V: 1e-10 of the largest entry."""
    Px, Py = (X @ got["U"]) * invdiv, Yh @ got["V"]
    assert np.abs(got["Px"] - Px).max() <= 1e-10 * max(np.abs(Px).max(), 1e-300), (label, np.abs(got["Px"] - Px).max(), np.abs(Px).max())
    assert np.abs(got["Py"] - Py).max() <= 1e-10 * max(np.abs(Py).max(), 1e-300), label


def run_ref(X, Ys, divisor, l1, l2, V0, **kw):
    r = reference_scca(X, Ys, divisor, l1, l2, V0, **kw)
    r["X"] = X
    return r


def hm3_phenotypes(X, stand, k=20, seed=1):
    """k phenotypes X B + 3 noise, B non-zero on 200 random SNPs, standardised; shaped for `stand` (0/1/2 classes for the binomial
    standardisations, an offset for "none"); 2 % NaN except for the plain "sd" case."""
    n, p = X.shape
    rng = np.random.default_rng(seed)
    B = np.zeros((p, k))
    B[rng.choice(p, 200, replace=False)] = rng.standard_normal((200, k))
    Y = X @ B + 3 * rng.standard_normal((n, k))
    Y = (Y - Y.mean(axis=0)) / Y.std(axis=0, ddof=1)
    if stand in ("binom", "binom2"):
        Y = (Y > -0.6).astype(float) + (Y > 0.6)
    elif stand == "none":
        Y = Y * rng.uniform(0.5, 2, k) + rng.uniform(-1, 1, k)
    elif stand == "center":
        Y = Y * rng.uniform(0.5, 2, k) + 3
    if stand != "sd":
        Y[rng.random((n, k)) < 0.02] = np.nan
    return Y, rng.standard_normal((k, 3))


@pytest.fixture(scope="module")
def hm3(fp, O):
    n = fp.count_fam_rows(HM3 + ".fam")
    X = O.OracleData(HM3 + ".bed", n, "binom2").dense()
    ctx = fp.Context.from_bed(HM3 + ".bed", n, accum="auto")
    yield ctx, X
    ctx.close()


@pytest.mark.parametrize("divisor", ["n1", "none"])
@pytest.mark.parametrize("stand", STANDS)
def test_parity_with_the_reference_loop(fp, O, hm3, stand, divisor):
    """hapmap3_data (957 x 14,389), k = 20, ndim = 3, tol 1e-9, Gaussian V0: dense, half-sparse and sparse penalties."""
    ctx, X = hm3
    Y, V0 = hm3_phenotypes(X, stand)
    Ys, _ = O.standardise(Y, stand)
    ctx.scca_prepare(Y, standy=stand, divisor=divisor)
    for l1, l2 in LAMBDAS:
        ref = run_ref(X, Ys, divisor, l1, l2, V0, tol=1e-9)
        assert ref["converged"], (stand, divisor, l1, l2, ref["iters"])
        got = ctx.scca_fit(l1, l2, 3, V0, tol=1e-9)
        compare(got, ref, 1e-9, "parity %s %s %g %g" % (stand, divisor, l1, l2))
        assert len(ONE_APART) <= 1, ONE_APART  # over ALL parity cases: the one-apart branch cannot hide a real difference
        assert np.array_equal(got["nzero_x"], (got["U"] != 0).sum(axis=0)) and np.array_equal(got["nzero_y"], (got["V"] != 0).sum(axis=0))


@pytest.mark.parametrize("k,ndim", [(1, 1), (3, 3), (63, 2), (64, 2), (65, 2), (150, 2)])
def test_chunked_prepare(fp, O, hm3, k, ndim):
    """k columns go through K2 in chunks of at most 64: one pass (1, 3, 63, 64), two (65), three (150); k = 1 makes v = +-1; ndim = k."""
    ctx, X = hm3
    rng = np.random.default_rng(100 + k)
    B = np.zeros((X.shape[1], k))
    B[rng.choice(X.shape[1], 200, replace=False)] = rng.standard_normal((200, k))
    Y = X @ B + 3 * rng.standard_normal((X.shape[0], k))
    V0 = rng.standard_normal((k, ndim))
    Ys, _ = O.standardise(Y, "sd")
    ctx.scca_prepare(Y, standy="sd")
    ref = run_ref(X, Ys, "n1", 5e-3, 1e-3, V0, tol=1e-9)
    assert ref["converged"]
    got = ctx.scca_fit(5e-3, 1e-3, ndim, V0, tol=1e-9)
    compare(got, ref, 1e-9, "k=%d" % k)
    if k == 1:
        assert np.all(np.abs(got["V"]) == 1.0)


def test_grid_shares_one_prepare(fp, O, hm3):
    """One prepare, 3 x 3 fits == nine prepare + fit pairs, bit for bit (a fit does not disturb C); scca() returns R's nested list."""
    ctx, X = hm3
    Y, V0 = hm3_phenotypes(X, "sd", k=8, seed=5)
    V0 = V0[:, :2]
    l1s, l2s = (1e-6, 5e-3, 2e-2), (1e-6, 1e-3, 1e-2)
    ctx.scca_prepare(Y, standy="sd")
    grid = [[ctx.scca_fit(a, b, 2, V0, tol=1e-6) for b in l2s] for a in l1s]
    for i, a in enumerate(l1s):
        for j, b in enumerate(l2s):
            ctx.scca_prepare(Y, standy="sd")
            one = ctx.scca_fit(a, b, 2, V0, tol=1e-6)
            for f in ("U", "V", "d", "Px", "Py", "iters", "nzero_x", "nzero_y"):
                assert np.array_equal(one[f], grid[i][j][f]), (a, b, f)
    res = fp.scca(HM3, Y, lambda1=l1s, lambda2=l2s, standx="binom2", standy="sd", ndim=2, tol=1e-6, V=V0)
    assert len(res) == 3 and all(len(r) == 3 for r in res)
    for i in range(3):
        for j in range(3):
            for f in ("U", "V", "d", "Px", "Py"):
                assert np.array_equal(res[i][j][f], grid[i][j][f]), (i, j, f)
    assert res[0][0]["snp_ids"] == [l.split()[1] for l in open(HM3 + ".bim").read().splitlines()]
    s = fp.scca(HM3, Y, lambda1=5e-3, lambda2=1e-3, standx="binom2", standy="sd", ndim=2, tol=1e-6, V=V0)
    assert isinstance(s, dict) and np.array_equal(s["U"], grid[1][1]["U"])
    s = fp.scca(HM3, Y, lambda1=5e-3, lambda2=1e-3, standx="binom2", standy="sd", ndim=2, tol=1e-6, V=V0, simplify=False)
    assert isinstance(s, list) and len(s) == 1 and len(s[0]) == 1
    # no V: R's warm start (one fit at 1e-9 from a Gaussian matrix of `seed`), reproducible, and a property of the result
    w1 = fp.scca(HM3, Y, lambda1=5e-3, lambda2=1e-3, standx="binom2", standy="sd", ndim=2, tol=1e-6, seed=3)
    w2 = fp.scca(HM3, Y, lambda1=5e-3, lambda2=1e-3, standx="binom2", standy="sd", ndim=2, tol=1e-6, seed=3)
    assert w1["converged"] and np.array_equal(w1["U"], w2["U"])
    assert np.allclose(np.linalg.norm(w1["U"], axis=0), 1, atol=1e-12) and np.allclose(np.linalg.norm(w1["V"], axis=0), 1, atol=1e-12)
    assert np.allclose(np.abs(w1["d"]), np.abs(grid[1][1]["d"]), rtol=1e-3)  # (same optimum from another start)


def test_missing_call_routes_and_arithmetics(fp, O):
    """The realistic profile (rare variants, concentrated missing calls, the hybrid missing-call route) at 3,000 x 2,000, X from
    download_packed() through the oracle; exact int8 (auto) and fp64 at the module's bounds.  fp32: C carries the fp32 products'
    error (about 1e-7 relative), so the stopping iteration is not pinned and the run is held against the fp64 one at the bounds scaled
    by 1e6, as the UCCA tests scale theirs."""
    N, P, k = 3000, 2000, 8
    rng = np.random.default_rng(3)
    out = {}
    for accum in ("auto", "fp64", "fp32"):
        with fp.Context.synthetic(N, P, n_pop=3, realistic=True, accum=accum) as ctx:
            if accum == "auto":
                assert ctx.missing_mode(16) == 4
                X = O.OracleData(packed=ctx.download_packed(), N=N, P=P, stand="binom2").dense()
                B = np.zeros((P, k))
                B[rng.choice(P, 50, replace=False)] = rng.standard_normal((50, k))
                Y = X @ B + 3 * rng.standard_normal((N, k))
                Y[rng.random((N, k)) < 0.01] = np.nan
                V0 = rng.standard_normal((k, 2))
                Ys, _ = O.standardise(Y, "sd")
                ref = run_ref(X, Ys, "n1", 1e-2, 1e-3, V0, tol=1e-9)
                assert ref["converged"]
            ctx.scca_prepare(Y, standy="sd")
            out[accum] = ctx.scca_fit(1e-2, 1e-3, 2, V0, tol=1e-9)
    compare(out["auto"], ref, 1e-9, "realistic auto")
    compare(out["fp64"], ref, 1e-9, "realistic fp64")
    a, b = out["fp32"], out["fp64"]
    assert a["converged"] and np.abs(np.asarray(a["iters"], int) - np.asarray(b["iters"], int)).max() <= 1
    print("fp32 vs fp64: max|dU| %.3g max|dV| %.3g" % (np.abs(a["U"] - b["U"]).max(), np.abs(a["V"] - b["V"]).max()))
    assert np.abs(a["U"] - b["U"]).max() < 1e-6 and np.abs(a["V"] - b["V"]).max() < 1e-6
    assert np.abs(a["d"] - b["d"]).max() < 1e-5 * np.abs(b["d"]).max()


def test_edge_rules(fp, O, hm3):
    ctx, X = hm3
    Y, V0 = hm3_phenotypes(X, "sd", k=6, seed=9)
    Ys, _ = O.standardise(Y, "sd")
    n, p = X.shape
    ctx.scca_prepare(Y, standy="sd")
    # lambda1 so large that u vanishes: in dimension 0 ...
    got = ctx.scca_fit(0.9, 1e-3, 3, V0)
    assert got["status"] == "lambda1 too large" and not got["converged"]
    assert np.all(got["U"] == 0) and np.array_equal(got["V"], V0) and np.all(got["d"] == 0)
    assert not np.isnan(got["Px"]).any() and not np.isnan(got["Py"]).any() and np.all(got["Px"] == 0)
    compare(got, run_ref(X, Ys, "n1", 0.9, 1e-3, V0), 1e-4, "u vanishes")
    # ... lambda2, the same
    got = ctx.scca_fit(1e-3, 1.0, 3, V0)
    assert got["status"] == "lambda2 too large" and not got["converged"] and np.array_equal(got["V"], V0) and np.all(got["U"] == 0)
    # maxiter = 2: the current u, v stay, d = 0, Px consistent with U
    got = ctx.scca_fit(5e-3, 1e-3, 3, V0, maxiter=2, tol=1e-9)
    ref = run_ref(X, Ys, "n1", 5e-3, 1e-3, V0, maxiter=2, tol=1e-9)
    assert got["status"] == "maxiter reached" and not got["converged"] and got["iters"].tolist() == [2, 0, 0]
    assert np.all(got["U"][:, 1:] == 0) and np.array_equal(got["V"][:, 1:], V0[:, 1:]) and abs(np.linalg.norm(got["U"][:, 0]) - 1) < 1e-12
    compare(got, ref, 1e-9, "maxiter")
    # refusals, each with its message
    for kw, msg in ((dict(ndim=7), "You asked for 7 dimensions, but only 6 allowed"), (dict(ndim=0), "ndim can't be less than 1"),
                    (dict(lambda1=-1.0), "lambda1 must be non-negative"), (dict(lambda2=-1e-3), "lambda2 must be non-negative"),
                    (dict(tol=0.0), "tol must be positive"), (dict(maxiter=0), "maxiter must be at least 1")):
        a = dict(lambda1=1e-3, lambda2=1e-3, ndim=3, maxiter=10, tol=1e-4)
        a.update(kw)
        nd = max(a["ndim"], 1)
        with pytest.raises(fp.FpcaError, match=msg) as e:
            ctx.scca_fit(a["lambda1"], a["lambda2"], a["ndim"], np.ones((6, nd)), maxiter=a["maxiter"], tol=a["tol"])
        assert e.value.code == -1
    with pytest.raises(ValueError, match="dimensions of V"):
        ctx.scca_fit(1e-3, 1e-3, 3, np.ones((5, 3)))
    with pytest.raises(fp.FpcaError, match="NULL pointer"):
        fp._lib.check(fp.lib().fpca_scca_prepare(ctx.h, None, n, 3, 1, 1))
    # a second prepare replaces the first (k changes with it)
    Y2 = Y[:, :4] * 2 + 1
    ctx.scca_prepare(Y2, standy="center", divisor="none")
    Ys2, _ = O.standardise(Y2, "center")
    compare(ctx.scca_fit(5e-3, 1e-3, 2, V0[:4, :2], tol=1e-9), run_ref(X, Ys2, "none", 5e-3, 1e-3, V0[:4, :2], tol=1e-9), 1e-9, "second prepare")
    with pytest.raises(fp.FpcaError, match="only 4 allowed"):
        ctx.scca_fit(5e-3, 1e-3, 5, np.ones((4, 5)))
    # fit before prepare; a context that is one shard of several
    with fp.Context.from_bed(HM3 + ".bed", n, accum="auto") as c2:
        with pytest.raises(fp.FpcaError, match="no phenotypes prepared") as e:
            c2.scca_fit(1e-3, 1e-3, 2, V0[:, :2])
        assert e.value.code == -1
        c2.set_rank(2, 0)
        with pytest.raises(fp.FpcaError, match="one shard of several") as e:
            c2.scca_prepare(Y)
        assert e.value.code == -1
        c2.set_rank(1, 0)
        c2.scca_prepare(Y)
        c2.set_rank(2, 1)
        with pytest.raises(fp.FpcaError, match="one shard of several"):
            c2.scca_fit(1e-3, 1e-3, 2, V0[:, :2])


def pack_codes(codes):
    """codes: (P, N) raw PLINK 2-bit codes -> the packed records."""
    P, N = codes.shape
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    return (c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)).astype(np.uint8)


def test_larger_problem(fp, O):
    """6,000 x 40,000 (the restatement's dense X is 1.9 GB and it runs in about a minute on 16 CPUs), k = 10, ndim = 2: same bounds."""
    N, P, k = 6000, 40000, 10
    rng = np.random.default_rng(11)
    maf = rng.uniform(0.05, 0.5, P)
    u = rng.random((P, N), dtype=np.float32)
    q = (maf * maf).astype(np.float32)[:, None]
    h = (maf * (2 - maf)).astype(np.float32)[:, None]  # P(dosage >= 1)
    codes = np.where(u < q, 0, np.where(u < h, 2, 3)).astype(np.uint8)  # hom A1, het, hom A2
    codes[rng.random((P, N), dtype=np.float32) < 0.002] = 1  # missing
    del u
    packed = pack_codes(codes)
    del codes
    X = O.OracleData(packed=packed, N=N, P=P, stand="binom2").dense()
    causal = rng.choice(P, 100, replace=False)
    Y = X[:, causal] @ rng.standard_normal((100, k)) + 3 * rng.standard_normal((N, k))
    V0 = rng.standard_normal((k, 2))
    Ys, _ = O.standardise(Y, "sd")
    with fp.Context.from_packed(packed, N, P, accum="auto") as ctx:
        ctx.scca_prepare(Y, standy="sd")
        got = ctx.scca_fit(1e-2, 1e-3, 2, V0, tol=1e-9)
    ref = run_ref(X, Ys, "n1", 1e-2, 1e-3, V0, tol=1e-9)
    assert ref["converged"], ref["iters"]
    compare(got, ref, 1e-9, "larger")


def test_dense_context(fp, O):
    """Context.from_dense (standx "sd", NaN = missing) against the in-memory restatement."""
    rng = np.random.default_rng(21)
    N, P, k = 500, 800, 12
    Xr = rng.standard_normal((N, P)) * rng.uniform(0.5, 2, P) + rng.uniform(-1, 1, P)
    Xr[rng.random((N, P)) < 0.01] = np.nan
    X, _ = O.standardise(Xr, "sd")
    B = np.zeros((P, k))
    B[rng.choice(P, 30, replace=False)] = rng.standard_normal((30, k))
    Y = X @ B + 3 * rng.standard_normal((N, k))
    V0 = rng.standard_normal((k, 3))
    Ys, _ = O.standardise(Y, "sd")
    ref = run_ref(X, Ys, "n1", 1e-2, 1e-2, V0, tol=1e-9)
    assert ref["converged"], ref["iters"]
    with fp.Context.from_dense(Xr, stand="sd") as ctx:
        ctx.scca_prepare(Y, standy="sd")
        compare(ctx.scca_fit(1e-2, 1e-2, 3, V0, tol=1e-9), ref, 1e-9, "dense")
    s = fp.scca(Xr, Y, lambda1=1e-2, lambda2=1e-2, standx="sd", standy="sd", ndim=3, tol=1e-9, V=V0)
    compare(s, ref, 1e-9, "dense scca()")
