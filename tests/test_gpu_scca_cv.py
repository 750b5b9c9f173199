"""fpca_scca_cv / flashpca_amd.cv_scca on the GPU against cv.scca() (flashpcaR/R/scca.R:410-557) restated in numpy AS WRITTEN: per fold
the training rows are RE-PACKED and given to the CPU oracle (dense matrix, mean / sd), the held-out rows go through a second oracle
object with the training mean / sd preloaded, Y is standardised by the oracle on the training rows, and every model is fitted by the
loop of tests/test_gpu_scca.py (reference_scca: two products per iteration, never via C = X'Y), copied here.  The yardstick never calls
the library.

Bounds.  For equal iteration counts the per-fit bound of tests/test_gpu_scca.py is 1e-12 per entry of U and V; a prediction is a sum of
P = 1.4e4 terms of size O(1) times those entries, so 2e-8 relative to the largest entry of xpred (ypred) and 1e-7 on corr follow.
Iteration counts are equal or exactly one apart in at most ONE fit of a run (the rule and the reasoning of tests/test_gpu_scca.py); for a
fit one apart the bound on its predictions is 2 sqrt(P) tol relative.  Fold counts and the training mean / sd are held to array_equal.
Every test prints what it measured (pytest -s).
Measured on the MI355X: the hapmap3_data fixture, all 35 fits on the yardstick's own iteration counts, max |dxpred| 4.0e-15, |dypred|
7.7e-15 of the largest entry, |dcorr| 7.8e-16 (auto and fp64 alike); standy "none" 6.6e-16 / 2.4e-15 / 3.3e-16; maxiter 80 3.8e-15 /
5.9e-15 / 4.4e-16; the 6,000 x 40,000 case (hybrid route) 2.2e-14 / 1.6e-14 / 3.3e-16; the public route as second witness at most
1.3e-15.  The one-apart branch was taken by no fit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
CHR1 = os.path.join(GOLD, "data_chr1")
B_PRED, B_CORR = 2e-8, 1e-7
L1S, L2S = (1e-3, 5e-3, 2e-2), (1e-3, 1e-2)


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


# ---- the yardstick -----------------------------------------------------------------------------------------
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
    """tests/test_gpu_scca.py::reference_scca, copied: randompca.cpp:402-528 on the standardised X (missing = 0) and the standardised
    Ys, with this project's edge rules where the reference has none."""
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
    return dict(U=U, V=V, d=d, iters=iters, converged=status == "ok", status=status, nzero_x=(U != 0).sum(axis=0), nzero_y=(V != 0).sum(axis=0))


def pack_codes(codes):
    """codes: (P, N) raw PLINK 2-bit codes -> the packed records."""
    P, N = codes.shape
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    return (c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)).astype(np.uint8)


def unpack_codes(packed, N, P):
    packed = np.asarray(packed, dtype=np.uint8).reshape(P, -1)
    return np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(P, -1)[:, :N]


def read_bed_codes(prefix, N):
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:]
    P = raw.size // ((N + 3) // 4)
    return unpack_codes(raw, N, P), P


def transform_y(Yrows, ms, stand):
    """util.cpp:24-110 applied to new rows with the training mean / sd `ms` (p x 2)."""
    mean, sd = ms[:, 0], ms[:, 1]
    nan = np.isnan(Yrows)
    if stand == "none":
        return np.where(nan, mean, Yrows)
    if stand == "center":
        return np.where(nan, 0.0, Yrows - mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = np.where(sd > 1e-9, (Yrows - mean) / sd, mean)
    return np.where(nan, 0.0, Z)


def fold_data(O, codes, folds, f, stand):
    """The oracle's view of fold f: X of the re-packed training rows, their mean / sd, X of the held-out rows under that mean / sd."""
    P = codes.shape[0]
    w = folds != f
    od = O.OracleData(packed=pack_codes(codes[:, w]), N=int(w.sum()), P=P, stand=stand)
    Xt, ms = od.dense(), od.meansd()
    Xh = np.zeros((0, P))
    if (~w).any():
        oh = O.OracleData(packed=pack_codes(codes[:, ~w]), N=int((~w).sum()), P=P, stand=stand)
        oh.set_preloaded_meansd(ms)
        Xh = oh.dense()
    return w, Xt, ms, Xh


def cv_yardstick(O, codes, Y, folds, nfolds, l1s, l2s, ndim, V0s, stand="binom2", standy="sd", divisor="n1", warm=1e-12, maxiter=1000, tol=1e-4,
                 opt_dim=1, use_c=False, cap_margin=0):
    """scca.R:410-557 with the departures of DESIGN 7c (training standardisation of the held-out rows).  cap_margin > 0: every fit is
    also classified against the cap -- one that converged within cap_margin iterations of maxiter, or stopped at maxiter and would
    have converged within cap_margin more, is listed in "near_cap" (two correct implementations could disagree on it)."""
    P, N = codes.shape
    n1, n2 = len(l1s), len(l2s)
    xpred, ypred = np.zeros((N, ndim, n1, n2)), np.zeros((N, ndim, n1, n2))
    conv = np.zeros((nfolds, n1, n2), dtype=bool)
    iters = np.zeros((nfolds, n1, n2, ndim), dtype=int)
    witers = np.zeros((nfolds, ndim), dtype=int)
    nzx, nzy = np.zeros((nfolds, ndim, n1, n2)), np.zeros((nfolds, ndim, n1, n2))
    near_cap = []

    def fit(Xt, Yt, a, b, V, what):
        r = reference_scca(Xt, Yt, divisor, a, b, V, maxiter=maxiter, tol=tol, use_c=use_c)
        if cap_margin and r["converged"] and r["iters"].max() >= maxiter - cap_margin:
            near_cap.append((what, r["iters"].tolist()))
        if cap_margin and r["status"] == "maxiter reached":
            r2 = reference_scca(Xt, Yt, divisor, a, b, V, maxiter=maxiter + cap_margin, tol=tol, use_c=use_c)
            j = int(np.argmax(r["iters"] >= maxiter))
            if r2["iters"][j] < maxiter + cap_margin:
                near_cap.append((what, r2["iters"].tolist()))
        return r

    for f in range(nfolds):
        w, Xt, ms, Xh = fold_data(O, codes, folds, f, stand)
        Yt, yms = O.standardise(Y[w], standy)
        Yho = transform_y(Y[~w], yms, standy)
        V = V0s[f]
        if warm is not None and warm >= 0:
            r0 = fit(Xt, Yt, warm, warm, V0s[f], (f, "warm"))
            V, witers[f] = r0["V"], r0["iters"]
        for i, a in enumerate(l1s):
            for j, b in enumerate(l2s):
                r = fit(Xt, Yt, a, b, V, (f, i, j))
                conv[f, i, j], iters[f, i, j] = r["converged"], r["iters"]
                nzx[f, :, i, j], nzy[f, :, i, j] = r["nzero_x"], r["nzero_y"]
                xpred[~w, :, i, j] = Xh @ r["U"] if r["converged"] else np.nan
                ypred[~w, :, i, j] = Yho @ r["V"] if r["converged"] else np.nan
    corr = np.full((ndim, n1, n2), np.nan)
    for q in range(ndim):
        for i in range(n1):
            for j in range(n2):
                x, y = xpred[:, q, i, j], ypred[:, q, i, j]
                if not (np.isnan(x).any() or np.isnan(y).any()) and x.std() > 0 and y.std() > 0:
                    corr[q, i, j] = np.corrcoef(x, y)[0, 1]
    best = dict(best_corr=np.nan, best_lambda1=np.nan, best_lambda2=np.nan)
    r = corr[opt_dim - 1]
    if np.isfinite(r).any():
        mx = np.nanmax(r)
        i, j = [(i, j) for j in range(n2) for i in range(n1) if r[i, j] == mx][0]  # which(): lambda1's index fastest, first hit
        best = dict(best_corr=mx, best_lambda1=l1s[i], best_lambda2=l2s[j])
    return dict(xpred=xpred, ypred=ypred, converged=conv, iters=iters, warm_iters=witers, nzero_x=nzx.mean(axis=0), nzero_y=nzy.mean(axis=0),
                corr=corr, near_cap=near_cap, **best)


def compare_cv(got, ref, P, tol, label, folds):
    """Prints what it measured, then asserts the module's bounds.  Returns the number of fits whose iteration counts were one apart."""
    assert np.array_equal(got["converged"], ref["converged"]), (label, got["converged"], ref["converged"])
    gi = np.concatenate([got["iters"].reshape(got["iters"].shape[0], -1), got["warm_iters"]], axis=1)
    ri = np.concatenate([ref["iters"].reshape(ref["iters"].shape[0], -1), ref["warm_iters"]], axis=1)
    ndim = got["warm_iters"].shape[1]
    apart = np.abs(gi - ri).reshape(gi.shape[0], -1, ndim).max(axis=2)  # per fold and fit
    assert apart.max() <= 1 and (apart > 0).sum() <= 1, (label, "iteration counts", gi.tolist(), ri.tolist())
    n_apart = int((apart > 0).sum())
    nfolds, n1, n2 = got["converged"].shape
    off = apart[:, :n1 * n2].reshape(nfolds, n1, n2) > 0  # grid fits one apart (or started from a warm start that was)
    if n_apart and (apart[:, n1 * n2:] > 0).any():
        off[np.argmax(apart[:, n1 * n2:].max(axis=1) > 0)] = True
    assert np.array_equal(got["nzero_y"], ref["nzero_y"]) or n_apart, (label, got["nzero_y"], ref["nzero_y"])
    if not n_apart:
        assert np.array_equal(got["nzero_x"], ref["nzero_x"]), (label, got["nzero_x"], ref["nzero_x"])
    worst = dict(x=0.0, y=0.0)
    for name in ("xpred", "ypred"):
        g, r = got[name], ref[name]
        assert g.shape == r.shape and np.array_equal(np.isnan(g), np.isnan(r)), (label, name)
        scale = np.nanmax(np.abs(r))
        for f in range(nfolds):
            for i in range(n1):
                for j in range(n2):
                    rows = folds == f
                    if not rows.any() or not ref["converged"][f, i, j]:
                        continue
                    e = np.abs(g[rows, :, i, j] - r[rows, :, i, j]).max() / scale
                    bound = 2 * np.sqrt(P) * tol if off[f, i, j] else B_PRED
                    if not off[f, i, j]:
                        worst[name[0]] = max(worst[name[0]], e)
                    assert e <= bound, (label, name, f, i, j, e, bound)
    fin = np.isfinite(ref["corr"])
    assert np.array_equal(np.isfinite(got["corr"]), fin), (label, got["corr"], ref["corr"])
    dc = np.abs(got["corr"][fin] - ref["corr"][fin]).max() if fin.any() else 0.0
    print("%s: iterations %d..%d, fits one apart %d, max rel |dxpred| %.3g |dypred| %.3g, max |dcorr| %.3g, corr[0] %s" % (
        label, ri[ri > 0].min() if (ri > 0).any() else 0, ri.max(), n_apart, worst["x"], worst["y"], dc, np.round(ref["corr"][0].ravel(), 4).tolist()))
    assert dc <= (B_CORR if not n_apart else 2 * np.sqrt(P) * tol), (label, dc)
    for kk in ("best_lambda1", "best_lambda2"):
        assert got[kk] == ref[kk] or (np.isnan(got[kk]) and np.isnan(ref[kk])), (label, kk, got[kk], ref[kk])
    if np.isfinite(ref["best_corr"]):
        assert abs(got["best_corr"] - ref["best_corr"]) <= B_CORR
    return n_apart


def hm3_phenotypes(X, stand, k=20, seed=1):
    """tests/test_gpu_scca.py::hm3_phenotypes, copied."""
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
    """The parity fixture: hapmap3_data (957 x 14,389), 5 folds from default_rng(7), V0_f from default_rng(100 + f)."""
    n = fp.count_fam_rows(HM3 + ".fam")
    codes, P = read_bed_codes(HM3, n)
    X = O.OracleData(HM3 + ".bed", n, "binom2").dense()
    folds = np.random.default_rng(7).integers(0, 5, n)
    assert np.bincount(folds).tolist() == [188, 177, 188, 191, 213]
    V0s = np.stack([np.random.default_rng(100 + f).standard_normal((20, 3)) for f in range(5)])
    return dict(n=n, P=P, codes=codes, X=X, folds=folds, V0s=V0s)


_REF = {}


def hm3_reference(O, hm3, stand, maxiter=1000):
    if (stand, maxiter) not in _REF:
        Y, _ = hm3_phenotypes(hm3["X"], stand)
        _REF[stand, maxiter] = (Y, cv_yardstick(O, hm3["codes"], Y, hm3["folds"], 5, L1S, L2S, 3, hm3["V0s"], standy=stand, tol=1e-6, maxiter=maxiter,
                                                cap_margin=2 if maxiter < 1000 else 0))
    return _REF[stand, maxiter]


# ---- 1. fold counts, bit for bit ------------------------------------------------------------------------------
def check_fold_stats(fp, O, ctx, codes, nfolds, seed, stand="binom2", empty=None):
    P, N = codes.shape
    folds = np.random.default_rng(seed).integers(0, nfolds, N)
    if empty is not None:
        folds[folds == empty] = (empty + 1) % nfolds
    which = [0, nfolds - 1] + ([empty] if empty is not None else [])
    for wf in which:
        counts, ms = ctx.fold_stats(folds, nfolds, wf)
        ref = np.stack([np.stack([((codes == raw) & (folds == f)).sum(axis=1) for raw in (3, 2, 0)], axis=1) for f in range(nfolds)])
        assert np.array_equal(counts, ref), (nfolds, wf)
        w = folds != wf
        od = O.OracleData(packed=pack_codes(codes[:, w]), N=int(w.sum()), P=P, stand=stand)
        od.dense()  # (the oracle, like the reference, takes mean / sd on its first visit of a SNP)
        assert np.array_equal(ms, od.meansd(), equal_nan=True), (nfolds, wf, np.abs(ms - od.meansd()).max())
    return folds


@pytest.mark.parametrize("nfolds", [2, 5, 10, 64])
def test_fold_counts_bit_for_bit(fp, O, nfolds):
    """k_fold_counts / k_fold_meansd on hapmap3_data (957 x 14,389, 0.15 % missing), data_chr1 and a synthetic matrix with 2 % missing
    calls whose N is a multiple of neither 4 nor 512; one run with an empty fold.  Counts equal numpy's, training mean / sd equal the
    oracle's on the re-packed training rows, bit for bit; the context's own statistics are untouched."""
    for prefix in (HM3, CHR1):
        n = fp.count_fam_rows(prefix + ".fam")
        codes, P = read_bed_codes(prefix, n)
        with fp.Context.from_bed(prefix + ".bed", n, accum="auto") as ctx:
            before = ctx.stats()
            check_fold_stats(fp, O, ctx, codes, nfolds, 10 + nfolds, empty=1 if nfolds == 5 else None)
            after = ctx.stats()
            assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    N, P = 2731, 1500
    for stand in ("binom2", "binom"):
        with fp.Context.synthetic(N, P, n_pop=4, missing_rate=0.02, stand=stand, accum="fp64") as ctx:
            codes = unpack_codes(ctx.download_packed(), N, P)
            assert 0.015 < (codes == 1).mean() < 0.025
            check_fold_stats(fp, O, ctx, codes, nfolds, 20 + nfolds, stand=stand, empty=0 if nfolds == 10 else None)


# ---- 2. parity of the whole procedure ------------------------------------------------------------------------
@pytest.mark.parametrize("stand,accum", [("sd", "auto"), ("sd", "fp64"), ("none", "auto")])
def test_parity_with_cv_scca_as_written(fp, O, hm3, stand, accum):
    """hapmap3_data, k = 20, 5 folds, warm start 1e-12, ndim 3, 3 x 2 penalties, divisor n1, tol 1e-6: all 30 fold x cell models and
    the 5 warm starts converge in the yardstick (checked below), every cell takes part.  "none": scaled and shifted phenotypes with
    2 % NaN, imputed by the training-row mean.
    Measured on the MI355X: max |dxpred| 4.0e-15, |dypred| 7.7e-15 relative, |dcorr| 7.8e-16 ("sd", both arithmetics); 6.6e-16, 2.4e-15,
    3.3e-16 ("none"); equal iteration counts in all 35 fits."""
    Y, ref = hm3_reference(O, hm3, stand)
    assert ref["converged"].all() and ref["warm_iters"].min() > 0 and ref["iters"].min() >= 1
    with fp.Context.from_bed(HM3 + ".bed", hm3["n"], accum=accum) as ctx:
        got = ctx.scca_cv(Y, hm3["folds"], L1S, L2S, 3, hm3["V0s"], standy=stand, tol=1e-6, return_pred=True)
    compare_cv(got, ref, hm3["P"], 1e-6, "parity %s %s" % (stand, accum), hm3["folds"])
    if stand == "sd":
        assert (got["best_lambda1"], got["best_lambda2"]) == (1e-3, 1e-3)
        assert np.argmax(got["corr"][2].max(axis=1)) == 2  # dimension 3 peaks at lambda1 = 2e-2
    assert not np.isnan(got["xpred"]).any() and not np.isnan(got["nzero_x"]).any()


# ---- 3. not-converged cells propagate as in R -----------------------------------------------------------------
def test_unconverged_cells_propagate(fp, O, hm3):
    """maxiter = 80 on the same fixture: some fold x cell models stop at the cap; the yardstick confirms first that no fit's own
    stopping iteration lies within 2 of it (otherwise two correct implementations could disagree on `converged`)."""
    Y, ref = hm3_reference(O, hm3, "sd", maxiter=80)
    assert not ref["near_cap"], ref["near_cap"]
    allc = ref["converged"].all(axis=0)
    print("converged models %d / 30, cells converged in every fold: %s" % (ref["converged"].sum(), np.argwhere(allc).tolist()))
    assert allc.sum() == 1 and allc[0, 0] and 0.5 < ref["converged"].mean() < 0.9
    with fp.Context.from_bed(HM3 + ".bed", hm3["n"], accum="auto") as ctx:
        got = ctx.scca_cv(Y, hm3["folds"], L1S, L2S, 3, hm3["V0s"], standy="sd", tol=1e-6, maxiter=80, return_pred=True)
    compare_cv(got, ref, hm3["P"], 1e-6, "maxiter 80", hm3["folds"])
    assert np.array_equal(np.isnan(got["corr"]), np.broadcast_to(~allc, got["corr"].shape))
    assert (got["best_lambda1"], got["best_lambda2"]) == (1e-3, 1e-3) and got["best_corr"] == got["corr"][0, 0, 0]
    for f in range(5):
        rows = hm3["folds"] == f
        for i in range(3):
            for j in range(2):
                bad = ~ref["converged"][f, i, j]
                assert np.isnan(got["xpred"][rows, :, i, j]).all() == bad and np.isnan(got["xpred"][rows, :, i, j]).any() == bad
                assert np.isnan(got["ypred"][rows, :, i, j]).all() == bad and np.isnan(got["ypred"][rows, :, i, j]).any() == bad


# ---- 4. the context is left as it was ------------------------------------------------------------------------
def context_fingerprint(ctx, Y, B):
    ms, tr = ctx.stats()
    return dict(ms=ms, tr=np.array(tr), xxt=ctx.apply_xxt(B), ucca=ctx.ucca(Y[:, :4], standy="sd"), pca=ctx.pca(ndim=3)["d"], pcaU=ctx.pca(ndim=3)["U"],
                mode=np.array(ctx.missing_mode(16)))


@pytest.mark.parametrize("accum", ["auto", "fp64"])
def test_context_is_left_as_it_was(fp, O, hm3, accum):
    Y, _ = hm3_phenotypes(hm3["X"], "sd")
    B = np.random.default_rng(4).standard_normal((hm3["n"], 16))
    with fp.Context.from_bed(HM3 + ".bed", hm3["n"], accum=accum) as ctx:
        before = context_fingerprint(ctx, Y, B)
        ctx.scca_cv(Y, hm3["folds"], L1S[:2], L2S[:1], 2, hm3["V0s"][:, :, :2], standy="sd", tol=1e-4)
        after = context_fingerprint(ctx, Y, B)
        for kk in before:
            assert np.array_equal(before[kk], after[kk], equal_nan=True), kk
        for bad in (dict(lambda1=[1e-3, np.nan]), dict(opt_dim=3), dict(ndim=25)):
            a = dict(lambda1=L1S[:2], ndim=2, opt_dim=1)
            a.update(bad)
            with pytest.raises(fp.FpcaError) as e:
                ctx.scca_cv(Y, hm3["folds"], a["lambda1"], L2S[:1], a["ndim"], np.ones((20, max(a["ndim"], 1))), opt_dim=a["opt_dim"])
            assert e.value.code == -1
        after = context_fingerprint(ctx, Y, B)
        for kk in before:
            assert np.array_equal(before[kk], after[kk], equal_nan=True), kk
    # a standardisation the caller had preloaded comes back too
    with fp.Context.from_bed(HM3 + ".bed", hm3["n"], accum=accum) as ctx:
        ms = ctx.stats()[0].copy()
        ms[:, 0] += 0.01
        ctx.set_meansd(ms)
        x0 = ctx.apply_xxt(B)
        ctx.scca_cv(Y, hm3["folds"], L1S[:1], L2S[:1], 2, hm3["V0s"][:, :, :2], standy="sd")
        assert np.array_equal(ctx.stats()[0], ms) and np.array_equal(ctx.apply_xxt(B), x0)


# ---- 5. equivalence with the existing public route -----------------------------------------------------------
def test_equivalence_with_the_public_scca_route(fp, O, hm3):
    """Two folds, three cells each, repeated through Context.from_packed on the re-packed training rows + scca_prepare + scca_fit, and a
    projection context on the held-out rows with the training mean / sd: a second witness beside the numpy yardstick."""
    Y, _ = hm3_phenotypes(hm3["X"], "sd")
    folds, codes, P = hm3["folds"], hm3["codes"], hm3["P"]
    with fp.Context.from_bed(HM3 + ".bed", hm3["n"], accum="auto") as ctx:
        got = ctx.scca_cv(Y, folds, L1S, L2S, 3, hm3["V0s"], standy="sd", tol=1e-6, return_pred=True)
    scale_x, scale_y = np.abs(got["xpred"]).max(), np.abs(got["ypred"]).max()
    for f in (0, 3):
        w = folds != f
        Yt, yms = O.standardise(Y[w], "sd")
        Yho = transform_y(Y[~w], yms, "sd")
        with fp.Context.from_packed(pack_codes(codes[:, w]), int(w.sum()), P, accum="auto") as ct, \
                fp.Context.from_packed(pack_codes(codes[:, ~w]), int((~w).sum()), P, accum="auto") as ch:
            ch.set_meansd(ct.stats()[0])
            ct.scca_prepare(Y[w], standy="sd", divisor="n1")
            warm = ct.scca_fit(1e-12, 1e-12, 3, hm3["V0s"][f], tol=1e-6)
            assert np.abs(warm["iters"] - got["warm_iters"][f]).max() <= 1
            for i, j in ((0, 0), (1, 1), (2, 0)):
                m = ct.scca_fit(L1S[i], L2S[j], 3, warm["V"], tol=1e-6)
                assert m["converged"] and np.abs(m["iters"] - got["iters"][f, i, j]).max() <= 1, (f, i, j, m["iters"], got["iters"][f, i, j])
                same = np.array_equal(m["iters"], got["iters"][f, i, j]) and np.array_equal(warm["iters"], got["warm_iters"][f])
                ex = np.abs(ch.apply_x(m["U"]) - got["xpred"][~w, :, i, j]).max() / scale_x
                ey = np.abs(Yho @ m["V"] - got["ypred"][~w, :, i, j]).max() / scale_y
                print("fold %d cell (%d, %d): iters %s, rel |dxpred| %.3g |dypred| %.3g" % (f, i, j, m["iters"].tolist(), ex, ey))
                bound = B_PRED if same else 2 * np.sqrt(P) * 1e-6
                assert ex <= bound and ey <= bound, (f, i, j, ex, ey)


# ---- 6. refusals on the device --------------------------------------------------------------------------------
def test_refusals(fp, O, hm3):
    Y, _ = hm3_phenotypes(hm3["X"], "sd", k=6)
    n, folds = hm3["n"], hm3["folds"]
    V0 = np.ones((6, 2))
    with fp.Context.from_bed(HM3 + ".bed", n, accum="auto") as ctx:
        def call(fold=folds, nfolds=5, ndim=2, opt_dim=1, l1=(1e-3,)):
            f8 = np.ascontiguousarray(fold, dtype=np.uint8)
            l1a, l2a = np.asarray(l1, dtype=np.float64), np.asarray([1e-3])
            Yf, V = np.asfortranarray(Y), np.asfortranarray(np.ones((6, max(ndim, 1))))
            p = fp.api._p
            return fp.lib().fpca_scca_cv(ctx.h, p(Yf), n, 6, p(f8), nfolds, p(l1a), l1a.size, p(l2a), 1, ndim, 1, 1, 50, 1e-4, p(V), 6, 0, 1e-12, opt_dim,
                                         *[None] * 11)

        bad = folds.copy()
        bad[5] = 7
        tiny = np.zeros(n, dtype=int)
        tiny[:3] = 1  # fold 0 leaves 3 samples to train on
        for kw, msg in ((dict(fold=bad), "fold id 7"), (dict(nfolds=1, fold=np.zeros(n, int)), "nfolds must be between 2 and 64"),
                        (dict(nfolds=65), "nfolds must be between 2 and 64"), (dict(opt_dim=0), "opt_dim must be between 1 and ndim"),
                        (dict(opt_dim=3), "opt_dim must be between 1 and ndim"), (dict(fold=tiny, nfolds=2, ndim=4), "only 3 allowed"),
                        (dict(l1=(-1.0,)), "lambda1 must be non-negative"), (dict(l1=(np.inf,)), "lambda1 must be non-negative"),
                        (dict(ndim=0), "ndim can't be less than 1")):
            assert call(**kw) == -1, kw
            assert msg in fp.lib().fpca_last_error().decode(), (kw, fp.lib().fpca_last_error())
        ctx.set_rank(2, 0)
        assert call() == -1 and "one shard of several" in fp.lib().fpca_last_error().decode()
        ctx.set_rank(1, 0)
        # an empty fold succeeds: it trains on everything and predicts nothing
        f6 = np.where(folds == 2, 5, folds)
        got = ctx.scca_cv(Y, f6, [1e-3], [1e-3], 2, V0, standy="sd", return_pred=True)
        assert got["converged"].shape == (6, 1, 1) and got["converged"][2, 0, 0] and np.isfinite(got["corr"]).all()
        one = np.zeros(n, dtype=int)
        one[0] = 1
        assert call(fold=np.ones(n, int), nfolds=2) == -1 and "fewer than two samples" in fp.lib().fpca_last_error().decode()
    with fp.Context.from_dense(hm3["X"][:, :200], stand="none") as cd:
        with pytest.raises(fp.FpcaError, match="dense matrix") as e:
            cd.scca_cv(Y, folds, [1e-3], [1e-3], 2, V0)
        assert e.value.code == -1


# ---- 7. reproducibility -----------------------------------------------------------------------------------
def test_two_calls_are_bit_identical(fp, hm3):
    Y, _ = hm3_phenotypes(hm3["X"], "sd")
    with fp.Context.from_bed(HM3 + ".bed", hm3["n"], accum="auto") as ctx:
        a = ctx.scca_cv(Y, hm3["folds"], L1S, L2S, 3, hm3["V0s"], standy="sd", tol=1e-6, return_pred=True)
        b = ctx.scca_cv(Y, hm3["folds"], L1S, L2S, 3, hm3["V0s"], standy="sd", tol=1e-6, return_pred=True)
    for kk in ("corr", "xpred", "ypred", "iters", "nzero_x", "nzero_y"):
        assert np.array_equal(a[kk], b[kk], equal_nan=True), kk
    # the R-style front end: R's field names, folds 1 .. nfolds, reproducible from its seed
    r1 = fp.cv_scca(HM3, Y, lambda1=L1S[:2], lambda2=L2S[:1], ndim=2, nfolds=4, standy="sd", seed=3)
    r2 = fp.cv_scca(HM3, Y, lambda1=L1S[:2], lambda2=L2S[:1], ndim=2, nfolds=4, standy="sd", seed=3)
    for kk in ("ndim", "lambda1", "lambda2", "opt_dim", "nfolds", "best_lambda1", "best_lambda2", "best_corr", "corr", "nzero_x", "nzero_y", "converged",
               "iters", "folds"):
        assert kk in r1
    assert r1["corr"].shape == (2, 2, 1) and set(r1["folds"]) == {1, 2, 3, 4} and np.array_equal(r1["corr"], r2["corr"], equal_nan=True)
    assert np.isfinite(r1["best_corr"]) and r1["best_corr"] > 0.3
    # a numeric 0 / 1 / 2 / NaN matrix is packed on the host: the same numbers as the fileset
    D = np.select([hm3["codes"].T == 3, hm3["codes"].T == 2, hm3["codes"].T == 0], [0.0, 1.0, 2.0], np.nan)
    with pytest.warns(UserWarning):
        r3 = fp.cv_scca(D, Y, lambda1=L1S[:2], lambda2=L2S[:1], ndim=2, nfolds=4, standy="sd", seed=3)
    assert np.array_equal(r1["corr"], r3["corr"], equal_nan=True)


# ---- 8. a larger, missing-heavy case --------------------------------------------------------------------------
LARGER = dict(N=6000, P=40000, k=10, l1s=(5e-3, 1e-2), l2s=(1e-3, 1e-2), tol=1e-6)


def larger_problem():
    """6,000 x 40,000 as tests/test_gpu_scca.py::test_larger_problem builds its own, the missing calls concentrated: 5 % of the SNPs
    at 10-30 % missing, the rest at most 0.1 %."""
    N, P, k = LARGER["N"], LARGER["P"], LARGER["k"]
    rng = np.random.default_rng(12)
    maf = rng.uniform(0.05, 0.5, P)
    u = rng.random((P, N), dtype=np.float32)
    q = (maf * maf).astype(np.float32)[:, None]
    h = (maf * (2 - maf)).astype(np.float32)[:, None]
    codes = np.where(u < q, 0, np.where(u < h, 2, 3)).astype(np.uint8)
    rate = np.where(rng.random(P) < 0.05, rng.uniform(0.10, 0.30, P), rng.uniform(0, 0.001, P)).astype(np.float32)[:, None]
    codes[rng.random((P, N), dtype=np.float32) < rate] = 1
    del u
    folds = rng.integers(0, 4, N)
    V0s = rng.standard_normal((4, k, 2))
    return codes, folds, V0s, rng


def larger_phenotypes(X, rng):
    P, k = LARGER["P"], LARGER["k"]
    causal = rng.choice(P, 100, replace=False)
    return X[:, causal] @ rng.standard_normal((100, k)) + 3 * rng.standard_normal((X.shape[0], k))


def test_larger_missing_heavy_problem(fp, O):
    """4 folds, a 2 x 2 grid, ndim 2 against the yardstick with the assertions of the parity test; the route of the exact-integer path's
    missing-call indicator while mean / sd were swapped is printed and asserted (3 sparse or 4 hybrid; otherwise the run is repeated on
    the test-hooks build with the hybrid route forced).  The yardstick runs the restated loop on C here (use_c): one as-written fit at
    this size takes about a minute (tests/test_gpu_scca.py::test_larger_problem), there are twenty, and the two loops differ by 1.5e-15
    (DESIGN 7b).  The penalties were checked on the CPU:
    all 16 models and the 4 warm starts converge, in 27 .. 280 iterations.  Measured on the MI355X: route 4 (hybrid), 2.2e-14 / 1.6e-14 /
    3.3e-16."""
    N, P = LARGER["N"], LARGER["P"]
    codes, folds, V0s, rng = larger_problem()
    packed = pack_codes(codes)
    X = O.OracleData(packed=packed, N=N, P=P, stand="binom2").dense()
    Y = larger_phenotypes(X, rng)
    del X
    ref = cv_yardstick(O, codes, Y, folds, 4, LARGER["l1s"], LARGER["l2s"], 2, V0s, standy="sd", tol=LARGER["tol"], use_c=True)
    assert ref["converged"].all(), ref["iters"]
    with fp.Context.from_packed(packed, N, P, accum="auto") as ctx:
        mode = ctx.missing_mode(16)
        print("missing-call route of the exact-integer path: %d" % mode)
        got = ctx.scca_cv(Y, folds, LARGER["l1s"], LARGER["l2s"], 2, V0s, standy="sd", tol=LARGER["tol"], return_pred=True)
        assert ctx.missing_mode(16) == mode
    compare_cv(got, ref, P, LARGER["tol"], "larger (route %d)" % mode, folds)
    if mode not in (3, 4):
        import flashpca_amd._lib as _lib

        os.environ["FPCA_I8_MODE"] = "4"
        try:
            with _lib.test_hooks():
                with fp.Context.from_packed(packed, N, P, accum="auto") as ctx:
                    mode2 = ctx.missing_mode(16)
                    print("forced route: %d" % mode2)
                    assert mode2 in (3, 4)
                    got = ctx.scca_cv(Y, folds, LARGER["l1s"], LARGER["l2s"], 2, V0s, standy="sd", tol=LARGER["tol"], return_pred=True)
        finally:
            del os.environ["FPCA_I8_MODE"]
        compare_cv(got, ref, P, LARGER["tol"], "larger (forced route %d)" % mode2, folds)
