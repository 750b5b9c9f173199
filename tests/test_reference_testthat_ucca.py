"""flashpcaR/tests/testthat/test_ucca.R restated against flashpca_amd.ucca() (GPU): the two test_that blocks (binom and binom2; the
matrix input with standx="none" and the PLINK input) against lm() / anova() restated with numpy least squares and scipy's F
distribution, at the script's tolerance test.tol = 1e-4 -- and at tight tolerances: R^2 and F within 1e-10 relative, P within 1e-8
relative, log P -- plus the input-checking block.  hm3.chr1$bed of the R package is tests/golden/data_chr1."""
import os

import numpy as np
import pytest
from scipy import special, stats

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BEDF = os.path.join(GOLD, "data_chr1")
K, TOL = 15, 1e-4  # test_ucca.R:5, :19


def hm3_chr1_bed():
    n = len(open(BEDF + ".fam").read().splitlines())
    raw = np.fromfile(BEDF + ".bed", dtype=np.uint8)[3:]
    raw = raw.reshape(raw.size // ((n + 3) // 4), -1)
    codes = np.empty((raw.shape[0], raw.shape[1] * 4), dtype=np.uint8)
    for s in range(4):
        codes[:, s::4] = (raw >> (2 * s)) & 3
    codes = codes[:, :n].T
    return np.where(codes == 0, 2.0, np.where(codes == 2, 1.0, np.where(codes == 3, 0.0, np.nan)))


def scale2(X, type_):
    """flashpcaR::scale2: type "1" = binom, "2" = binom2; missing -> 0."""
    p = np.nansum(X, axis=0) / (2 * np.sum(~np.isnan(X), axis=0))
    scale = np.sqrt(p * (1 - p)) if type_ == "1" else np.sqrt(2 * p * (1 - p))
    with np.errstate(invalid="ignore", divide="ignore"):
        S = (X - 2 * p) / scale
    S[np.isnan(S)] = 0
    return S


def r_scale(A):
    return (A - A.mean(axis=0)) / A.std(axis=0, ddof=1)


def lm_anova(X, Y):
    """lm(X[, i] ~ Y): R^2 (summary), F and Pr(>F) of the model row of anova() -- with k phenotypes in one model that row is the
    overall F test.  Zero-variance columns give NaN like R."""
    n, k = Y.shape
    A = np.column_stack([np.ones(n), Y])
    beta, *_ = np.linalg.lstsq(A, X, rcond=None)
    fitted = A @ beta
    xm = X.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = np.sum((fitted - xm) ** 2, axis=0) / np.sum((X - xm) ** 2, axis=0)
        F = r2 / (1 - r2) * (n - k - 1) / k
    P = stats.f.sf(F, k, n - k - 1)
    P_exact = special.betaincc(k / 2.0, (n - k - 1) / 2.0, r2)  # the same tail, exact in r2 (f.sf loses digits forming 1 - x)
    return r2, F, P, P_exact


def check(s, X, Y):
    r2_exp, F_exp, p_exp, p_exact = lm_anova(X, Y)
    res = s["result"]
    r2_obs, F_obs, p_obs = res[:, 0] ** 2, res[:, 1], res[:, 2]
    nan = np.isnan(r2_exp)
    assert np.array_equal(nan, np.isnan(r2_obs)) and np.array_equal(nan, np.isnan(p_obs))
    ok = ~nan
    assert ok.sum() > 0.9 * X.shape[1]
    # test_ucca.R:44-47 (all.equal: mean relative difference)
    for e, o in ((r2_exp, r2_obs), (F_exp, F_obs), (p_exp, p_obs), (np.log(p_exp), np.log(p_obs))):
        assert np.mean(np.abs(e[ok] - o[ok])) / np.mean(np.abs(e[ok])) < TOL
    # tight
    assert np.max(np.abs(r2_obs[ok] - r2_exp[ok]) / r2_exp[ok]) < 1e-10
    assert np.max(np.abs(F_obs[ok] - F_exp[ok]) / F_exp[ok]) < 1e-10
    assert np.max(np.abs(p_obs[ok] - p_exact[ok]) / p_exact[ok]) < 1e-8
    assert np.max(np.abs(np.log(p_obs[ok]) - np.log(p_exact[ok]))) < 1e-8


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.mark.parametrize("standx,type_", [("binom", "1"), ("binom2", "2")])
def test_ucca_matrix_and_plink(fp, standx, type_):  # test_ucca.R:50-78
    X = scale2(hm3_chr1_bed(), type_)
    n, p = X.shape
    rng = np.random.default_rng(7 if standx == "binom" else 8)
    By = rng.standard_normal((p, K))
    Y = r_scale(X @ By + rng.standard_normal((n, K)))
    s1 = fp.ucca(X, Y, standx="none", standy="none")
    s2 = fp.ucca(BEDF, Y, standx=standx, standy="none")
    assert s1["result"].shape == (p, 3) and s2["result"].shape == (p, 3)
    assert s2["snp_ids"] == [l.split()[1] for l in open(BEDF + ".bim").read().splitlines()]
    check(s1, X, Y)
    check(s2, X, Y)


@pytest.mark.parametrize("k", [15, 64])
def test_ucca_uncentred_dosages(fp, k):
    """ucca(X, Y, standx="none") on the raw 0/1/2 dosages (missing calls mean-imputed by the standardisation): the SNP columns are
    NOT centred, so sum_i x_ij != 0 and den_j = sum x^2 - (sum x)^2 / N takes the ones column of [W | 1] -- in its own K2 chunk at
    k = 64.  lm's R^2 does not depend on centring X, so lm on the imputed dosages is the reference."""
    D = hm3_chr1_bed()
    n, p = D.shape
    Xi = np.where(np.isnan(D), np.nanmean(D, axis=0), D)
    assert np.mean(np.abs(Xi.sum(axis=0)) > 1.0) > 0.9
    rng = np.random.default_rng(100 + k)
    Y = r_scale(scale2(D, "2") @ rng.standard_normal((p, k)) + rng.standard_normal((n, k)))
    check(fp.ucca(D, Y, standx="none", standy="none"), Xi, Y)


def test_ucca_input_checking(fp):  # test_ucca.R:80-110
    X = scale2(hm3_chr1_bed(), "1")
    n = X.shape[0]
    rng = np.random.default_rng(9)
    Z = rng.standard_normal((n + 3, 10))
    with pytest.raises(ValueError):
        fp.ucca(X, Z, standx="none", standy="none")
    with pytest.raises(ValueError):
        fp.ucca(BEDF, Z, standx="binom2", standy="none")
    Z = rng.standard_normal((n, n + 3))
    with pytest.raises(ValueError):
        fp.ucca(X, Z, standx="none", standy="none")
    with pytest.raises(ValueError):
        fp.ucca(BEDF, Z, standx="binom2", standy="none")
    # the library's own refusals behind those: k > N - 2, a rank-deficient Y, a Y of the wrong height
    with fp.Context.from_bed(BEDF + ".bed", n, accum="auto") as ctx:
        with pytest.raises(fp.FpcaError, match="at least"):
            ctx.ucca(rng.standard_normal((n, n - 1)), standy="none")
        Yd = rng.standard_normal((n, 3))
        Yd[:, 2] = Yd[:, 0] - 2 * Yd[:, 1]
        with pytest.raises(fp.FpcaError, match="rank deficient"):
            ctx.ucca(Yd, standy="none")
        with pytest.raises(ValueError):
            ctx.ucca(rng.standard_normal((n - 1, 3)))
