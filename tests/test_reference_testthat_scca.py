"""flashpcaR/tests/testthat/test_scca.R restated against flashpca_amd.scca() (GPU), every block but cv.scca, at the script's own
tolerance test.tol = 1e-4 (expect_equal = all.equal: mean relative difference): self-self SCCA of X with X at tiny penalties gives
d = the top eigenvalues of X X' / (n - 1) and canonical correlations diag(cor(Px, Py)) = 1, for the matrix and the PLINK input, with
divisor "none", and with V given; SCCA of X with Y agrees between the two inputs in d, U[:, :2], V[:, :2] and the correlations;
d(n1) = d(none) / (n - 1); the input checks.  hm3.chr1$bed of the R package is tests/golden/data_chr1 (957 x 1,129)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BEDF = os.path.join(GOLD, "data_chr1")
K, L1, L2, TOL = 50, 1e-6, 1e-6, 1e-4  # test_scca.R:17, :27-29
NDIM = 5  # min(n, m, k, 5)


def hm3_chr1_bed():
    n = len(open(BEDF + ".fam").read().splitlines())
    raw = np.fromfile(BEDF + ".bed", dtype=np.uint8)[3:]
    raw = raw.reshape(raw.size // ((n + 3) // 4), -1)
    codes = np.empty((raw.shape[0], raw.shape[1] * 4), dtype=np.uint8)
    for s in range(4):
        codes[:, s::4] = (raw >> (2 * s)) & 3
    codes = codes[:, :n].T
    return np.where(codes == 0, 2.0, np.where(codes == 2, 1.0, np.where(codes == 3, 0.0, np.nan)))


def scale2(X):
    """flashpcaR::scale2, type "2" (binom2); missing -> 0."""
    p = np.nansum(X, axis=0) / (2 * np.sum(~np.isnan(X), axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        S = (X - 2 * p) / np.sqrt(2 * p * (1 - p))
    S[np.isnan(S)] = 0
    return S


def expect_equal(a, b, what=""):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    rel = np.mean(np.abs(a - b)) / np.mean(np.abs(a))
    print("%s: mean relative difference %.3g" % (what, rel))
    assert rel < TOL, (what, rel)


def diag_cor(A, B):
    A, B = A - A.mean(axis=0), B - B.mean(axis=0)
    return np.sum(A * B, axis=0) / np.sqrt(np.sum(A * A, axis=0) * np.sum(B * B, axis=0))


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def data():
    X = scale2(hm3_chr1_bed())
    n, m = X.shape
    rng = np.random.default_rng(31)
    Y = X @ rng.standard_normal((m, K)) + rng.standard_normal((n, K))
    Y = (Y - Y.mean(axis=0)) / Y.std(axis=0, ddof=1)
    return X, Y, rng


@pytest.mark.parametrize("divisor,given_v", [("n1", False), ("none", False), ("n1", True)])
def test_self_self_scca(fp, data, divisor, given_v):  # test_scca.R:32-89
    X, _, rng = data
    n, m = X.shape
    ev = np.linalg.eigvalsh(X @ X.T / ((n - 1) if divisor == "n1" else 1.0))[::-1][:NDIM]
    V = rng.standard_normal((m, NDIM)) if given_v else None
    s1 = fp.scca(X, X, lambda1=L1, lambda2=L2, ndim=NDIM, standx="none", standy="none", divisor=divisor, V=V)
    s2 = fp.scca(BEDF, X, lambda1=L1, lambda2=L2, ndim=NDIM, standx="binom2", standy="none", divisor=divisor, V=V)
    assert s1["converged"] and s2["converged"]
    assert s1["U"].shape == (m, NDIM) and s1["V"].shape == (m, NDIM) and s1["Px"].shape == (n, NDIM) and s1["Py"].shape == (n, NDIM)
    expect_equal(ev, s1["d"], "d vs eigenvalues")
    expect_equal(s1["d"], s2["d"], "d matrix vs PLINK")
    expect_equal(np.ones(NDIM), diag_cor(s1["Px"], s1["Py"]), "cor matrix")
    expect_equal(np.ones(NDIM), diag_cor(s2["Px"], s2["Py"]), "cor PLINK")


@pytest.mark.parametrize("given_v", [False, True])
def test_scca_x_with_y(fp, data, given_v):  # test_scca.R:91-112, 157-180
    X, Y, rng = data
    l1, l2 = rng.uniform(1e-6, 1e-3, 2)
    V = rng.standard_normal((K, NDIM)) if given_v else None
    s1 = fp.scca(X, Y, lambda1=l1, lambda2=l2, ndim=NDIM, standx="none", standy="none", V=V)
    s2 = fp.scca(BEDF, Y, lambda1=l1, lambda2=l2, ndim=NDIM, standx="binom2", standy="none", V=V)
    expect_equal(s1["d"], s2["d"], "d")
    for j in (0, 1):
        expect_equal(s1["V"][:, j], s2["V"][:, j], "V[, %d]" % (j + 1))
        expect_equal(s1["U"][:, j], s2["U"][:, j], "U[, %d]" % (j + 1))
    expect_equal(diag_cor(s1["Px"], s1["Py"]), diag_cor(s2["Px"], s2["Py"]), "cor")


def test_scca_divisor(fp, data):  # test_scca.R:114-155
    X, Y, rng = data
    n = X.shape[0]
    l1, l2 = rng.uniform(1e-6, 1e-3, 2)
    kw = dict(lambda1=l1, lambda2=l2, ndim=NDIM, standy="none")
    s1 = fp.scca(X, Y, standx="none", **kw)
    s2 = fp.scca(BEDF, Y, standx="binom2", **kw)
    s3 = fp.scca(X, Y, standx="none", divisor="none", **kw)
    s4 = fp.scca(BEDF, Y, standx="binom2", divisor="none", **kw)
    for a, b in ((s1, s3), (s2, s4)):
        expect_equal(a["d"], b["d"] / (n - 1), "d")
        for j in (0, 1):
            expect_equal(a["V"][:, j], b["V"][:, j], "V[, %d]" % (j + 1))
            expect_equal(a["U"][:, j], b["U"][:, j], "U[, %d]" % (j + 1))
        expect_equal(diag_cor(a["Px"], a["Py"]), diag_cor(b["Px"], b["Py"]), "cor")


def test_scca_input_checking(fp, data):  # test_scca.R:182-198
    X, _, rng = data
    Z = rng.standard_normal((X.shape[0] + 3, 100))
    with pytest.raises(ValueError, match="The number of rows in X and Y don't match"):
        fp.scca(X, Z, lambda1=L1, lambda2=L2, ndim=NDIM, standx="none", standy="none")
    with pytest.raises(ValueError, match="fam and Y don't match"):
        fp.scca(BEDF, Z, lambda1=L1, lambda2=L2, ndim=NDIM, standx="binom2", standy="none")
    with pytest.raises(ValueError):
        fp.scca(X, Z, lambda1=L1, lambda2=-1, ndim=NDIM, standx="none", standy="none")
    with pytest.raises(ValueError):
        fp.scca(X, Z, lambda1=-1, lambda2=L2, ndim=NDIM, standx="none", standy="none")
    with pytest.raises(ValueError):
        fp.scca(BEDF, Z, lambda1=-1, lambda2=-1, ndim=NDIM, standx="binom2", standy="none")
