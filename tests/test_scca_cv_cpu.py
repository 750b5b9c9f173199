"""Cross-validated SCCA without a GPU: the two entry points in the headers, the binding and both builds of the library; their refusals
that need no device; the R-style input checks of flashpca_amd.cv_scca() (flashpcaR/R/scca.R:415-442 and the scca() checks that apply,
raised as ValueError before any device work); the host-side packing of a numeric genotype matrix; and the register discipline of the
new kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data_chr1")


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert re.search(r"^int fpca_scca_cv\(fpca_ctx \*ctx,", main, re.M) and "int fpca_scca_cv(" not in dbg
    assert re.search(r"^int fpca_debug_fold_stats\(fpca_ctx \*ctx,", dbg, re.M) and "fpca_debug_fold_stats" not in main  # (the drop-in header carries no lab bench)
    assert "#define FPCA_ABI_VERSION 4" in main and '#define FPCA_VERSION "0.3.0"' in main  # (no struct changed)
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in ("fpca_scca_cv", "fpca_debug_fold_stats"):
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    # refusals that are decided before anything touches a device
    L = fp.lib()
    Y = np.zeros((4, 2), order="F")
    fold = np.zeros(4, dtype=np.uint8)
    lam = np.array([1e-3])
    V0 = np.ones((2, 1), order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.fpca_scca_cv(None, p(Y), 4, 2, p(fold), 2, p(lam), 1, p(lam), 1, 1, 1, 1, 10, 1e-4, p(V0), 2, 0, 1e-12, 1, *[None] * 11)
    assert rc == -1 and b"NULL context" in L.fpca_last_error()
    assert L.fpca_debug_fold_stats(None, p(fold), 2, None, 0, None) == -1 and b"NULL" in L.fpca_last_error()
    assert all(hasattr(fp.Context, m) for m in ("scca_cv", "fold_stats")) and callable(fp.cv_scca)


def test_python_cv_scca_input_checks(built_lib):
    import flashpca_amd as fp

    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, size=(50, 20)).astype(float)
    Y = rng.standard_normal((50, 3))
    kw = dict(standy="none", ndim=2, nfolds=5)
    ok_folds = np.arange(50) % 5 + 1
    cases = (
        (dict(X=X, Y=Y, standy="none", ndim=2, nfolds=51), "nfolds is too large for the number of samples"),
        (dict(X=X, Y=Y, opt_dim=0, **kw), "opt.dim must be between 1 and ndim"),
        (dict(X=X, Y=Y, opt_dim=3, **kw), "opt.dim must be between 1 and ndim"),
        (dict(X=X, Y=Y, init="yes", **kw), "init muct be TRUE or FALSE"),
        (dict(X=X, Y=Y, init=1, **kw), "init muct be TRUE or FALSE"),
        (dict(X=X, Y=Y, folds=ok_folds[:49], **kw), "'folds' must be of same number of rows as X and Y"),
        (dict(X=X, Y=Y, folds=np.where(ok_folds == 3, 7, ok_folds), **kw), "'folds' must be a set of contiguous integers from 1 to nfolds"),
        (dict(X=X, Y=Y, folds=ok_folds - 1, **kw), "'folds' must be a set of contiguous integers from 1 to nfolds"),
        (dict(X=X, Y=Y, standx="bogus", **kw), "'arg' should be one of"),
        (dict(X=X, Y=Y, standy="bogus", ndim=2), "'arg' should be one of"),
        (dict(X=X, Y=Y, divisor="p", **kw), "'arg' should be one of"),
        (dict(X=X, Y=[["a", "b"]] * 50, **kw), "Y must be a numeric matrix"),
        (dict(X={"x": 1}, Y=Y, **kw), "X must be a numeric matrix or a string naming a PLINK fileset"),
        (dict(X=X[:, :1], Y=Y, **kw), "X must have at least two columns"),
        (dict(X=X, Y=rng.standard_normal((53, 3)), **kw), "The number of rows in X and Y don't match"),
        (dict(X=X + 0.5, Y=Y, **kw), "re-standardises the genotypes on every fold's training samples and needs genotype input"),
        (dict(X=X, Y=Y, standx="sd", **kw), "re-standardises the genotypes on every fold's training samples and needs genotype input"),
        (dict(X=DATA, Y=Y, standx="center", **kw), "needs genotype input"),
        (dict(X=DATA, Y=Y, **kw), "The number of rows in .*data_chr1.fam and Y don't match"),
        (dict(X=X, Y=Y, standy="binom2", ndim=2, nfolds=5), "standy='binom'/'binom2' can't be used here"),
        (dict(X=X, Y=Y, lambda1=[1e-3, -1.0], **kw), "lambda1 must be non-negative"),
        (dict(X=X, Y=Y, lambda1=None, **kw), "lambda1 must be non-negative"),
        (dict(X=X, Y=Y, lambda1=[np.nan], **kw), "lambda1 must be non-negative"),
        (dict(X=X, Y=Y, lambda2=-1, **kw), "lambda2 must be non-negative"),
        (dict(X=X, Y=Y, standy="none", ndim=0, opt_dim=0), "opt.dim must be between 1 and ndim"),
        (dict(X=X, Y=Y, standy="none", ndim=4, nfolds=5), "You asked for 4 dimensions, but only 3 allowed"),
        (dict(X=X, Y=Y, standy="none", ndim=2, nfolds=1), "between 2 and 64 folds"),
        (dict(X=X[:, :12], Y=rng.standard_normal((50, 45)), standy="none", ndim=11, nfolds=2, folds=np.r_[np.ones(40), 2 * np.ones(10)]),
         "You asked for 11 dimensions, but only 10 allowed"),  # the smallest training set has 10 samples
    )
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for args, msg in cases:
            with pytest.raises(ValueError, match=msg):
                fp.cv_scca(**args)
    with pytest.warns(UserWarning, match="'folds' will override 'nfolds' parameter"):
        with pytest.raises(ValueError, match="only 3 allowed"):
            fp.cv_scca(X, Y, folds=ok_folds, standy="none", ndim=4)
    # R's defaults
    import inspect

    d = {k: v.default for k, v in inspect.signature(fp.cv_scca).parameters.items()}
    assert np.array_equal(d["lambda1"], np.linspace(1e-6, 1e-3, 5)) and np.array_equal(d["lambda2"], np.linspace(1e-6, 1e-3, 5))
    assert (d["ndim"], d["nfolds"], d["folds"], d["opt_dim"], d["init"], d["standx"], d["standy"], d["divisor"], d["maxiter"], d["tol"]) == (
        3, 10, None, 1, True, "binom2", "binom2", "n1", 1000, 1e-4)


def test_numeric_genotypes_are_packed_like_plink(built_lib):
    """pack_dosages: dosage 0 / 1 / 2 / NaN -> codes 3 / 2 / 0 / 1, four samples to a byte, low bits first; the oracle reads it back."""
    import flashpca_amd as fp
    from oracle import oracle as O

    rng = np.random.default_rng(1)
    for n in (5, 8, 11):
        X = rng.integers(0, 3, size=(n, 7)).astype(float)
        X[rng.random((n, 7)) < 0.15] = np.nan
        pk = fp.api.pack_dosages(X)
        assert pk.shape == (7, (n + 3) // 4) and pk.dtype == np.uint8
        codes = np.stack([(pk >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(7, -1)
        assert np.all(codes[:, n:] == 0)
        back = np.select([codes[:, :n] == 3, codes[:, :n] == 2, codes[:, :n] == 0], [0.0, 1.0, 2.0], np.nan).T
        assert np.array_equal(back, X, equal_nan=True)
        Xs, _ = O.standardise(X, "binom2")
        with np.errstate(invalid="ignore"):
            D = O.OracleData(packed=pk, N=n, P=7, stand="binom2").dense()
        ok = np.isfinite(Xs).all(axis=0) & (np.nanstd(X, axis=0) > 0)
        assert np.allclose(D[:, ok], Xs[:, ok], atol=1e-12)


def test_cv_kernels_do_not_spill():
    """The pattern of test_gemm_kernels_do_not_spill: no kernel of scca_cv.hip (k_fold_counts keeps 24 counters per thread) may
    compile with VGPR spills."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "scca_cv.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                               os.path.join(csrc, "scca_cv.hip"), "-o", out], stderr=subprocess.DEVNULL)
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    spills = re.findall(r"\.vgpr_spill_count:\s+(\d+)", txt)
    assert len(names) == len(spills) and names
    for k in ("k_fold_counts", "k_fold_meansd", "k_cv_corr", "k_cv_gather_x"):
        assert any(k in n for n in names), k
    assert all(int(s) == 0 for s in spills), [(n, s) for n, s in zip(names, spills) if int(s)]
