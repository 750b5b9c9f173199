"""UCCA without a GPU: the F tail of fpca_ucca (fpca_debug_f_sf, the host build of the source the finishing kernel runs) against
scipy, the CLI's refusals of --ucca / --scca (all decided before any device work), and the R-style input checks of
flashpca_amd.ucca()."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy import special, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flashpca_amd", "_build", "flashpca")
DATA = os.path.join(ROOT, "tests", "golden", "data_chr1")


def f_sf(r2, n, k):
    import flashpca_amd as fp

    F, P = C.c_double(), C.c_double()
    rc = fp.lib().fpca_debug_f_sf(float(r2), int(n), int(k), C.byref(F), C.byref(P))
    assert rc == 0, fp.lib().fpca_last_error()
    return F.value, P.value


sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from f_tail_yardstick import KS, R2_GRID  # noqa: E402  (shared with tests/test_gpu_f_tail.py, which runs the device build on it)


@pytest.mark.parametrize("n", [10, 957, 500000, 1000000])
def test_f_tail_matches_scipy(built_lib, n):
    """P = I_{1 - r2}((n - k - 1) / 2, k / 2) to 1e-8 relative wherever P >= 1e-290 (exact in r2: betaincc(k/2, (n-k-1)/2, r2)),
    and scipy.stats.f.sf at the F the library returns to 1e-6; F to 1e-14."""
    checked = 0
    for k in (1, 2, 10, 15, 63, 256):
        if k > n - 2:
            continue
        a, b = (n - k - 1) / 2.0, k / 2.0
        for r2 in R2_GRID:
            F, P = f_sf(r2, n, k)
            Fe = r2 / (1 - r2) * (n - k - 1) / k
            assert abs(F - Fe) <= 1e-14 * Fe, (n, k, r2, F, Fe)
            Pe = special.betaincc(b, a, r2)
            if Pe >= 1e-290:
                assert abs(P - Pe) <= 1e-8 * Pe, (n, k, r2, P, Pe)
                # (f.sf starts from F and forms 1 - x = k F / (n - k - 1 + k F) itself: at tiny r2 and large n that costs it digits)
                Ps = stats.f.sf(F, k, n - k - 1)
                assert abs(P - Ps) <= 1e-6 * Ps, (n, k, r2, P, Ps)
                checked += 1
            else:
                assert 0.0 <= P < 1e-280, (n, k, r2, P, Pe)
    assert checked > 300


def test_f_tail_matches_scipy_at_one_residual_degree(built_lib):
    """n = k + 2, the smallest n f_sf accepts (F(k, 1): a = 1/2), on the same grid at the same bounds."""
    checked = 0
    for k in KS:
        n = k + 2
        for r2 in R2_GRID:
            F, P = f_sf(r2, n, k)
            Fe = r2 / (1 - r2) * (n - k - 1) / k
            assert abs(F - Fe) <= 1e-14 * Fe, (n, k, r2, F, Fe)
            Pe = special.betaincc(k / 2.0, 0.5, r2)
            if Pe >= 1e-290:
                assert abs(P - Pe) <= 1e-8 * Pe, (n, k, r2, P, Pe)
                checked += 1
            else:
                assert 0.0 <= P < 1e-280, (n, k, r2, P, Pe)
    assert checked > 300


def test_f_tail_edges(built_lib):
    import flashpca_amd as fp

    for n, k in ((10, 1), (957, 15), (1000000, 256)):
        assert f_sf(0.0, n, k) == (0.0, 1.0)
        F, P = f_sf(1.0, n, k)
        assert F == np.inf and P == 0.0
        F, P = f_sf(1.5, n, k)
        assert F == np.inf and P == 0.0
        F, P = f_sf(np.nan, n, k)
        assert np.isnan(F) and np.isnan(P)
    F, P = C.c_double(), C.c_double()
    assert fp.lib().fpca_debug_f_sf(0.5, 10, 9, C.byref(F), C.byref(P)) == -1  # k = n - 1
    assert fp.lib().fpca_debug_f_sf(0.5, 10, 0, C.byref(F), C.byref(P)) == -1


def run(args, cwd=None):
    return subprocess.run([CLI] + args, capture_output=True, text=True, cwd=cwd)


def write_pheno(path, rows, k, bad=None):
    fam = [l.split() for l in open(DATA + ".fam").read().splitlines()]
    rng = np.random.default_rng(1)
    with open(path, "w") as f:
        for i in range(rows):
            vals = ["%.6f" % v for v in rng.standard_normal(k)]
            if bad is not None and i == bad:
                vals[0] = "x1"
            f.write("%s %s %s\n" % (fam[i][0], fam[i][1], " ".join(vals)))
    return str(path)


def test_cli_ucca_refusals(built_lib, tmp_path):
    """Every refusal exits 1 with its message, before a context exists (so on a machine without a GPU too)."""
    n = len(open(DATA + ".fam").read().splitlines())
    good = write_pheno(tmp_path / "ph.txt", n, 3)
    cases = (
        (["--ucca"], "you must specify a phenotype file in CCA/UCCA/SCCA mode using --pheno"),
        (["--ucca", "--pheno", write_pheno(tmp_path / "short.txt", n - 1, 3)], "has %d rows, but" % (n - 1)),
        (["--ucca", "--pheno", write_pheno(tmp_path / "wide.txt", n, n - 1)], "UCCA needs between 1 and N - 2"),
        (["--ucca", "--pheno", write_pheno(tmp_path / "bad.txt", n, 2, bad=4)], "line 5: 'x1' cannot be parsed as a number"),
        (["--ucca", "--pheno", good, "--standy", "bogus"], "unknown standardization method (--standy): bogus"),
        (["--ucca", "--pheno", good, "--gpus", "2"], "--gpus applies to PCA only"),
        (["--ucca", "--check"], "conflicting modes requested"),
        (["--ucca", "--scca", "--pheno", good], "conflicting modes requested"),
        (["--scca"], "outside the PCA path"),
        (["--scca", "--pheno", good], "outside the PCA path"),
    )
    for extra, msg in cases:
        r = run(["--bfile", DATA, "--notime"] + extra, cwd=tmp_path)
        assert r.returncode == 1, (extra, r.stdout, r.stderr)
        assert msg in r.stderr, (extra, r.stderr)
    assert not os.path.exists(tmp_path / "ucca.txt")
    # PCA mode keeps ignoring --standy and --pheno: the run gets past the whole command line and the .fam / .bim to the check of
    # --ndim against the file sizes (which needs no device)
    r = run(["--bfile", DATA, "--notime", "--standy", "bogus", "--pheno", "/nonexistent", "--ndim", "5000"])
    assert r.returncode == 1 and "You asked for 5000 dimensions" in r.stderr, r.stderr
    assert "standy" not in r.stderr and "pheno" not in r.stderr


def test_cli_help_describes_ucca(built_lib):
    r = run(["--help"])
    assert r.returncode == 0
    line = [l for l in r.stderr.splitlines() if l.strip().startswith("--ucca")]
    assert line and "not supported" not in line[0]


def test_python_ucca_input_checks(built_lib):
    """flashpcaR/R/ucca.R's stop() checks, raised before any device work."""
    import flashpca_amd as fp

    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, size=(50, 20)).astype(float)
    Y = rng.standard_normal((50, 3))
    with pytest.raises(ValueError, match="'arg' should be one of"):
        fp.ucca(X, Y, standx="bogus")
    with pytest.raises(ValueError, match="'arg' should be one of"):
        fp.ucca(X, Y, standy="bogus")
    with pytest.raises(ValueError, match="Y must be a numeric matrix"):
        fp.ucca(X, [["a", "b"]] * 50)
    with pytest.raises(ValueError, match="X must be a numeric matrix or a string naming a PLINK fileset"):
        fp.ucca({"x": 1}, Y, standy="none")
    with pytest.raises(ValueError, match="The number of rows in X and Y don't match"):
        fp.ucca(X, rng.standard_normal((53, 3)), standx="none", standy="none")
    with pytest.raises(ValueError, match="cannot have more columns than the sample size"):
        fp.ucca(X, rng.standard_normal((50, 53)), standx="none", standy="none")
    with pytest.raises(ValueError, match="Your X matrix contains values other than"):
        fp.ucca(X + 0.5, Y, standx="binom", standy="none")
    with pytest.raises(ValueError, match="Your Y matrix contains values other than"):
        fp.ucca(X, Y, standx="binom2", standy="binom2")
    with pytest.raises(ValueError, match="you must use standx='binom' or 'binom2'"):
        fp.ucca(DATA, Y, standx="sd", standy="none")
    n = fp.count_fam_rows(DATA + ".fam")
    with pytest.raises(ValueError, match="The number of rows in .*data_chr1.fam and Y don't match"):
        fp.ucca(DATA, rng.standard_normal((n + 3, 10)), standx="binom2", standy="none")
    with pytest.raises(ValueError, match="cannot have more columns than the sample size"):
        fp.ucca(DATA, rng.standard_normal((n, n + 3)), standx="binom2", standy="none")
