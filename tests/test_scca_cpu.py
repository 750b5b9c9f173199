"""SCCA without a GPU: the R-style input checks of flashpca_amd.scca() (flashpcaR/R/scca.R:106-222, raised as ValueError before any
device work), the two entry points in the header, the binding and the library, their refusals that need no device, and the CLI, whose
--scca still refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "flashpca_amd", "_build", "flashpca")
DATA = os.path.join(ROOT, "tests", "golden", "data_chr1")


def test_python_scca_input_checks(built_lib):
    import flashpca_amd as fp

    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, size=(50, 20)).astype(float)
    Y = rng.standard_normal((50, 3))
    kw = dict(standx="none", standy="none", ndim=2)
    cases = (
        (dict(X=X, Y=Y, standx="bogus"), "'arg' should be one of"),
        (dict(X=X, Y=Y, standy="bogus"), "'arg' should be one of"),
        (dict(X=X, Y=Y, divisor="p", **kw), "'arg' should be one of"),
        (dict(X=X, Y=[["a", "b"]] * 50, **kw), "Y must be a numeric matrix"),
        (dict(X={"x": 1}, Y=Y, **kw), "X must be a numeric matrix or a string naming a PLINK fileset"),
        (dict(X=X[:, :1], Y=Y, **kw), "X must have at least two columns"),
        (dict(X=X[:1], Y=Y[:1], **kw), "X must have at least two rows"),
        (dict(X=X, Y=rng.standard_normal((53, 3)), **kw), "The number of rows in X and Y don't match"),
        (dict(X=X + 0.5, Y=Y, standx="binom2", standy="none", ndim=2), "Your data contains values other than"),
        (dict(X=DATA, Y=Y, standx="sd", standy="none", ndim=2), "you must use standx='binom' or 'binom2'"),
        (dict(X=DATA, Y=Y, standx="binom2", standy="none", ndim=2), "The number of rows in .*data_chr1.fam and Y don't match"),
        (dict(X=X, Y=Y, lambda1=-1e-3, **kw), "lambda1 must be non-negative"),
        (dict(X=X, Y=Y, lambda1=[1e-3, -1.0], **kw), "lambda1 must be non-negative"),
        (dict(X=X, Y=Y, lambda1=None, **kw), "lambda1 must be non-negative"),
        (dict(X=X, Y=Y, lambda2=-1, **kw), "lambda2 must be non-negative"),
        (dict(X=X, Y=Y, lambda2=None, **kw), "lambda2 must be non-negative"),
        (dict(X=X, Y=Y, standx="none", standy="none", ndim=0), "ndim can't be less than 1"),
        (dict(X=X, Y=Y, standx="none", standy="none", ndim=4), "You asked for 4 dimensions, but only 3 allowed"),
        (dict(X=X, Y=Y, V=np.ones((3, 3)), **kw), r"dimensions of V must be \(ncol\(Y\) x \(ndim\)\)"),
        (dict(X=X, Y=Y, V=np.ones((2, 2)), **kw), r"dimensions of V must be"),
    )
    for args, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fp.scca(**args)
    n = fp.count_fam_rows(DATA + ".fam")
    with pytest.raises(ValueError, match="You asked for 11 dimensions, but only 10 allowed"):
        fp.scca(DATA, rng.standard_normal((n, 10)), standy="none", ndim=11)


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    header = open(os.path.join(ROOT, "include", "fpca.h")).read()
    for name in ("fpca_scca_prepare", "fpca_scca_fit"):
        assert re.search(r"^int %s\(fpca_ctx \*ctx," % name, header, re.M), name
        assert name in _lib.SIGNATURES
        assert getattr(fp.lib(), name) is not None
    assert "#define FPCA_ABI_VERSION 4" in header  # (no struct changed)
    for k, v in {0: "OK", 1: "MAXITER", 2: "LAMBDA1_TOO_LARGE", 3: "LAMBDA2_TOO_LARGE"}.items():
        assert "#define FPCA_SCCA_%s %d" % (v, k) in header and k in _lib.SCCA_STATUS
    # refusals that are decided before anything touches a device
    Y = np.zeros((4, 2), order="F")
    assert fp.lib().fpca_scca_prepare(None, Y.ctypes.data_as(C.c_void_p), 4, 2, 1, 1) == -1
    assert b"NULL" in fp.lib().fpca_last_error()
    st = C.c_int(0)
    assert fp.lib().fpca_scca_fit(None, 0.0, 0.0, 1, 10, 1e-4, None, 1, None, 0, None, 0, None, None, 0, None, 0, C.byref(st), None, None, None,
                                  C.byref(st)) == -1
    assert b"NULL context" in fp.lib().fpca_last_error()
    assert all(hasattr(fp.Context, m) for m in ("scca_prepare", "scca_fit")) and callable(fp.scca)


def test_the_limit_on_k_is_one_number_and_fits_the_lds(tmp_path):
    """SCCA_MAX_K is written in scca.hpp, include/fpca.h, INTEGRATION.md and DESIGN.md: one number.  What it costs k_scca_v<1024> in LDS
    -- the static part from the code object's metadata, 16 B per column of k_pad dynamic -- is the figure scca.hpp and the refusal's
    message carry (tests/test_gpu_scca_widths.py holds it against the device's per-workgroup limit and runs the fit at the maximum)."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    hpp = open(os.path.join(csrc, "scca.hpp")).read()
    max_k = int(re.search(r"constexpr int SCCA_MAX_K = (\d+);", hpp).group(1))
    assert max_k % 16 == 0
    assert "k > %d," % max_k in open(os.path.join(ROOT, "include", "fpca.h")).read()
    assert "k > %s," % format(max_k, ",") in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "1 ≤ k ≤ %s " % format(max_k, ",") in design
    out = str(tmp_path / "scca.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", os.path.join(csrc, "scca.hip"),
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    static = {}
    for block in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if "k_scca_v" in name:
            static[re.search(r"k_scca_vILi(\d+)E", name).group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    assert static == {"256": 8 * (256 + 4), "1024": 8 * (1024 + 16)}, static
    need = static["1024"] + 2 * 8 * max_k
    assert "SCCA_V_LDS_MAX = 8 * (1024 + 16) + 2 * 8 * SCCA_MAX_K;" in hpp and "%s B at the maximum" % format(need, ",") in hpp
    assert "%s B at the maximum" % format(need, ",") in design


def test_cli_scca_still_refuses(built_lib, tmp_path):
    """The library has SCCA, the command line does not yet: wiring flashpca --scca is a follow-up, the flag keeps its
    refusal and its --help line."""
    import flashpca_amd as fp

    assert callable(fp.scca) and "fpca_scca_fit" in open(os.path.join(ROOT, "include", "fpca.h")).read()
    fam = [l.split() for l in open(DATA + ".fam").read().splitlines()]
    with open(tmp_path / "ph.txt", "w") as f:
        for r in fam:
            f.write("%s %s 0.5 1.5\n" % (r[0], r[1]))
    for extra in (["--scca"], ["--scca", "--pheno", "ph.txt"], ["--scca", "--pheno", "ph.txt", "--lambda1", "0.01", "--lambda2", "0.01"]):
        r = subprocess.run([CLI, "--bfile", DATA, "--notime"] + extra, capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 1 and "outside the PCA path" in r.stderr, (extra, r.stderr)
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    line = [l for l in r.stderr.splitlines() if l.strip().startswith("--scca")]
    assert r.returncode == 0 and line
