"""fpca_scca_fit at the widths and heights the k-sized kernel (k_scca_v, csrc/scca.hip) treats differently, against the restatement
of tests/test_gpu_scca.py (reference_scca, run_ref, compare, check_projections, pack_codes: imported, not copied) at that module's
bounds, unchanged: 1e-12 on U and V, 1e-11 relative on d for equal iteration counts, and its one-apart branch -- which this module
allows ONE case over all of its own (its own list: a case here never spends the allowance of tests/test_gpu_scca.py).

k_scca_v deals the nb = ceil(P / 256) workgroup partials of C'u over ng = VT / cw thread groups, cw = min(k_pad, VT), VT = 256 for
k_pad <= 64 and 1024 above, four independent chains while 4 ng partials are left; k_pad > 1024 takes the columns in passes of 1024.
CASES names what each shape reaches.  Data: binomial dosages, MAF in [0.1, 0.5], 1 % missing calls, packed and loaded with
from_packed(accum="auto"); X is the oracle's dense(); Y = X B + 3 noise with 20 causal SNPs (all of them where P < 20); standy "sd",
divisor n - 1, Gaussian V0, tol 1e-9, maxiter 1000; penalties (1e-6, 1e-6) and (2e-2, 1e-3).  The seeds were chosen on the CPU so that
the restatement converges in every dimension of every case (it is asserted), and the two edge-rule cases come out of the restatement
as named.  The restatement on C = X'Y stops on the same iteration as the one as written in every case here and differs from it by at
most 4.3e-16 in U, 2.8e-15 in V, 3.9e-16 relative in d (iteration counts 1 to 618): the reference spends none of the one-apart
allowance.  Measured on the MI355X: every case stopped on the restatement's own iteration; worst max |dU| 1.3e-15, max |dV| 1.2e-15 (both
gs7, the eight-dimensional case), d 3.9e-16 relative.

The limit.  k_scca_v<1024> has 8,320 B of static LDS (the code object's metadata: buf 8 x 1024, red 8 x 16) and takes 16 k_pad
dynamic: 69,760 B at SCCA_MAX_K = 3840.  The MI355X reports 163,840 B of LDS per workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock),
so the documented maximum launches; test_the_documented_limit runs it and pins the refusal one above it with the number in its message.
Every case prints what it measured (pytest -s)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_scca as S  # noqa: E402

pytestmark = pytest.mark.gpu

LAMBDAS = ((1e-6, 1e-6), (2e-2, 1e-3))
TOL = 1e-9
MAX_K = 3840  # SCCA_MAX_K (csrc/scca.hpp), include/fpca.h, INTEGRATION.md, DESIGN.md 7b
LDS_STATIC_V1024 = 8320
ONE_APART = []  # this module's own

# (N, P, k, ndim, seed): what it reaches
CASES = {
    "kpad48_k33": (96, 300, 33, 4, 1),  # k_pad 48: ng = 5, threads 240-255 hold g == ng and idle
    "kpad48_k48": (96, 300, 48, 4, 2),
    "ng12_P255": (96, 255, 80, 3, 3),  # k_pad 80: ng = 12; one workgroup, one row short
    "ng9_P257": (96, 257, 112, 3, 4),  # k_pad 112: ng = 9; the second workgroup holds one row
    "P256": (96, 256, 20, 3, 5),  # P % 256 = 0
    "P5": (64, 5, 17, 2, 6),  # P < 16: most of every workgroup idle
    "P1": (64, 1, 3, 1, 7),  # u = +-1
    "nb19_kpad64": (96, 4859, 64, 3, 8),  # nb = 19 against 4 ng = 16: one unrolled round plus a tail of 3
    "nb67_kpad16": (64, 16897, 5, 2, 9),  # k_pad 16, nb = 67 > 4 ng = 64: the unrolled loop at ng = 16
    "k1024": (96, 300, 1024, 2, 10),  # ng = 1, one pass of 1024 columns
    "k1025": (96, 300, 1025, 2, 11),  # two passes, the second 16 wide with 15 pad columns
    "k2049": (96, 300, 2049, 2, 12),  # three passes
    "limit": (96, 300, MAX_K, 2, 13),  # the documented maximum
    "gs7": (200, 600, 40, 8, 14),  # Gram-Schmidt depth 7, G 8 x 8, pstride = 9
}
# the edge rules in a dimension j > 0, chosen on the CPU from the restatement alone: (case, lambda1, the dimension in which u vanishes)
# -- lambda1 from 0.18 to 0.1875 gives the same supports and the same stopping dimension, from 0.19 on u vanishes in dimension 1 --
# and (case, penalties): iters 94, 127, 330 without a limit, so maxiter = 110
VANISH = ("kpad48_k33", 0.184, 3)
MAXITER = ("nb19_kpad64", LAMBDAS[0])


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


_DATA = {}


def case_data(O, name):
    """packed, X (the oracle's dense()), Y, the standardised Y and V0 of a case; built once."""
    if name not in _DATA:
        N, P, k, ndim, seed = CASES[name]
        rng = np.random.default_rng(20261020 + seed)
        maf = rng.uniform(0.1, 0.5, P)
        u = rng.random((P, N))
        q, h = (maf * maf)[:, None], (maf * (2 - maf))[:, None]  # P(dosage = 2 of A1), P(dosage >= 1)
        codes = np.where(u < q, 0, np.where(u < h, 2, 3)).astype(np.uint8)  # hom A1, het, hom A2
        codes[rng.random((P, N)) < 0.01] = 1  # missing
        packed = S.pack_codes(codes)
        X = O.OracleData(packed=packed, N=N, P=P, stand="binom2").dense()
        assert np.all(X.std(axis=0) > 0)  # no monomorphic SNP
        nc = min(20, P)
        causal = rng.choice(P, nc, replace=False)
        Y = X[:, causal] @ rng.standard_normal((nc, k)) + 3 * rng.standard_normal((N, k))
        V0 = rng.standard_normal((k, ndim))
        Ys, _ = O.standardise(Y, "sd")
        _DATA[name] = dict(N=N, P=P, k=k, ndim=ndim, packed=packed, X=X, Y=Y, Ys=Ys, V0=V0)
    return _DATA[name]


def compare(got, ref, label):
    """tests/test_gpu_scca.py::compare with this module's one-apart list in place of that module's."""
    before = len(S.ONE_APART)
    try:
        S.compare(got, ref, TOL, label)
    finally:
        while len(S.ONE_APART) > before:
            ONE_APART.append(S.ONE_APART.pop())
    assert len(ONE_APART) <= 1, ONE_APART  # over the whole module


def fit_both(fp, O, name, check=None):
    d = case_data(O, name)
    with fp.Context.from_packed(d["packed"], d["N"], d["P"], accum="auto") as ctx:
        ctx.scca_prepare(d["Y"], standy="sd", divisor="n1")
        for l1, l2 in LAMBDAS:
            label = "%s N=%d P=%d k=%d ndim=%d %g %g" % (name, d["N"], d["P"], d["k"], d["ndim"], l1, l2)
            ref = S.run_ref(d["X"], d["Ys"], "n1", l1, l2, d["V0"], tol=TOL, maxiter=1000)
            assert ref["converged"] and ref["status"] == "ok", (label, ref["status"], ref["iters"])
            got = ctx.scca_fit(l1, l2, d["ndim"], d["V0"], tol=TOL, maxiter=1000)
            compare(got, ref, label)
            assert np.array_equal(got["nzero_x"], (got["U"] != 0).sum(axis=0)) and np.array_equal(got["nzero_y"], (got["V"] != 0).sum(axis=0))
            if check:
                check(got)


@pytest.mark.parametrize("name", [n for n in CASES if n != "limit"])
def test_width_classes(fp, O, name):
    def check(got):
        if name == "P1":
            assert np.all(np.abs(got["U"]) == 1.0)

    fit_both(fp, O, name, check)


def test_the_documented_limit(fp, O):
    """k = SCCA_MAX_K: the number in the message is the number that launches.  The LDS it needs is held against the device's
    per-workgroup limit (a property query) BEFORE the fit, so a limit that cannot launch fails here as arithmetic, not as a launch."""
    need = LDS_STATIC_V1024 + 2 * 8 * MAX_K  # (MAX_K is a multiple of 16: k_pad = k)
    max_k, lib_need, have = C.c_int(0), C.c_int(0), C.c_int(0)
    fp._lib.check(fp.lib().fpca_debug_scca_lds(0, C.byref(max_k), C.byref(lib_need), C.byref(have)))
    print("k = %d needs %d B of LDS in k_scca_v<1024>; the device gives a workgroup %d B" % (max_k.value, lib_need.value, have.value))
    assert max_k.value == MAX_K and lib_need.value == need and MAX_K % 16 == 0
    assert need <= have.value, (need, have.value)
    fit_both(fp, O, "limit")
    d = case_data(O, "limit")
    with fp.Context.from_packed(d["packed"], d["N"], d["P"], accum="auto") as ctx:
        Y1 = np.zeros((d["N"], MAX_K + 1))
        with pytest.raises(fp.FpcaError, match=r"%d phenotypes; at most %d are supported \(.*: %d B at the maximum" % (MAX_K + 1, MAX_K, need)) as e:
            ctx.scca_prepare(Y1)
        assert e.value.code == -1
        with pytest.raises(fp.FpcaError, match="no phenotypes prepared"):  # (the refused prepare left nothing behind)
            ctx.scca_fit(1e-6, 1e-6, 2, np.ones((MAX_K + 1, 2)))


def test_u_vanishes_in_a_later_dimension(fp, O):
    """lambda1 between the largest normalised entry of dimension 0 and that of dimension VANISH_J: dimension 0 .. VANISH_J - 1 are
    kept, column VANISH_J onwards is U = 0, V = V0, d = 0."""
    d = case_data(O, VANISH[0])
    l1, l2, jstop = VANISH[1], 1e-3, VANISH[2]
    ref = S.run_ref(d["X"], d["Ys"], "n1", l1, l2, d["V0"], tol=TOL, maxiter=1000)
    assert ref["status"] == "lambda1 too large" and not ref["converged"]
    assert jstop >= 1 and np.all(ref["d"][:jstop] != 0) and np.all(ref["d"][jstop:] == 0) and np.all(ref["U"][:, jstop:] == 0)
    assert np.all(np.abs(ref["U"][:, :jstop]).max(axis=0) > 0)
    with fp.Context.from_packed(d["packed"], d["N"], d["P"], accum="auto") as ctx:
        ctx.scca_prepare(d["Y"], standy="sd", divisor="n1")
        got = ctx.scca_fit(l1, l2, d["ndim"], d["V0"], tol=TOL, maxiter=1000)
    assert got["status"] == "lambda1 too large" and not got["converged"]
    assert np.all(got["U"][:, jstop:] == 0) and np.array_equal(got["V"][:, jstop:], d["V0"][:, jstop:]) and np.all(got["d"][jstop:] == 0)
    assert np.all(np.abs(np.linalg.norm(got["U"][:, :jstop], axis=0) - 1) < 1e-12) and np.all(got["d"][:jstop] != 0)
    compare(got, ref, "u vanishes in dimension %d" % jstop)


def test_maxiter_in_a_later_dimension(fp, O):
    """maxiter between iters[0] and iters[1] of the unlimited fit: dimension 0 converges, dimension 1 stops at maxiter and keeps its
    current u and v, d[1] = 0, nothing later is attempted."""
    d = case_data(O, MAXITER[0])
    l1, l2 = MAXITER[1]
    full = S.run_ref(d["X"], d["Ys"], "n1", l1, l2, d["V0"], tol=TOL, maxiter=1000)
    assert full["converged"] and full["iters"][0] + 2 <= full["iters"][1], full["iters"]
    maxiter = int(full["iters"][0] + full["iters"][1]) // 2
    ref = S.run_ref(d["X"], d["Ys"], "n1", l1, l2, d["V0"], tol=TOL, maxiter=maxiter)
    assert ref["status"] == "maxiter reached" and ref["iters"].tolist()[:2] == [full["iters"][0], maxiter] and ref["d"][0] != 0
    with fp.Context.from_packed(d["packed"], d["N"], d["P"], accum="auto") as ctx:
        ctx.scca_prepare(d["Y"], standy="sd", divisor="n1")
        got = ctx.scca_fit(l1, l2, d["ndim"], d["V0"], tol=TOL, maxiter=maxiter)
    assert got["status"] == "maxiter reached" and not got["converged"]
    assert got["iters"].tolist() == [int(full["iters"][0]), maxiter] + [0] * (d["ndim"] - 2)
    assert got["d"][0] != 0 and np.all(got["d"][1:] == 0)
    assert abs(np.linalg.norm(got["U"][:, 1]) - 1) < 1e-12 and abs(np.linalg.norm(got["V"][:, 1]) - 1) < 1e-12  # the current u, v stay
    assert np.all(got["U"][:, 2:] == 0) and np.array_equal(got["V"][:, 2:], d["V0"][:, 2:])
    compare(got, ref, "maxiter %d in dimension 1" % maxiter)

