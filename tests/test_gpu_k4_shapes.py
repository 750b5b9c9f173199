"""Small-shape parity of the eigensolver's K4 helpers (kernels.hip: k_gram / k_gram_tiled, k_block_gemm / k_block_gemm_lds with and
without the fused Gram, k_update_gram16, k_reduce_sum / k_reduce_tall) through the backend object the solver drives (fpca_debug_k4,
fpca_debug_k4_fused, fpca_debug_k4_inplace).

Main body: EXACT data.  V and W are integers in [-4, 4], the coefficients integers in [-3, 3], all stored as fp64.  Every product
and every partial sum is then an integer far below 2^53 (asserted on the host for every case), so any summation order -- MFMA tree,
LDS fold, split-K plane reduction -- must give exactly the int64 result: np.array_equal, no tolerance.  One dropped or duplicated
row, one plane a workgroup did not leave, one stale LDS stage changes an integer.

Second layer: a handful of the same shapes with standard-normal data against np.longdouble and the standard forward bound of a sum
of n products, so that the integer data cannot hide a precision loss (an fp32 temporary is exact on small integers).

Heights: a block has N_pad = 4 * round_up(ceil(N / 4), 128) rows (a multiple of 512); the expected N_pad is part of each case's id.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53  # unit roundoff of fp64


def n_pad(N):
    return 4 * (-(-(-(-N // 4)) // 128) * 128)


def _id(N, b, nq):
    return "N%d-pad%d-b%d-nq%d" % (N, n_pad(N), b, nq)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a):
    """int64 -> the fp64 column-major array the hooks read (exact: |a| < 2^53 is asserted by the callers)"""
    return np.asfortranarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------
# data and references (host only)
def int_case(N, b, nq, edge=None):
    """V (N x nq b), W (N x b), C (nq, b, b) as int64.  edge = 'last': V and W are zero except row N - 1; 'ends': except rows 0 and
    N - 1."""
    rng = np.random.default_rng([N, b, nq])
    V = rng.integers(-4, 5, size=(N, nq * b), dtype=np.int64)
    W = rng.integers(-4, 5, size=(N, b), dtype=np.int64)
    Cin = rng.integers(-3, 4, size=(nq, b, b), dtype=np.int64)
    if edge is not None:
        keep = np.zeros(N, dtype=bool)
        keep[N - 1] = True
        if edge == "ends":
            keep[0] = True
        V[~keep] = 0
        W[~keep] = 0
        # a kept row must not vanish by chance: no zero in it
        V[keep] = np.where(V[keep] == 0, 3, V[keep])
        W[keep] = np.where(W[keep] == 0, -2, W[keep])
    return V, W, Cin


def int_refs(V, W, Cin, want):
    """the quantities in `want` that the hooks return, in int64 (int64 products are slow on the host: only what the case compares),
    with the check that makes 'exact' true: all of them below 2^53"""
    nq, b = Cin.shape[0], Cin.shape[1]
    VC = V @ Cin.reshape(nq * b, b)
    upd = VC + W
    r = {"out0": VC, "out1": upd}  # gemm without Init / with Init = W
    if "gram" in want:
        r["gram"] = (V.T @ W).reshape(nq, b, b)  # C_gram
    if "g0" in want:
        r["g0"] = VC.T @ VC  # Out' Out
    if "g1" in want or "cg" in want:
        r["g1"] = upd.T @ upd
    if "cg" in want:
        r["cg"] = np.concatenate([(V.T @ upd).reshape(nq, b, b), r["g1"][None]], axis=0)  # fused: V_q' Out, then Out' Out
    r["max"] = max(int(np.max(np.abs(x))) for x in r.values())
    assert r["max"] < 2 ** 53, r["max"]
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# the hooks
def k4(fp, ctx, b, nq, V, W, Cin=None, use_init=0, want_gram=False, want_out=False, want_g=False):
    N = V.shape[0]
    Cg = np.full((nq, b, b), np.nan) if want_gram else None
    Out = np.full((N, b), np.nan, order="F") if want_out else None
    G = np.full((b, b), np.nan) if want_g else None
    fp._lib.check(fp.lib().fpca_debug_k4(ctx.h, b, nq, _ptr(V), _ptr(W), _ptr(Cg), _ptr(Cin), use_init, _ptr(Out), _ptr(G)))
    return Cg, Out, G


def k4_fused(fp, ctx, b, nq, V, W, Cin):
    Out = np.full((V.shape[0], b), np.nan, order="F")
    Cg = np.full((nq + 1, b, b), np.nan)
    fp._lib.check(fp.lib().fpca_debug_k4_fused(ctx.h, b, nq, _ptr(V), _ptr(W), _ptr(Cin), _ptr(Out), _ptr(Cg)))
    return Out, Cg


def k4_inplace(fp, ctx, b, nq, V, W, Cin, mode):
    Out = np.full((V.shape[0], b), np.nan, order="F")
    G = np.full((b, b), np.nan) if mode == 2 else None
    fp._lib.check(fp.lib().fpca_debug_k4_inplace(ctx.h, b, nq, _ptr(V), _ptr(W), _ptr(Cin), mode, _ptr(Out), _ptr(G)))
    return Out, G


def _same(got, ref, what):
    """bit-exact against the int64 reference; the message names the output and where it first differs"""
    want = ref.astype(np.float64)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d entries differ, first at %s: got %r, want %r" % (
            what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def check_exact(fp, N, b, nq, calls, edge=None):
    """calls: any of 'gram', 'gemm' (with and without Init), 'gemm_gram' (the fused update + Gram of its output, with and without
    Init), 'fused' (fpca_debug_k4_fused)"""
    Vi, Wi, Ci = int_case(N, b, nq, edge)
    ref = int_refs(Vi, Wi, Ci, [w for c in calls for w in WANT[c]])
    V, W, Cin = _f(Vi), _f(Wi), np.ascontiguousarray(Ci, dtype=np.float64)
    with fp.Context.synthetic(N, 256, n_pop=4, accum="fp64") as ctx:
        # Twice: the hooks fill the context's partial planes and the output block with NaNs before they run, at the size earlier
        # calls left them -- in the second round every plane and every row tile that a kernel does not write is a NaN in the
        # result, not a lucky zero of fresh memory (the planes of workgroups that own no row tile are summed like all others).
        for rnd in ("first call", "second call"):
            if "gram" in calls:
                Cg, _, _ = k4(fp, ctx, b, nq, V, W, want_gram=True)
                _same(Cg, ref["gram"], "%s, gram: C_gram" % rnd)
            for init in (0, 1):
                if "gemm" in calls:
                    _, Out, _ = k4(fp, ctx, b, nq, V, W, Cin, init, want_out=True)
                    _same(Out, ref["out%d" % init], "%s, gemm (Init %d): Out" % (rnd, init))
                if "gemm_gram" in calls:
                    _, Out, G = k4(fp, ctx, b, nq, V, W, Cin, init, want_out=True, want_g=True)
                    _same(Out, ref["out%d" % init], "%s, gemm_gram (Init %d): Out" % (rnd, init))
                    _same(G, ref["g%d" % init], "%s, gemm_gram (Init %d): G_out" % (rnd, init))
            if "fused" in calls:
                Out, Cg = k4_fused(fp, ctx, b, nq, V, W, Cin)
                _same(Out, ref["out1"], "%s, fused: Out" % rnd)
                for q in range(nq + 1):
                    _same(Cg[q], ref["cg"][q], "%s, fused: Cg[%d]%s" % (rnd, q, " (Out'Out)" if q == nq else ""))


WANT = {"gram": ("gram",), "gemm": (), "gemm_gram": ("g0", "g1"), "fused": ("cg",)}  # the references of each kind of call
ALL = ("gram", "gemm", "gemm_gram", "fused")
K4 = ("gram", "gemm", "gemm_gram")

# Heights at 16 columns: one 512-row block (N = 1, 17, 511, 512), two (513), the last height below the fused update's threshold
# (N_pad 7680), exactly one row tile per workgroup of its 512 (N_pad 8192), two tiles for some and none for 240 of them (N_pad
# 8704), three tiles (N = 16897: N_pad 17408, 1088 tiles) -- and with them the steps of the gram_rows / gram_splits ladder and
# both plane reductions (8 planes of k_reduce_sum at N_pad 512, >= 64 planes of k_reduce_tall from N_pad 4096 on).
HEIGHTS = [(N, 16, nq) for N in (1, 17, 511, 512, 513, 7680, 7681, 8192, 8193, 16897) for nq in (1, 5)]
HEIGHTS += [(N, b, nq) for b in (32, 48, 64) for N in (1, 513, 8193) for nq in (1, 5)]


@pytest.mark.parametrize("N,b,nq", HEIGHTS, ids=[_id(*c) for c in HEIGHTS])
def test_k4_exact_over_heights(built_lib, N, b, nq):
    import flashpca_amd as fp

    check_exact(fp, N, b, nq, ALL)


# k_block_gemm_lds stages the coefficient blocks through LDS 12 (16 columns) or 3 (32 columns) at a time: a full stage, a full one
# followed by a partial one (13, 25; 4, 5, 7), two full ones (24).  k_gram_tiled shares one W tile among 8 (16 columns) or 2 (32
# columns) basis blocks: 7, 8, 9 blocks / 2, 3.  48 and 64 columns: k_gram<3 / 4>, k_block_gemm<3 / 4>, no fused Gram.
STAGES = [(1537, 16, nq) for nq in (7, 8, 9, 11, 12, 13, 24, 25)]
STAGES += [(1537, 32, nq) for nq in (2, 3, 4, 5, 7)]
STAGES += [(1537, b, nq) for b in (48, 64) for nq in (1, 2, 5)]


@pytest.mark.parametrize("N,b,nq", STAGES, ids=[_id(*c) for c in STAGES])
def test_k4_exact_over_lds_stages_and_gram_groups(built_lib, N, b, nq):
    import flashpca_amd as fp

    check_exact(fp, N, b, nq, K4)


# k_update_gram16<4> serves nq <= 16, <7> nq <= 28; the wave nq & 3 takes Out'Out in accumulator nq >> 2 (16: the last shape of <4>,
# Out'Out in G[QW]; 17: the first of <7>; 28: the cap, G[QW] again).  29 blocks, 32 columns and N_pad 7680 take the two launches.
FUSED = [(N, 16, nq) for N in (8193, 7681) for nq in (1, 2, 3, 4, 5, 15, 16, 17, 27, 28)]
FUSED += [(8193, 16, 29), (8193, 32, 3), (7680, 16, 5)]


@pytest.mark.parametrize("N,b,nq", FUSED, ids=[_id(*c) for c in FUSED])
def test_k4_exact_fused_update_and_gram(built_lib, N, b, nq):
    import flashpca_amd as fp

    check_exact(fp, N, b, nq, ("fused",))


# Which end broke when a random case fails: everything zero except the last row (the only row of the last, mostly padded, tile), or
# except the first and the last.
EDGES = [(N, b, nq, e) for N in (513, 8193) for b, nq in ((16, 5), (48, 2)) for e in ("last", "ends")]


@pytest.mark.parametrize("N,b,nq,edge", EDGES, ids=["%s-%s" % (_id(*c[:3]), c[3]) for c in EDGES])
def test_k4_exact_edge_rows(built_lib, N, b, nq, edge):
    import flashpca_amd as fp

    check_exact(fp, N, b, nq, ALL, edge)


# The solver's in-place forms (solver.cpp): gemm(V, m, negC, w, w) -- Out aliases Init; gemm(&w, 1, M, -1, w) and the Ritz rotation
# -- Out aliases the last operand block; gemm_gram(VW, M + 1, negC, -1, W) -- the same with the Gram matrix of what was written.
INPLACE = [(N, b, nq) for N in (513, 8193) for b, nq in ((16, 1), (16, 12), (16, 13), (32, 1), (32, 3), (32, 4), (48, 2), (64, 2))]


@pytest.mark.parametrize("N,b,nq", INPLACE, ids=[_id(*c) for c in INPLACE])
def test_k4_exact_in_place(built_lib, N, b, nq):
    import flashpca_amd as fp

    Vi, Wi, Ci = int_case(N, b, nq)
    ref = int_refs(Vi, Wi, Ci, ("g0",))
    V, W, Cin = _f(Vi), _f(Wi), np.ascontiguousarray(Ci, dtype=np.float64)
    with fp.Context.synthetic(N, 256, n_pop=4, accum="fp64") as ctx:
        for rnd in ("first call", "second call"):  # (as in check_exact: the second on NaN-filled partial planes)
            Out, _ = k4_inplace(fp, ctx, b, nq, V, W, Cin, 0)
            _same(Out, ref["out1"], "%s, mode 0 (out = init): Out" % rnd)
            Out, _ = k4_inplace(fp, ctx, b, nq, V, W, Cin, 1)
            _same(Out, ref["out0"], "%s, mode 1 (out = last operand): Out" % rnd)
            Out, G = k4_inplace(fp, ctx, b, nq, V, W, Cin, 2)
            _same(Out, ref["out0"], "%s, mode 2 (gemm_gram, out = last operand): Out" % rnd)
            _same(G, ref["g0"], "%s, mode 2 (gemm_gram, out = last operand): G_out" % rnd)


# ---------------------------------------------------------------------------------------------------------------------------
# Rounded data.  A sum of n products computed in fp64 in ANY order (fused multiply-adds included) differs from the exact sum by at
# most gamma_n sum |a_i| |b_i|, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).
# The bound used is 2 (n + 4) u |A|'|B| elementwise: once for the kernel, once more for a host whose longdouble is a plain double,
# the + 4 over the 1 / (1 - n u) factor and the final roundings.  n = N for the Gram outputs, nq b + 1 for the update (Init counts
# as one more term).  The Gram outputs that involve Out are judged against the DOWNLOADED Out: the kernels form them from exactly
# the values they store.
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def _within(got, ref_ld, absprod_ld, n, what):
    err = np.abs(_ld(got) - ref_ld)
    bound = 2.0 * (n + 4) * U * absprod_ld
    worst = float(np.max(err - bound))
    print("%s: max error %.3e, smallest bound %.3e" % (what, float(np.max(err)), float(np.min(bound))))
    assert worst <= 0.0, "%s: error exceeds 2 (n + 4) u |A|'|B| by %.3e (n = %d)" % (what, worst, n)


def normal_case(N, b, nq):
    rng = np.random.default_rng([N, b, nq, 1])
    V = np.asfortranarray(rng.standard_normal((N, nq * b)))
    W = np.asfortranarray(rng.standard_normal((N, b)))
    Cin = rng.standard_normal((nq, b, b))
    return V, W, Cin


ROUNDED_K4 = [(8193, 16, 13), (8193, 32, 4), (513, 48, 2), (513, 64, 2)]


@pytest.mark.parametrize("N,b,nq", ROUNDED_K4, ids=[_id(*c) for c in ROUNDED_K4])
def test_k4_rounded_within_the_forward_bound(built_lib, N, b, nq):
    """gram, gemm and the fused gemm + Gram on standard-normal data against np.longdouble; every call twice: the plane reductions are
    deterministic, so the two results are bit-identical."""
    import flashpca_amd as fp

    V, W, Cin = normal_case(N, b, nq)
    Vl, Wl, Cl = _ld(V), _ld(W), _ld(Cin.reshape(nq * b, b))
    nu = nq * b + 1
    with fp.Context.synthetic(N, 256, n_pop=4, accum="fp64") as ctx:
        Cg, _, _ = k4(fp, ctx, b, nq, V, W, want_gram=True)
        Cg2, _, _ = k4(fp, ctx, b, nq, V, W, want_gram=True)
        assert np.array_equal(Cg, Cg2), "gram is not deterministic"
        _within(Cg.reshape(nq * b, b), Vl.T @ Wl, np.abs(Vl).T @ np.abs(Wl), N, "gram: C_gram")
        for init in (0, 1):
            ref = Vl @ Cl + (Wl if init else 0)
            absprod = np.abs(Vl) @ np.abs(Cl) + (np.abs(Wl) if init else 0)
            _, Out, _ = k4(fp, ctx, b, nq, V, W, Cin, init, want_out=True)
            _, Out2, _ = k4(fp, ctx, b, nq, V, W, Cin, init, want_out=True)
            assert np.array_equal(Out, Out2), "gemm is not deterministic"
            _within(Out, ref, absprod, nu, "gemm (Init %d): Out" % init)
            _, Outg, G = k4(fp, ctx, b, nq, V, W, Cin, init, want_out=True, want_g=True)
            _, Outg2, G2 = k4(fp, ctx, b, nq, V, W, Cin, init, want_out=True, want_g=True)
            assert np.array_equal(Outg, Outg2) and np.array_equal(G, G2), "gemm_gram is not deterministic"
            _within(Outg, ref, absprod, nu, "gemm_gram (Init %d): Out" % init)
            Ol = _ld(Outg)
            _within(G, Ol.T @ Ol, np.abs(Ol).T @ np.abs(Ol), N, "gemm_gram (Init %d): G_out" % init)


ROUNDED_FUSED = [(8193, 16, 28), (7681, 16, 5), (8193, 32, 3)]


@pytest.mark.parametrize("N,b,nq", ROUNDED_FUSED, ids=[_id(*c) for c in ROUNDED_FUSED])
def test_k4_fused_rounded_within_the_forward_bound(built_lib, N, b, nq):
    """fpca_debug_k4_fused (k_update_gram16<7>, <4>, and the two launches at 32 columns) on standard-normal data, twice."""
    import flashpca_amd as fp

    V, W, Cin = normal_case(N, b, nq)
    Vl, Wl, Cl = _ld(V), _ld(W), _ld(Cin.reshape(nq * b, b))
    with fp.Context.synthetic(N, 256, n_pop=4, accum="fp64") as ctx:
        Out, Cg = k4_fused(fp, ctx, b, nq, V, W, Cin)
        Out2, Cg2 = k4_fused(fp, ctx, b, nq, V, W, Cin)
    assert np.array_equal(Out, Out2) and np.array_equal(Cg, Cg2), "the fused update + Gram is not deterministic"
    _within(Out, Vl @ Cl + Wl, np.abs(Vl) @ np.abs(Cl) + np.abs(Wl), nq * b + 1, "fused: Out")
    Ol = _ld(Out)
    _within(Cg[:nq].reshape(nq * b, b), Vl.T @ Ol, np.abs(Vl).T @ np.abs(Ol), N, "fused: Cg[:nq]")
    _within(Cg[nq], Ol.T @ Ol, np.abs(Ol).T @ np.abs(Ol), N, "fused: Cg[nq] (Out'Out)")
