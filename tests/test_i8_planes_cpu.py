"""The data of tests/test_gpu_i8_planes.py, checked without a GPU (tests/i8_planes_yardstick.py builds them; the GPU test multiplies the
very same objects): the slicing of every operand is exact and finds the pinned exponent, every digit plane is busy, the sums are exact
in any order, the statistics are dyadic, the digit-level model of the product equals the int64 reference -- and THE DATA TELL: a plane
dropped, weighted by 256 too much or exchanged with its neighbour changes at least a quarter of the outputs of the columns that use it,
for every plane at every S.  The same mutations leave X'B of an integer block in [-4, 4] -- the exact check of the earlier int8 GEMM
tests -- unchanged for every plane but the top one: the gap these tests close.
The data of tests/test_gpu_i8_cheap_passes.py (passes on fewer slices than the context holds) follow at the end: D4's routes per pass, the
transitions every context's sequence of passes must hold, the witness block's digits, and the int64 model of the chained product."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8_planes_yardstick as PY  # noqa: E402
import i8_slice_yardstick as Y  # noqa: E402

SETS = ("D0", "D1", "D2", "D3", "D4")


@pytest.mark.parametrize("name,tall", [(s, False) for s in SETS] + [("D0", True), ("D1", True)])
def test_genotypes_have_dyadic_statistics(name, tall):
    n, P = PY.dims(tall)
    codes = PY.genotypes(name, n, P)
    assert codes.shape == (P, n) and n % 4 == 1
    mean, sd = PY.bed_stats(codes)
    special = {PY.MONO_SNP} | ({PY.NOCALL_SNP} if name in ("D2", "D3") else set())
    plain = np.array([j not in special for j in range(P)])
    assert np.all(mean[plain] == 1.0) and np.all(sd[plain] == 0.5)  # exactly, by k_bed_stats' formulas
    assert mean[PY.MONO_SNP] == 2.0 and sd[PY.MONO_SNP] == 0.0
    GM, M = PY.dosage_called(codes)
    nmiss = (M == 0).sum(axis=1)
    if name in ("D2", "D3"):
        assert nmiss[PY.NOCALL_SNP] == n and np.isnan(mean[PY.NOCALL_SNP]) and np.isnan(sd[PY.NOCALL_SNP])
        M = np.delete(M, PY.NOCALL_SNP, axis=0)
    # the pin samples and pin SNPs: identical records, every call made (the SNP without a call apart)
    assert np.array_equal(codes[:, PY.PIN_SAMPLE], codes[:, PY.PIN_SAMPLE + 1]) and M[:, PY.PIN_SAMPLE].all() and M[:, PY.PIN_SAMPLE + 1].all()
    assert np.array_equal(codes[PY.PIN_SNP], codes[PY.PIN_SNP + 1]) and nmiss[PY.PIN_SNP] == 0 and nmiss[PY.PIN_SNP + 1] == 0
    assert PY.PIN_SAMPLE % 2 == 0 and PY.PIN_SNP % 2 == 0  # adjacent rows of one 256-row chunk
    if name == "D0":
        assert nmiss.sum() == 0
    if name == "D1":
        assert nmiss.max() == 3 and 0.001 < nmiss.sum() / (PY.N * P) < 0.002  # (0.12 % of 701 samples; per SNP the same when taller)
    if name == "D2":
        assert (nmiss == n // 5).sum() == P // 20 and np.sort(nmiss)[-P // 20 - 2] <= 1
    if name == "D4":
        special = [PY.MONO_SNP, PY.PIN_SNP, PY.PIN_SNP + 1, PY.NOCALL_SNP]
        assert not nmiss[special].any() and sorted(np.delete(nmiss, special)) == sorted(np.resize([2, 3, 3, 4], P - 4))
    ms = PY.meansd(name, n, P)
    if name == "D3":
        assert set(ms[:, 0]) <= {0.5, 0.75, 1.0, 1.25, 1.5} and set(ms[:, 1]) <= {0.0, 0.25, 0.5, 1.0, 2.0, 4.0}
        assert len(set(ms[:, 0])) == 5 and len(set(ms[:, 1])) == 6
        assert np.all(ms[[PY.PIN_SNP, PY.PIN_SNP + 1]] == 1.0)
    # the packed stream decodes to the codes
    packed = PY.pack(codes).reshape(P, -1)
    back = np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=2).reshape(P, -1)
    assert np.array_equal(back[:, :n], codes) and np.all(back[:, n:] == 0)


def test_routes():
    """What fpca_missing_mode must answer (the GPU test asserts it per case): D0 2; D1 3 and D2 4 at every S for 16 / 32 / 64 columns."""
    for name, tall, want in (("D0", False, 2), ("D1", False, 3), ("D2", False, 4), ("D0", True, 2), ("D1", True, 3)):
        n, P = PY.dims(tall)
        nmiss = (PY.dosage_called(PY.genotypes(name, n, P))[1] == 0).sum(axis=1)
        for S in range(2, 9):
            for b in (16, 32, 64):
                assert PY.route(nmiss, n, S, b) == want, (name, n, S, b)
    for child in PY.CHILDREN:
        for r in PY.child_runs(child):
            want = {"D0": 2, "D1": 3, "D2": 4}.get(r["ds"]) if r["mode"] is None else r["mode"]
            assert PY.expected_mode(r) == want, r


def test_instance_table(built_lib):
    """fpca_debug_i8_instances (host only): 51 distinct instances; the 8-wave ones are the G.M-alone kernels at 2 and 3.5 tiles, the band-tiled
    layout exists for the two-operand and the G.M-alone kernels only."""
    import flashpca_amd as fp

    table = fp.api.debug_i8_instances()
    assert len(table) == len(set(table)) == 51
    assert {k[:4] for k in table if k[4] == 512} == {(False, 2, 2, False), (False, 2, 4, True)}
    assert all(k[0] or k[1] == 2 for k in table if k[5]) and {k[4] for k in table} == {128, 256, 512}
    n = C.c_int(0)
    assert fp.lib().fpca_debug_i8_instances(None, 0, None) == -1 and "count" in fp.lib().fpca_last_error().decode()
    assert fp.lib().fpca_debug_i8_instances(None, 3, C.byref(n)) == -1 and "keys" in fp.lib().fpca_last_error().decode()
    two = np.full((3, 6), -7, dtype=np.int32)  # a short buffer: the first rows only, the count all the same
    assert fp.lib().fpca_debug_i8_instances(two.ctypes.data_as(C.c_void_p), 2, C.byref(n)) == 0 and n.value == 51
    assert [tuple(int(v) for v in r) for r in two[:2]] == [tuple(int(v) for v in k) for k in table[:2]] and np.all(two[2] == -7)


def test_int_matmul_is_the_int64_product():
    """The references' fast exact product against numpy's own int64 matmul, at the largest magnitudes and the tall shape."""
    rng = np.random.default_rng(3)
    for rows, cols, bits in ((523, 701, 40), (300, 2301, 59), (64, 2560, 37)):
        A = rng.integers(-8, 9, size=(rows, cols), dtype=np.int64)
        n = rng.integers(-(2 ** bits) + 1, 2 ** bits, size=(cols, 16), dtype=np.int64)
        want = A @ n
        if bits == 59:  # (beyond int64 in the sum: Python ints)
            want = np.array([[sum(int(a) * int(v) for a, v in zip(A[i], n[:, c])) for c in range(2)] for i in range(4)], dtype=object)
            got = PY.int_matmul(A, n)
            assert all(int(got[i, c]) == want[i, c] % 2 ** 64 - (2 ** 64 if want[i, c] % 2 ** 64 >= 2 ** 63 else 0) for i in range(4) for c in range(2))
            continue
        assert np.array_equal(PY.int_matmul(A, n), want)
    for key in (("D3", 5, 64, "xt", False), ("D2", 8, 16, "x", False), ("D1", 7, 32, "xt", True)):
        name, S, b, op, tall = key
        n_, p_ = PY.dims(tall)
        o = PY.case_operand(name, S, b, op, 1, n_, p_)
        A = PY.quarter_matrix(name, n_, p_)
        A = A if op == "xt" else A.T
        assert np.array_equal(PY.int_matmul(A, o.n), A @ o.n)


def test_windows_cover_planes_and_pairs():
    for S, W in ((4, 3), (6, 5), (7, 5), (8, 5)):
        offs = PY.window_digits(S, W)
        assert len(offs) == 2  # two blocks rotate every column through every window
        cover = [set(range(j, j + W)) for j in offs]
        assert set().union(*cover) == set(range(S))
        assert all(any({i, i + 1} <= c for c in cover) for i in range(S - 1))


MUTATIONS = ("zero", "weight", "swap")


@pytest.mark.parametrize("key", PY.data_keys(), ids=lambda k: "%s-S%d-b%d-%s" % k[:4] + ("-tall" if k[4] else ""))
def test_case_data(key):
    name, S, b, op, tall = key
    n, P = PY.dims(tall)
    F = 8 * S - 2
    seen = np.zeros((S, b), dtype=bool)
    for block in (0, 1):
        o = PY.case_operand(name, S, b, op, block, n, P)
        V = PY.host_block(name, o, op, n, P)
        ops = [o.x] if op == "xt" else list(PY.k3_operands(name, V, n, P))
        if op == "x":  # T / sd is x again wherever the SNP counts
            live = PY.live_snps(PY.meansd(name, n, P))
            assert np.array_equal(ops[0][live], o.x[live]) and not ops[0][~live].any() and not ops[1][~live].any()
        # the largest partial sum, in quarter units of the lowest occupied plane, over sum |digits| = t.  mean 1 (binom): the G.M sums
        # reach 8 t, the M sums 4 t, their difference 4 t.  D3 (mean = k / 4 <= 1.5): the G.M sums 8 t and mean x the M sums 6 t are
        # partial sums on their own, and the combine's difference of the two can reach 14 t
        amax = 14 if name == "D3" else 8
        for which, x in enumerate(ops):
            sl = Y.Sliced(x, x.shape[0], S, S * b)
            # slicing is exact, entry by entry, and finds the pinned exponent
            assert np.array_equal(np.ldexp(sl.m.astype(np.float64), (sl.e - F)[None, :].astype(np.int32)), x)
            if which == 0:
                assert np.array_equal(sl.e, o.e), (sl.e, o.e)
            elif o.pin is not None:
                assert np.array_equal(sl.e, o.e)  # (the second operand of X T: the pins are SNPs of mean 1, sd 1 -- or mean / sd = 2)
            # the planes meant to be busy are, nothing else is (pins apart)
            D = sl.D.copy()
            if o.pin is not None:
                assert np.all(D[0, o.pin] == 32) and np.all(D[0, o.pin + 1] == -32) and not D[1:, [o.pin, o.pin + 1]].any()
                D[:, [o.pin, o.pin + 1]] = 0
            busy = (D != 0).any(axis=1)
            if which == 0:
                assert np.array_equal(busy, o.planes), (name, S, b, op, block)
                seen |= busy
            # order-free exactness
            tot = PY.order_free_total(sl, o.pin)
            assert amax * max(tot) < 2 ** 53, (max(tot).bit_length(), name, S, b)
            # per-plane column sums are free of the pins
            if o.pin is not None:
                assert np.array_equal(sl.D.astype(np.int64).sum(axis=1), D.astype(np.int64).sum(axis=1))
        if S <= 4 and name in PY.LIST_SETS:  # the fp32 rows of the list routes (k_slice: float32(x 2^(1 - e))) lose nothing
            for x in ops:  # (X T gathers the second operand; today the two are equal, mean / sd = 1 / sd = 2 -- both are held to it)
                e = Y.exponents(Y.column_maxima(x))
                y = np.ldexp(x, (1 - e)[None, :].astype(np.int32))
                assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
                m = np.abs(Y.fixed_point(x, e, S))
                m = m[m > 0]
                assert np.frexp((m // (m & -m)).astype(np.float64))[1].max() <= 21  # significant bits: 13 (S = 2), 21 (S = 3, 4) of 24
        # the digit model equals the integer reference
        model = PY.PlaneProducts(name, o.x, op, S, n, P)
        ref = PY.reference(name, o, op, n, P)
        assert np.isfinite(ref).all() and np.array_equal(model.output(), ref)
        if op == "xt":
            assert not ref[~PY.live_snps(PY.meansd(name, n, P))].any()
        # the data tell
        for s in range(S):
            cols = o.planes[s]
            assert cols.any() or o.kind != "full"
            for mut in MUTATIONS:
                if mut == "swap" and s + 1 >= S:
                    continue
                changed = model.output(mut, s) != ref
                if cols.any():
                    frac = changed[:, cols].mean()
                    assert frac >= 0.25, (name, S, b, op, block, mut, s, frac)
    assert seen.all()  # over the rotation every (plane, column) pair occurred


@pytest.mark.parametrize("S", [3, 4, 7, 8])
def test_integer_blocks_see_the_top_plane_only(S):
    """The gap: X'B on an integer block in [-4, 4] (the exact check of test_gpu_i8_plan / _wide / _pipe3 / _tiled / _missing_gathers) has
    digits in plane 0 alone, so no mutation of a lower plane changes the expected output."""
    b = 16
    B = np.random.default_rng(5).integers(-4, 5, size=(PY.N, b)).astype(np.float64)
    model = PY.PlaneProducts("D1", B, "xt", S)
    assert not model.sl[0].D[1:].any() and model.sl[0].D[0].any()
    ref = model.output()
    for s in range(1, S):
        for mut in MUTATIONS:
            if mut == "swap" and s + 1 >= S:
                continue
            assert np.array_equal(model.output(mut, s), ref)
    assert not np.array_equal(model.output("zero", 0), ref)


# ---- the data of tests/test_gpu_i8_cheap_passes.py: passes on fewer slices than the context holds ----------------------------------------
def test_d4_routes_and_pass_routes():
    """D4 lies between the two break-evens: the context's route is the lists, a pass on at most 4 slices takes the two-matrix kernels."""
    n, P = PY.N, PY.P
    nm = PY.nmiss_of("D4")
    rate = nm.sum() / (n * P)
    assert PY.CHEAP_SPARSE_BREAK_EVEN < rate <= PY.SPARSE_BREAK_EVEN and round(100 * rate, 3) == 0.424
    thr = {S: PY.D_CELL * S / PY.G_CALL * n for S in (6, 7, 8)}
    assert round(thr[6], 2) == 4.12 and round(thr[7], 2) == 4.81 and nm.max() == 4 < thr[6]  # no SNP passes the hybrid route's per-SNP rule
    for S in (6, 7, 8):
        assert not PY.hybrid_dense(nm, n, S).any()
        assert [PY.route(nm, n, S, b) for b in PY.WIDTHS] == [3, 3, 0, 3]
        for Sc in range(2, S + 1):
            for b in (16, 32, 64):
                assert PY.pass_route(nm, n, S, Sc, b) == (0 if Sc <= 4 else 3), (S, Sc, b)
                for name, want in (("D0", 2), ("D1", 3), ("D2", 4)):
                    assert PY.pass_route(PY.nmiss_of(name), n, S, Sc, b) == want, (name, S, Sc, b)
        # the hybrid route's dense SNPs of D2 are the ones `witness_rows` leaves to the matrix cores
        assert np.array_equal(PY.hybrid_dense(PY.nmiss_of("D2"), n, S), PY.nmiss_of("D2") > n // 10)
    for child in PY.CHEAP_CHILDREN:
        for r in PY.cheap_runs(child):
            ctx, cur = PY.expected_pass_modes(r)
            want = {"D0": 2, "D1": 3, "D2": 4, "D3": 0, "D4": 3}[r["ds"]]
            assert ctx == want and cur == (0 if r["ds"] == "D4" and r["Sc"] <= 4 else want), r
    for r in PY.chain_runs():
        assert PY.expected_pass_modes(r)[0] == {"D0": 2, "D1": 3, "D2": 4, "D4": 3}[r["ds"]]


def _nsc_pad(S, b):
    import flashpca_amd as fp

    n = C.c_int(0)
    assert fp.lib().fpca_debug_i8_nsc_pad(S, b, C.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("child", sorted(PY.CHEAP_CHILDREN))
def test_pass_sequences_hold_every_transition(built_lib, child):
    """Whatever the schedules are trimmed to: every context's sequence of (slices, width) still walks through the states ensure_i8,
    ensure_hybrid and the gathers' one operand buffer keep between passes."""
    S, layouts = PY.CHEAP_CHILDREN[child]
    runs = PY.cheap_runs(child)
    assert len({PY.pass_run_id(r) for r in runs}) == len(runs)
    seen_sets = set()
    for tiled in layouts:
        for ds, mode in PY.CHEAP_SETS:
            seq = PY.pass_sequence(S, tiled, ds)
            assert seq == [(r["Sc"], r["b"]) for r in runs if r["ds"] == ds and r["tiled"] == tiled]
            assert all(2 <= Sc <= S and b in PY.WIDTHS and not (b == 48 and ds in PY.LIST_SETS) for Sc, b in seq)
            pairs = list(zip(seq, seq[1:]))
            ragged = lambda Sc, b: Sc * b != _nsc_pad(Sc, b)  # noqa: E731
            assert seq[0][0] == S and seq[-1][0] == S, (ds, tiled)                                              # first and last run exact
            assert any(a[0] == S and c[0] < S for a, c in pairs) and any(a[0] < S and c[0] == S for a, c in pairs)  # exact <-> cheap
            assert any(a[0] <= 4 and c[0] in (5, 6) for a, c in pairs), (ds, tiled)                            # fp32 -> fp64 gather rows
            assert any(a[0] in (5, 6) and c[0] <= 4 for a, c in pairs), (ds, tiled)                            # ... and back
            assert any(a != c and a[0] * a[1] == c[0] * c[1] for a, c in pairs), (ds, tiled)                   # the pad rows' key shared
            assert any(ragged(*c) and a[0] * a[1] > c[0] * c[1] for a, c in pairs), (ds, tiled)                # pad rows under old digits
            assert any(a[0] == c[0] and a[1] != c[1] for a, c in pairs), (ds, tiled)                            # a width change alone
            seen_sets.add(ds)
    assert seen_sets == {"D0", "D1", "D2", "D3", "D4"}
    if None in layouts:  # the default layout runs the whole schedule: every slice count below the context's, every width
        full = PY.pass_sequence(S, None, "D0")
        assert {Sc for Sc, b in full} >= set(range(2, 6)) | {S} and {b for Sc, b in full} == set(PY.WIDTHS)


def _witness_cases():
    keys = set()
    for child in PY.CHEAP_CHILDREN:
        for r in PY.cheap_runs(child):
            if r["ds"] in PY.WITNESS_SETS:
                keys |= {(r["ds"], r["S"], r["Sc"], r["b"], op) for op in ("xt", "x")}
    return sorted(keys)


def test_witness_rows_are_never_gathered():
    for name in PY.WITNESS_SETS:
        GM, M = PY.dosage_called(PY.genotypes(name))
        nm = PY.nmiss_of(name)
        A = PY.quarter_matrix(name)
        dense = PY.hybrid_dense(nm, PY.N, 7) if name == "D2" else np.zeros(PY.P, dtype=bool)
        for op in ("xt", "x"):
            rows = PY.witness_rows(name, op)
            assert 1 <= rows.size <= PY.WITNESS_ROWS
            if op == "xt":  # samples: in no SNP's list (the lists of the hybrid route leave the dense SNPs out)
                assert M[~dense][:, rows].all() and not set(rows) & set(range(PY.PIN_SAMPLE, PY.PIN_SAMPLE + 7))
                assert (A[:, rows] != 0).mean() > 0.2  # ... and they count: most SNPs see them
            else:           # SNPs: in no sample's list
                assert M[rows].all() and not set(rows) & set(range(PY.PIN_SNP, PY.PIN_SNP + 7)) and PY.live_snps(PY.meansd(name))[rows].all()
                assert (A[rows] != 0).mean() > 0.2


@pytest.mark.parametrize("S_ctx", sorted({k[1] for k in _witness_cases()}))
def test_witness_digits(S_ctx):
    """The witness block: at Sc < S its digits ARE block 0's on Sc slices and are not on the context's S; at Sc == S it is exact on the
    finer grid, within the bounds of the other blocks, and its reference is not block 0's."""
    for name, S, Sc, b, op in (k for k in _witness_cases() if k[1] == S_ctx):
        o = PY.case_operand(name, Sc, b, op, 0)
        w = PY.witness_operand(name, S, Sc, b, op)
        rows = PY.witness_rows(name, op)
        assert w.witnessed.shape == (rows.size, b) and w.witnessed.any(axis=0).mean() >= 0.4, (name, S, Sc, b, op, w.witnessed.mean())
        changed = np.zeros(o.x.shape, dtype=bool)
        changed[rows] = w.witnessed
        assert np.array_equal(w.x != o.x, changed)
        V0, V1 = PY.host_block(name, o, op), PY.host_block(name, w, op)
        ops0 = [o.x] if op == "xt" else list(PY.k3_operands(name, V0))
        ops1 = [w.x] if op == "xt" else list(PY.k3_operands(name, V1))
        if op == "x":
            live = PY.live_snps(PY.meansd(name))
            assert all(np.array_equal(x[live], w.x[live]) for x in ops1)  # mean 1, sd 1/2: both operands are the block itself
        for x0, x1 in zip(ops0, ops1):
            at_Sc = Y.Sliced(x0, x0.shape[0], Sc, Sc * b), Y.Sliced(x1, x1.shape[0], Sc, Sc * b)
            if Sc < S:
                at_S = Y.Sliced(x0, x0.shape[0], S, S * b), Y.Sliced(x1, x1.shape[0], S, S * b)
                assert np.array_equal(at_Sc[0].D, at_Sc[1].D) and np.array_equal(at_Sc[0].e, at_Sc[1].e)
                assert np.array_equal(at_S[0].e, at_S[1].e) and np.array_equal((at_S[0].D != at_S[1].D).any(axis=0), changed)
                assert np.array_equal(np.ldexp(at_S[1].m.astype(np.float64), (at_S[1].e - at_S[1].F)[None, :].astype(np.int32)), x1)
            else:
                sl = at_Sc[1]
                assert np.array_equal(np.ldexp(sl.m.astype(np.float64), (sl.e - sl.F)[None, :].astype(np.int32)), x1) and np.array_equal(sl.e, o.e)
                tot = PY.total_in_units(sl, o.pin, w.unit)  # (every digit's term a whole number of the finer units)
                assert 8 * max(tot) < 2 ** 53, (max(tot).bit_length(), name, S, b, op)
        if Sc == S:
            ref0, ref1 = PY.reference(name, o, op), PY.reference(name, w, op)
            cols = w.witnessed.any(axis=0)
            assert np.isfinite(ref1).all() and (ref1 != ref0)[:, cols].mean() > 0.2 and np.array_equal(ref1[:, ~cols], ref0[:, ~cols])
            assert np.array_equal(PY.PlaneProducts(name, w.x, op, S).output(), ref1)


@pytest.mark.parametrize("name", PY.CHAIN_SETS)
def test_chain_data(name):
    """The chained product's model: K2 exact at every slice count, the K3 operands exact at 7 slices and rounded at 4 and 3, every
    partial sum of either stage a whole number of units below 2^53 -- exact in fp64 in any order -- and the slice count TELLS: the model
    of a pass on 4 or 3 slices is not that of 7.  (mean 1, sd 1/2: the two K3 operands are one and the same, T / sd = mean T / sd --
    which of the two maxima the combine leaves for which operand cannot show on these sets.)"""
    GM, M = PY.dosage_called(PY.genotypes(name))
    for b in PY.CHAIN_WIDTHS:
        for k in (0, 1):
            blk = PY.chain_block(name, b, k)
            assert np.abs(blk.n).max() < 2 ** PY.CHAIN_BITS and np.abs(blk.n).max(axis=0).min() >= 2 ** (PY.CHAIN_BITS - 2)
            models = {}
            for Sc in sorted(set(PY.CHAIN_PASSES)):
                slb = Y.Sliced(blk.x, PY.N, Sc, Sc * b)  # K2: the block is exact on the slices, in fp32 rows too
                assert np.array_equal(np.ldexp(slb.m.astype(np.float64), (slb.e - slb.F)[None, :].astype(np.int32)), blk.x)
                y = np.ldexp(blk.x, (1 - slb.e)[None, :].astype(np.int32))
                assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
                assert 8 * max(PY.total_in_units(slb, None, blk.unit)) + 4 * int(np.abs(blk.n).sum(axis=0).max()) < 2 ** 53
                c = models[Sc] = PY.chain_model(name, blk, PY.CHAIN_S, Sc)
                assert c.route == PY.pass_route(PY.nmiss_of(name), PY.N, PY.CHAIN_S, Sc, b)
                assert len(c.ops) == (3 if c.route == 4 else 2) and np.isfinite(c.Y).all()
                for which, sl in enumerate(c.ops):
                    tot = PY.total_in_units(sl, None, c.units)
                    assert 8 * max(tot) + 4 * max(c.gathered) < 2 ** 53
                    deq = np.ldexp(sl.m.astype(np.float64), (sl.e - sl.F)[None, :].astype(np.int32))
                    if Sc == PY.CHAIN_S:
                        assert np.array_equal(deq, sl.x)  # at 7 slices nothing rounds
                    elif which < 2:  # (the few dense SNPs of the hybrid route have column maxima of their own)
                        assert (deq != sl.x)[sl.x != 0].mean() > 0.25, (name, b, k, Sc)  # at 4 and 3 the operands do
            if name == "D0":  # nothing missing, 7 slices: the plain product
                A = PY.quarter_matrix(name)
                want = PY.int_matmul(A.T, PY.int_matmul(A, blk.n))  # (A' A n) 2^(unit - 4) / sd^2 = (A' A n) 2^(unit - 2)
                assert np.array_equal(models[7].Y, np.ldexp(want.astype(np.float64), (blk.unit - 2)[None, :].astype(np.int32)))
            for Sc in (3, 4):
                assert (models[Sc].Y != models[7].Y).mean() > 0.5 and (models[3].Y != models[4].Y).mean() > 0.5, (name, b, k, Sc)
