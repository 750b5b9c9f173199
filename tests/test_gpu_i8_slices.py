"""Byte-level tests of the kernels that cut an fp64 operand into int8 digit planes (csrc/kernels_i8.hip: k_colmax, k_slice, k_maxbits_fold,
k_maxbits_set, k_slice_rows, k_unpack_slices, k_dequant_rows) through fpca_debug_i8_slices, which drives the host launchers the operator
calls, in its order, on poisoned buffers.  The reference is tests/i8_slice_yardstick.py: the contract of the kernel file's header in
int64 arithmetic.  The operand is test_i8_slices_cpu.special_block, whose premises that file asserts without a device.

Every comparison is exact: np.array_equal on bytes, integers and the bit patterns of floats.  No tolerances -- except in the one
end-to-end check at the bottom, which says why.

 route 0 (the operator's own slicing: i8_colmax, i8_slice)
   tiny (rows, rows_pad, b, S) = (1, 16, 16, 7), (17, 32, 16, 4); the sweep b x S at 1003 / 1056 rows (three whole pad groups behind a
   cut one; 17 workgroups at b = 64: all 8 accumulator shards); 16 columns at 2112 rows (9 workgroups); two operands with row scales,
   column sums on the second or on both, copies on one or both; the 1024-workgroup cap of i8_colmax at 16400 rows; the 4096-workgroup
   cap of i8_slice at 262184 / 262192 rows.
 route 1 (the exchange: i8_slice_rows, i8_unpack_slices, i8_dequant_rows) against the yardstick AND against route 0 with the same
   maxima installed: S b over every class of i8_unpack_slices' tile height and its boundaries, rows_pad below one tile / 2 tiles + 3
   groups / whole tiles, rows_valid 0 / mid-group in the last tile / all, peers none / one smaller / seven with larger maxima.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8_slice_yardstick as Y  # noqa: E402
import test_i8_slices_cpu as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(built_lib):
    from flashpca_amd import api

    return api


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(Y.bits(a), Y.bits(b))


def check_common(out, y, colsum, what):
    """What both routes leave: maxima, digits in the GEMM's layout, weights at their padded length, column sums."""
    S, b = y.S, y.b
    assert out["nsc_pad"] == y.nsc_pad and out["colw"].shape == (y.nsc_pad,), what
    assert same_bits(out["colmax"][:b], y.own_max), (what, "own maxima")
    assert not out["colmax"][b:].any(), (what, "maxima behind b")
    assert same_bits(Y.fold_maxbits(out["maxbits_own"])[:b], y.own_max), (what, "the raw shards do not fold to the maxima")
    assert same_bits(Y.fold_maxbits(out["maxbits"])[:b], y.colmax), (what, "installed maxima")
    assert same_bits(out["colw"], y.colw), (what, "colw", np.nonzero(Y.bits(out["colw"]) != Y.bits(y.colw))[0][:8])
    q = y.Q()
    if not np.array_equal(out["Q"], q):
        sc, pos = np.nonzero(out["Q"] != q)
        raise AssertionError("%s: Q differs in %d bytes, first at slice %d column %d position %d: %d, expected %d" % (
            what, sc.size, sc[0] // b, sc[0] % b, pos[0], out["Q"][sc[0], pos[0]], q[sc[0], pos[0]]))
    if colsum:
        assert np.array_equal(out["colsum"][:S * b], y.colsum), (what, "colsum")
        assert not out["colsum"][S * b:].any() and not out["colsum_shards"][:, S * b:].any(), (what, "colsum behind S b")
    else:
        assert "colsum" not in out


def copy_kind(S):
    return 32 if S <= 4 else 64  # what the operator asks for: fp32 rows carry the 30 bits of four slices, no more


def check_slice_copy(out, y, kind, what):
    want = y.slice_copy32() if kind == 32 else y.slice_copy64()
    if kind == 32:
        a = np.abs(want[:y.rows].astype(np.float64))
        assert np.all((a == 0) | (a >= 2.0 ** -100))  # (premise: fp32 denormal modes play no part)
    assert same_bits(out["copy%d" % kind], want), (what, "copy%d" % kind)


def run_a(api, rows, rows_pad, b, S, seed=0, copy=True):
    V = G.special_block(rows, rows_pad, b, S, seed)
    kind = copy_kind(S) if copy else None
    out, = api.debug_i8_slices(V, b, S, rows=rows, route=0, colsum=(True, True), copy=(kind, None))
    y = Y.Sliced(V, rows, S, out["nsc_pad"])
    return V, out, y, kind


# ---- route 0 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,rows_pad,b,S", [(1, 16, 16, 7), (17, 32, 16, 4)])
def test_slice_tiny(api, rows, rows_pad, b, S):
    V, out, y, kind = run_a(api, rows, rows_pad, b, S)
    check_common(out, y, True, (rows, b, S))
    check_slice_copy(out, y, kind, (rows, b, S))


@pytest.mark.parametrize("S", [2, 4, 5, 7, 8])
@pytest.mark.parametrize("b", [16, 32, 48, 64])
def test_slice_sweep(api, b, S):
    rows, rows_pad = G.MAIN
    V, out, y, kind = run_a(api, rows, rows_pad, b, S)
    check_common(out, y, True, (b, S))
    check_slice_copy(out, y, kind, (b, S))
    assert not out["Q"][:S * b, rows // 16 * 16 + 16:].any()  # the three whole pad groups are written, as zeros
    # different columns' maxima sit in different accumulator shards; unused shards stay zero
    own = out["maxbits_own"]
    spiked = [c for c in range(b) if c % 16 in (G.POW2NEG, G.SINGLE, G.BIG, G.SMALL, G.LASTROW) or c % 16 >= 10]
    holders = {int(np.argmax(own[:, c])) for c in spiked}
    assert len(holders) >= 4, holders
    assert all(np.count_nonzero(own[:, c]) == 1 for c in range(b) if c % 16 == G.SINGLE)
    cs = y.colsum.reshape(S, b)
    assert all(cs[:, c].any() for c in range(b) if c % 16 != G.ZERO)  # no column sum is trivially zero
    if b == 64:
        assert all(out["colsum_shards"][k].any() for k in range(8))  # 17 workgroups: every shard took part


def test_slice_16_columns_all_shards(api):
    rows, rows_pad, b, S = 2101, 2112, 16, 4
    V, out, y, kind = run_a(api, rows, rows_pad, b, S)
    check_common(out, y, True, "16 columns, 9 workgroups")
    check_slice_copy(out, y, kind, "16 columns, 9 workgroups")
    assert all(out["colsum_shards"][k].any() for k in range(8))


TWO_OPS = [  # b, S, colsum, copy
    (32, 4, (False, True), (None, 32)), (32, 4, (True, True), (32, 32)), (16, 2, (False, True), (32, None)),
    (48, 7, (False, True), (None, 64)), (64, 5, (True, True), (64, 64)), (64, 8, (True, True), (64, None)),
]


@pytest.mark.parametrize("b,S,colsum,copy", TWO_OPS)
def test_slice_two_operands(api, b, S, colsum, copy):
    rows, rows_pad = G.MAIN
    V = G.special_block(rows, rows_pad, b, S)
    rs = [G.row_scales(rows, 100 * S + b, o) for o in range(2)]
    assert all((r == 0).any() for r in rs)
    outs = api.debug_i8_slices(V, b, S, rows=rows, route=0, rowscales=rs, colsum=colsum, copy=copy)
    ys = [Y.Sliced(V, rows, S, outs[0]["nsc_pad"], rowscale=r) for r in rs]
    assert (ys[0].e != ys[1].e).any() and not np.array_equal(ys[0].D, ys[1].D)  # each operand's maxima and digits are its own
    for o in range(2):
        check_common(outs[o], ys[o], colsum[o], (b, S, "operand", o))
        for kind in (32, 64):
            if copy[o] == kind:
                check_slice_copy(outs[o], ys[o], kind, (b, S, "operand", o))
            else:
                assert "copy%d" % kind not in outs[o]


def test_slice_one_scaled_operand(api):
    rows, rows_pad, b, S = 333, 336, 48, 5
    V = G.special_block(rows, rows_pad, b, S)
    rs = G.row_scales(rows, 5)
    out, = api.debug_i8_slices(V, b, S, rows=rows, route=0, rowscales=[rs], copy=(64, None))
    y = Y.Sliced(V, rows, S, out["nsc_pad"], rowscale=rs)
    check_common(out, y, True, "one scaled operand")
    check_slice_copy(out, y, 64, "one scaled operand")


def test_colmax_workgroup_cap(api):
    """16400 rows x 64 columns: i8_colmax would want 1026 workgroups and takes 1024, so the grid-stride loop comes round for rows from
    16384 on.  Only the maxima are compared."""
    rows, b, S = 16400, 64, 4
    rng = np.random.default_rng(16400)
    V = rng.uniform(-1.0, 1.0, size=(rows, b))
    where = {3: 16399, 17: 16383, 40: 16384, 41: 16384, 63: 16399, 0: 0, 5: 4095, 6: 4096}
    for c, r in where.items():
        V[r, c] = -7.0 - c
    out, = api.debug_i8_slices(V, b, S, route=0, colsum=(False, False))
    want = np.abs(V).max(axis=0)
    assert all(want[c] == 7.0 + c for c in where)
    assert same_bits(out["colmax"], want) and same_bits(Y.fold_maxbits(out["maxbits_own"]), want)
    assert same_bits(Y.fold_maxbits(out["maxbits"]), want)


def test_slice_workgroup_cap(api):
    """262184 rows x 64 columns: 16387 row groups, four per workgroup, 4097 wanted and 4096 taken -- the one shape at which k_slice's
    grid-stride loop runs a second time (for the last three groups).  All outputs."""
    rows, rows_pad, b, S = 262184, 262192, 64, 4
    V, out, y, kind = run_a(api, rows, rows_pad, b, S)
    check_common(out, y, True, "4096-workgroup cap")
    check_slice_copy(out, y, kind, "4096-workgroup cap")


# ---- route 1 ------------------------------------------------------------------------------------------------
def trg_of(SB):
    """16-row groups per workgroup of i8_unpack_slices, from the comment at its launch: 32 up to 128 slice-columns, 16 up to 272, else 8."""
    return 32 if SB <= 128 else 16 if SB <= 272 else 8


SB_CASES = [(4, 16), (4, 32), (8, 16), (3, 48), (7, 32), (4, 64), (7, 48), (7, 64), (8, 64)]  # S b = 64 128 128 144 224 256 336 448 512
PAD_KINDS = ("below one tile", "two tiles and three groups", "whole tiles")
PEER_KINDS = ("none", "one smaller", "seven, one larger in half of the columns")


def make_peers(kind, own_max, b, seed):
    if kind == PEER_KINDS[0]:
        return None
    rng = np.random.default_rng(seed)
    if kind == PEER_KINDS[1]:
        p = np.zeros((1, 64))
        p[0, :b] = own_max * 0.75
        return p
    p = np.zeros((7, 64))
    p[:, :b] = own_max[None, :] * rng.uniform(0.0, 0.9, size=(7, b))
    p[4, 1:b:2] = own_max[1:b:2] * 600.0 + 3.0  # (+ 3: the 2^-900 columns' exponents rise by 900)
    p[:, b:] = 0.0
    return p


@pytest.mark.parametrize("peer_kind", PEER_KINDS)
@pytest.mark.parametrize("pad_kind", PAD_KINDS)
@pytest.mark.parametrize("S,b", SB_CASES)
def test_exchange(api, S, b, pad_kind, peer_kind):
    trg = trg_of(S * b)
    assert [trg_of(n) for n in (128, 129, 144, 272, 273, 512)] == [32, 16, 16, 16, 8, 8]
    groups = {PAD_KINDS[0]: 3, PAD_KINDS[1]: 2 * trg + 3, PAD_KINDS[2]: 2 * trg}[pad_kind]
    rows_pad = 16 * groups
    assert (groups < trg) == (pad_kind == PAD_KINDS[0]) and (groups % trg == 3) == (pad_kind != PAD_KINDS[2])
    rows = rows_pad - 3
    V = G.special_block(rows, rows_pad, b, S, seed=1)
    own = np.abs(V).max(axis=0)
    peers = make_peers(peer_kind, own, b, 1000 * S + b)
    allmax = own if peers is None else np.maximum(own, peers[:, :b].max(axis=0))
    kind = copy_kind(S)
    dequant = (32, 64) if S <= 4 else (64,)
    y = None
    last_tile0 = (groups - 1) // trg * trg * 16  # first row of the last tile
    mid = max(last_tile0 + 16, rows_pad - 16) + 11 if groups > 1 else 11  # five rows short of a group boundary, inside the last tile
    assert last_tile0 <= mid < rows_pad and mid % 16 == 11
    for rows_valid in (0, mid, rows_pad):
        what = (S, b, rows_pad, rows_valid, peer_kind)
        out, = api.debug_i8_slices(V, b, S, rows=rows, route=1, peers=peers, rows_valid=rows_valid, copy=(kind, None), dequant=dequant)
        if y is None:
            y = Y.Sliced(V, rows, S, out["nsc_pad"], colmax=allmax)
            if peer_kind == PEER_KINDS[1]:
                assert same_bits(y.colmax, y.own_max)  # smaller maxima change nothing
            if peer_kind == PEER_KINDS[2]:
                alone = Y.Sliced(V, rows, S, out["nsc_pad"])
                odd = np.arange(1, b, 2)
                assert np.all(y.e[odd] > alone.e[odd] + 8) and np.array_equal(y.e[::2], alone.e[::2])  # exponents rise ...
                assert not y.D[0][:, odd].any() and np.all(y.colw[odd] > alone.colw[odd])                # ... top digits shrink, weights follow
        check_common(out, y, True, what)
        assert not out["maxbits"][1:].any() and same_bits(out["maxbits"][0].view(np.float64)[:b], allmax), (what, "shards after i8_maxbits_set")
        assert not out["maxbits"][0][b:].any()
        assert np.array_equal(out["Qrm"], y.Qrm()), (what, "Qrm")
        want = y.exchange_copy32(rows_valid) if kind == 32 else y.exchange_copy64(rows_valid)
        got = out["copy%d" % kind]
        assert same_bits(got, want), (what, "copy%d of i8_unpack_slices" % kind)
        assert np.all(Y.bits(got[rows_valid:]) == Y.bits(want[rows_valid:])) and np.all(np.isnan(got[rows_valid:]))  # the poison stays
        for w in dequant:
            full = y.exchange_copy32(rows_pad) if w == 32 else y.exchange_copy64(rows_pad)
            assert same_bits(out["dq%d" % w], full), (what, "dq%d of i8_dequant_rows" % w)
            if w == kind:
                assert same_bits(out["dq%d" % w][:rows_valid], got[:rows_valid]), (what, "the two kernels' rows differ")
    # route 0 with the same maxima installed: the same bytes
    a, = api.debug_i8_slices(V, b, S, rows=rows, route=0, peers=peers)
    check_common(a, y, True, (S, b, rows_pad, "route 0", peer_kind))
    assert np.array_equal(a["Q"], out["Q"]) and same_bits(a["colw"], out["colw"]) and np.array_equal(a["colsum"], out["colsum"])
    if peers is not None:
        assert not a["maxbits"][1:].any() and same_bits(a["maxbits"][0].view(np.float64)[:b], allmax)


def test_exchange_copy64_at_four_slices(api):
    """The fp64 rows at S <= 4: what a rank on the fp64 kernels makes of the gathered slices (apply_sharded: i8_dequant_rows, copy64)."""
    S, b, rows_pad = 4, 48, 16 * 19
    rows = rows_pad - 9
    V = G.special_block(rows, rows_pad, b, S, seed=2)
    out, = api.debug_i8_slices(V, b, S, rows=rows, route=1, rows_valid=rows, copy=(64, None), dequant=(64,))
    y = Y.Sliced(V, rows, S, out["nsc_pad"])
    check_common(out, y, True, "copy64 at four slices")
    assert same_bits(out["copy64"], y.exchange_copy64(rows)) and same_bits(out["dq64"], y.exchange_copy64(rows_pad))


# ---- the operator uses what was tested ------------------------------------------------------------------------
def test_operator_multiplies_the_tested_operand(api):
    """One apply_xt on a 517 x 300 synthetic i8x4 context (no missing calls: at four slices their term is gathered from the fp32 rows,
    which carry 24 bits of an entry, not the 30 of the slices, and have tests of their own) of a block with the special columns, against
    X' Bq where Bq = sum_s colw digit
    is the operand recombined from the yardstick's digits and weights (exact in fp64: 30-bit integers times powers of two) and X the
    oracle's dense standardised matrix, multiplied in extended precision.
    This one check is a bound, 2^-(8S-2) of the column maximum times |X|' 1, not an identity: the product is recombined on the device
    as diag(1/sd) ((G.M)'Q - diag(mean) M'Q) per split-K part and per slice, with the missing calls' term from a gather route chosen
    where calls are missing; its summation order follows the split plan of the launch, which the comments of k_i8_combine do not fix for a
    reader who does not copy the kernels.  A digit plane that the operator cut differently from the tested kernels by one unit in
    one entry of a top plane, a wrong weight or another byte order moves the result by 2^-(8S-2) 256^(S-1) of the maximum or more."""
    import flashpca_amd as fp
    from oracle import oracle as O

    N, P, b, S = 517, 300, 16, 4
    B = G.special_block(N, 528, b, S)[:N]
    with fp.Context.synthetic(N, P, n_pop=4, missing_rate=0.0, accum="i8x4") as ctx:
        X = O.OracleData(packed=ctx.download_packed(), N=N, P=P, stand="binom2").dense()
        T = ctx.apply_xt(B)
    y = Y.Sliced(np.vstack([B, np.zeros((11, b))]), N, S, G.nsc_pad_of(S, b))
    LD = np.longdouble
    Bq = np.zeros((N, b), dtype=LD)
    for s in range(S):
        Bq += y.D[s, :N].astype(LD) * y.colw[s * b:(s + 1) * b].astype(LD)[None, :]
    assert np.array_equal(Bq.astype(np.float64), np.ldexp(y.m[:N].astype(np.float64), (y.e - y.F)[None, :].astype(np.int32)))
    ref = X.astype(LD).T @ Bq
    bound = np.abs(X).sum(axis=0)[:, None].astype(LD) * (y.own_max.astype(LD) * LD(2.0) ** -(8 * S - 2))[None, :]
    err = np.abs(T.astype(LD) - ref)
    print("worst error / bound per column:", np.array2string(np.max(err / np.where(bound > 0, bound, 1), axis=0).astype(np.float64), precision=2))
    assert np.all(np.isfinite(T)) and np.all(err <= bound), np.argwhere(err > bound)[:5]
    assert not T[:, G.ZERO].any()
