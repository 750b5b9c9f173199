"""The inputs of tests/test_gpu_i8_slices.py, the yardstick's own consistency, and the refusals of fpca_debug_i8_slices.  No device.

 * special_block(rows, rows_pad, b, S): the operand every GPU case slices.  Column c is of kind c % 16 (below), repeated every 16 columns
   at another scale; the tests here assert on the block itself that it holds what the GPU tests are about, so that an edit of the
   generator cannot hollow them out.
 * the yardstick (tests/i8_slice_yardstick.py): digits recombine to m in Python ints, ranges, the layout maps are permutations.
 * every refusal of the hook comes before anything touches the device, so they are tested here, on the product library.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8_slice_yardstick as Y  # noqa: E402

TIES, ALT, CARRY, POW2NEG, ZERO, SINGLE, BIG, SMALL, DECAY, LASTROW = range(10)  # kinds 10 .. 15: normal columns with one spike
ALL_S = (2, 3, 4, 5, 6, 7, 8)
MAIN = (1003, 1056)  # rows, rows_pad of the main sweep: three whole pad groups behind a cut one
REP_SHIFT = (-3, 5, 0, 11)  # binary exponent offset of the r-th repetition of the 16 kinds


def spike_row(c, rows):
    """Where column c holds its maximum (the kinds with one): spread over the rows, so over the accumulator shards."""
    return rows - 1 if c % 16 == LASTROW else (37 * c + 11) % rows


def carry_integers(S):
    """Integers below 2^(8S-2), each exact in fp64 (at most 48 significant bits), whose digits reach -128 and +127 in every plane below
    the top and +-64 in the top one: runs of one byte value over up to six planes.  The bytes 0x80 and 0x7F and their negatives make
    the carries run the whole length of the run (0x80 reads as -128 and carries one into the next 0x80, and so on)."""
    top = 256 ** (S - 1)

    def run(d, lo, hi):
        return sum(d * 256 ** i for i in range(lo, hi))

    near_top = (max(0, S - 6), S - 1)
    vals = [64 * top + run(-128, *near_top), -64 * top + run(127, *near_top)]  # (first: the column maximum, in [2^(F-1), 2^F))
    for lo in range(S - 1):
        hi = min(lo + 6, S - 1)
        for d in (-128, 127, 0x80, 0x7F):
            vals += [run(d, lo, hi), -run(d, lo, hi)]
    for v in vals:
        assert int(float(v)) == v and abs(v) < 2 ** (8 * S - 2)
    return vals


def special_block(rows, rows_pad, b, S, seed=0):
    rng = np.random.default_rng([seed, rows, b, S])
    F = 8 * S - 2
    V = np.zeros((rows_pad, b))
    r = np.arange(rows)
    sign3 = np.where(r % 3 == 2, -1.0, 1.0)  # + + - : a column of them sums to something
    for c in range(b):
        kind, k = c % 16, REP_SHIFT[c // 16]
        sp = spike_row(c, rows)
        if kind == TIES:  # e = 1: scaled values k + 1/2, odd and even k; the maximum 1.0 at the spike
            lim = 2 ** min(F - 2, 50)
            col = np.ldexp(rng.integers(-lim, lim, size=rows).astype(np.float64) + 0.5, 1 - F)
            col[sp] = 1.0
            col = np.ldexp(col, k)
        elif kind == ALT:
            col = sign3 * np.nextafter(np.ldexp(1.0, k), 0.0)
        elif kind == CARRY:  # e = k + 1
            vals = np.array([np.ldexp(float(v), k + 1 - F) for v in carry_integers(S)])
            col = vals[r % vals.size]
        elif kind == POW2NEG:
            col = np.ldexp(rng.uniform(-0.9, 0.9, size=rows), k)
            col[sp] = -np.ldexp(1.0, k)
        elif kind == ZERO:
            col = np.zeros(rows)
        elif kind == SINGLE:
            col = np.zeros(rows)
            col[sp] = np.ldexp(rng.uniform(1.0, 2.0), k) * (-1.0 if c // 16 % 2 else 1.0)
        elif kind == DECAY:
            col = sign3 * rng.uniform(0.5, 1.0, size=rows) * np.ldexp(1.0, k) * 2.0 ** (-70.0 * r / max(rows - 1, 1))
        else:
            shift = {BIG: 900, SMALL: -900}.get(kind, k + kind)
            col = rng.standard_normal(rows)
            col[sp] = (5.0 if kind == LASTROW else 1.5) * np.abs(col).max() * (-1.0 if c % 2 else 1.0)
            col = np.ldexp(col, shift)
        V[:rows, c] = col
    return V


def row_scales(rows, seed, col=0):
    """The K3 operands' row factors: log-uniform over six decades, some rows exactly zero, either sign."""
    rng = np.random.default_rng([seed, rows, col])
    rs = 10.0 ** rng.uniform(-3, 3, size=rows) * rng.choice([-1.0, 1.0], size=rows)
    rs[rng.random(rows) < 0.05] = 0.0
    return rs


def nsc_pad_of(S, b):
    import flashpca_amd as fp

    n = C.c_int(0)
    assert fp.lib().fpca_debug_i8_nsc_pad(S, b, C.byref(n)) == 0
    return n.value


# ---- the yardstick -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=ALL_S)
def main_block(request):
    S = request.param
    V = special_block(MAIN[0], MAIN[1], 16, S)
    return S, V, Y.Sliced(V, MAIN[0], S, 16 * S + 16)


def test_digits_recombine_in_python_ints(main_block):
    S, V, y = main_block
    F = 8 * S - 2
    assert y.D.dtype == np.int8 and y.D.shape == (S, MAIN[1], 16)
    assert np.all(np.abs(y.D[0].astype(int)) <= 64) and np.all(np.abs(y.m) <= 2 ** F)
    rng = np.random.default_rng(S)
    rows = set(rng.integers(0, MAIN[0], 60).tolist()) | {0, MAIN[0] - 1, MAIN[0], MAIN[1] - 1}
    for r in rows:
        for c in range(16):
            assert Y.python_int_value(y.D, r, c) == int(y.m[r, c])
            e = int(y.e[c])
            want = int(np.rint(np.ldexp(np.longdouble(y.x[r, c]), F - e))) if abs(F - e) < 16000 else None  # 64-bit mantissa: exact up to 2^62
            assert want == int(y.m[r, c])
    # the same recombination for all entries at once: Horner from the top, exact in int64 as |m| <= 2^62
    acc = np.zeros(y.m.shape, dtype=np.int64)
    for s in range(S):
        acc = acc * 256 + y.D[s]
    assert np.array_equal(acc, y.m)
    assert not y.m[MAIN[0]:].any() and not y.D[:, MAIN[0]:].any()  # rows >= rows hold zero
    assert np.array_equal(y.colsum, np.array([int(y.D[s, :, c].astype(int).sum()) for s in range(S) for c in range(16)]))


def test_layouts_are_permutations():
    S, rows_pad, b = 3, 48, 16
    assert sorted(Y.GROUP_ROW.tolist()) == list(range(16))
    tag = np.arange(S * rows_pad * b, dtype=np.int64).reshape(S, rows_pad, b)  # every entry its own number
    q = Y.q_layout(tag)
    qrm = Y.qrm_layout(tag)
    assert q.shape == (S * b, rows_pad) and qrm.shape == (rows_pad, S * b)
    assert sorted(q.ravel().tolist()) == sorted(qrm.ravel().tolist()) == list(range(tag.size))
    for s, c, g, qq, t in [(0, 0, 0, 0, 0), (1, 5, 2, 3, 1), (2, 15, 1, 0, 3), (0, 7, 2, 2, 2), (2, 0, 0, 1, 0)]:
        row = 16 * g + qq + 4 * t
        assert q[s * b + c, 16 * g + 4 * qq + t] == tag[s, row, c] == qrm[row, s * b + c]


def test_weights_and_exponents():
    e = Y.exponents(np.array([0.0, 1.0, 0.75, np.nextafter(1.0, 0), 2.0 ** 900, 2.0 ** -900, 3.0]))
    assert e.tolist() == [0, 1, 0, 0, 901, -899, 2]
    w = Y.weights(np.array([1, -2] + [0] * 14), 3, 64)
    assert w[0] == 2.0 ** (1 - 22 + 16) and w[16] == 2.0 ** (1 - 22 + 8) and w[32] == 2.0 ** (1 - 22) and w[33] == 2.0 ** (-2 - 22)
    assert not w[48:].any() and np.all(w[:48] > 0)


# ---- the premises of the GPU inputs ----------------------------------------------------------------------------
def test_special_block_premises(main_block):
    S, V, y = main_block
    F, rows = 8 * S - 2, MAIN[0]
    x, D, e = y.x[:rows], y.D[:, :rows], y.e
    assert np.all(np.isfinite(V)) and not V[rows:].any()
    nz = x != 0
    assert np.all(np.abs(x[nz]) >= 2.0 ** -1022) and np.all(e - F > -1000) and np.all(e < 1000)  # no denormals, weights far from underflow
    # rint ties, in both directions
    t = np.ldexp(x[:, TIES], F - int(e[TIES]))
    half = (t - np.floor(t)) == 0.5
    assert half.sum() >= 100
    odd = np.floor(t[half]) % 2 == 1
    assert odd.sum() >= 30 and (~odd).sum() >= 30
    assert np.array_equal(y.m[:rows, TIES][half], np.where(odd, np.floor(t[half]) + 1, np.floor(t[half])).astype(np.int64))
    # every plane below the top reaches both ends of the digit range
    for s in range(1, S):
        assert D[s].min() == -128 and D[s].max() == 127, (S, s)
    # the top digit reaches +-64 by both kinds of column
    for c in (ALT, CARRY):
        assert D[0, :, c].max() == 64 and D[0, :, c].min() == -64, (S, c)
    assert np.all(np.abs(V[:rows, ALT]) == np.nextafter(2.0 ** REP_SHIFT[0], 0)) and (V[:rows, ALT] > 0).any() and (V[:rows, ALT] < 0).any()
    carry_m = set(int(v) for v in y.m[:rows, CARRY])
    assert carry_m == set(carry_integers(S))  # the column holds exactly the integers it was built from
    # a maximum that is a power of two, attained by a negative entry
    f, _ = np.frexp(y.own_max[POW2NEG])
    assert f == 0.5 and x[np.argmax(np.abs(x[:, POW2NEG])), POW2NEG] < 0 and D[0, :, POW2NEG].min() == -32
    assert not x[:, ZERO].any() and e[ZERO] == 0
    assert np.count_nonzero(x[:, SINGLE]) == 1
    assert e[BIG] > 890 and e[SMALL] < -890
    d = np.abs(x[:, DECAY])
    assert d.min() > 0 and d.min() / d.max() <= 2.0 ** -69
    if F < 69:
        assert (y.m[:rows, DECAY] == 0).sum() > 10  # low entries round to zero
    # the maxima: one per spiked column, at its row; one of them in the last valid row
    for c in range(16):
        if c in (POW2NEG, SINGLE, BIG, SMALL, LASTROW) or c >= 10:
            assert np.argmax(np.abs(x[:, c])) == spike_row(c, rows), c
    assert spike_row(LASTROW, rows) == rows - 1 and len({spike_row(c, rows) // 64 for c in range(16)}) >= 8
    # colsum is nowhere trivially zero
    cs = y.colsum.reshape(S, 16)
    assert all(cs[:, c].any() for c in range(16) if c != ZERO)


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("two", [False, True])
def test_copy32_values_are_far_from_fp32_denormals(S, two):
    """Every expected copy32 value is zero or at least 2^-100 in magnitude: fp32 denormal modes play no part."""
    V = special_block(MAIN[0], MAIN[1], 64, S)
    ys = [Y.Sliced(V, MAIN[0], S, 640, rowscale=row_scales(MAIN[0], S, o)) for o in range(2)] if two else [Y.Sliced(V, MAIN[0], S, 640)]
    for y in ys:
        for got in (y.slice_copy32()[:MAIN[0]], y.exchange_copy32(MAIN[0])[:MAIN[0]]):
            a = np.abs(got.astype(np.float64))
            assert np.all(np.isfinite(a)) and np.all((a == 0) | (a >= 2.0 ** -100)) and a.max() <= 2.0


def test_two_operand_inputs_differ():
    """Each operand's maxima and digits are its own: the two row scalings give different exponents in several columns (five are asked:
    an operand sliced with the other's maxima then differs in more than a corner) and different digits."""
    S = 5
    V = special_block(MAIN[0], MAIN[1], 32, S)
    rs = [row_scales(MAIN[0], 77, o) for o in range(2)]
    assert all((r == 0).sum() >= 20 and np.log10(np.abs(r[r != 0]).max() / np.abs(r[r != 0]).min()) > 5 for r in rs)
    a, b = (Y.Sliced(V, MAIN[0], S, 256, rowscale=r) for r in rs)
    assert (a.e != b.e).sum() >= 5 and not np.array_equal(a.D, b.D)
    assert (a.x[:MAIN[0]][rs[0] == 0] == 0).all()


# ---- the hook's refusals ------------------------------------------------------------------------------------
def _call(L, route=0, b=16, S=4, rows=20, rows_pad=32, rows_valid=0, V="ok", rs0=None, rs1=None, peers=None, n_peers=None, out0="ok", out1=None,
          fields=()):
    import flashpca_amd as fp

    keep = []

    def ptr(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    if isinstance(V, str):
        V = np.ones((max(rows_pad, 16), 64))
    st = [fp._lib.SlicesOut(), fp._lib.SlicesOut()]
    scratch = np.zeros(8)  # (a refused call writes nothing: any non-NULL address serves as a switch)
    for o, name in fields:
        setattr(st[o], name, scratch.ctypes.data)
    rc = L.fpca_debug_i8_slices(route, b, S, rows, rows_pad, rows_valid, ptr(V), ptr(rs0), ptr(rs1), ptr(peers),
                                (0 if peers is None else len(peers)) if n_peers is None else n_peers,
                                C.byref(st[0]) if out0 is not None else None, C.byref(st[1]) if out1 is not None else None, None)
    return rc, L.fpca_last_error().decode()


ONES = np.ones(20)
NAN_V = np.ones((32, 16))
NAN_V[19, 3] = np.nan
INF_V = np.ones((32, 16))
INF_V[0, 0] = -np.inf
BAD_RS = np.ones(20)
BAD_RS[7] = np.inf
REFUSALS = [
    (dict(route=2), "route"),
    (dict(b=24), "b must be"), (dict(b=0), "b must be"), (dict(b=80), "b must be"),
    (dict(S=1), "S must be"), (dict(S=9), "S must be"),
    (dict(rows_pad=40), "rows_pad"), (dict(rows_pad=0, rows=0), "rows_pad"), (dict(rows_pad=(1 << 20) + 16), "rows_pad"),
    (dict(rows=33), "rows is larger"), (dict(rows_valid=33, route=1), "rows_valid"),
    (dict(route=1, S=7, b=64 + 16), "b must be"),  # (S b > 512 is refused too, but no b and S of the two sets reach it)
    (dict(V=None), "V is NULL"), (dict(out0=None), "out0"),
    (dict(rs1=ONES), "rowscale1"), (dict(rs0=ONES, rs1=ONES), "out1"), (dict(rs0=ONES, out1="ok"), "out1"),
    (dict(route=1, rs0=ONES, rs1=ONES, out1="ok"), "rowscale1"),
    (dict(peers=np.ones((1, 64)), n_peers=0), "n_peers"), (dict(n_peers=2), "n_peers"), (dict(peers=np.ones((64, 64))), "n_peers"),
    (dict(peers=np.ones((1, 64)), rs0=ONES, rs1=ONES, out1="ok"), "peers"),
    (dict(fields=[(0, "copy32"), (0, "copy64")]), "copy32 and copy64"),
    (dict(S=5, fields=[(0, "copy32")]), "copy32"), (dict(S=5, route=1, fields=[(0, "dq32")]), "dq32"),
    (dict(fields=[(0, "Qrm")]), "Qrm"), (dict(fields=[(0, "dq64")]), "dq64"),
    (dict(V=NAN_V), "V holds"), (dict(V=INF_V), "V holds"),
    (dict(rs0=BAD_RS), "rowscale0"), (dict(rs0=ONES, rs1=BAD_RS, out1="ok"), "rowscale1"),
    (dict(peers=np.full((2, 64), np.nan)), "peers"), (dict(peers=np.full((1, 64), -1.0)), "peers"), (dict(peers=np.full((1, 64), np.inf)), "peers"),
]


@pytest.mark.parametrize("kw,word", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_hook_refuses(built_lib, kw, word):
    import flashpca_amd as fp

    rc, msg = _call(fp.lib(), **kw)
    assert rc == -1, (kw.keys(), msg)  # FPCA_EINVAL
    assert msg.startswith("fpca_debug_i8_slices: ") and word in msg, msg


def test_non_finite_rows_behind_rows_are_not_read(built_lib):
    """V's rows >= rows are not part of the operand: a NaN there is no reason to refuse -- and the first refusal after it is the next
    check's, which shows the scan of V passed."""
    import flashpca_amd as fp

    V = np.ones((32, 64))
    V[20:] = np.nan
    rc, msg = _call(fp.lib(), V=V, peers=np.full((1, 64), -1.0))
    assert rc == -1 and "peers" in msg


def test_nsc_pad(built_lib):
    import flashpca_amd as fp

    n = C.c_int(0)
    for S in ALL_S:
        for b in (16, 32, 48, 64):
            got = nsc_pad_of(S, b)
            assert S * b <= got <= 640 and got % 32 == 0, (S, b, got)
    for S, b, word in [(1, 16, "S must be"), (9, 16, "S must be"), (4, 20, "b must be")]:
        assert fp.lib().fpca_debug_i8_nsc_pad(S, b, C.byref(n)) == -1 and word in fp.lib().fpca_last_error().decode()
    assert fp.lib().fpca_debug_i8_nsc_pad(4, 16, None) == -1 and "nsc_pad" in fp.lib().fpca_last_error().decode()
