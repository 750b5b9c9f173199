"""The 512-row (8-wave) instances of the int8 GEMM (csrc/kernels_i8.hip: I8Cfg with WR = 8, i8_tile_rows) at small shapes.

Eight waves share one set of operand tiles; the per-wave code is that of the 4-wave kernel, so the int32 sums are the same numbers and
only the fp64 additions across splits depend on the plan.  FPCA_I8_ROWS=256|512 (test build) forces the tile height wherever an 8-wave
instance exists: the G.M-alone kernel at 3.5 tiles (b 16, S 7) and at 2 tiles (b 16, S 4), band-tiled and row-major.  The children,
the marks, the plan / launch lines, the poison and the references are those of test_gpu_i8_plan.py.

 * Bit-equality across tile heights: the same contexts under FPCA_I8_ROWS=512 and =256, both with FPCA_I8_SPLITS=2 so that the K
   ranges of the partial sums coincide: X'B, X T and X X'B are np.array_equal.  N 2500 x P 2100: X'B has 2304 rows = 4.5 tiles of 512
   (the last one half a tile: waves 4..7 stage, reach the barriers, load no packed words and write nothing) and 10 chunks, X T has 2560
   rows = 5 tiles and 9 chunks (ragged 5 + 4).  Band-tiled and FPCA_I8_TILED=0, missing rates 0 and 0.001 (sparse route: the gather
   plane enters the combine), S 7 and S 4.
 * Plans with a half tile, FPCA_I8_ROWS=512, every output finite under the poison, repeatable, and against the exact integer reference
   / the oracle's dense product at the tolerances of test_gpu_i8_plan.py:
     FPCA_I8_NCU=8, N 4500 x P 4300: X'B rows 4352 = 8.5 tiles, X T rows 4608 = 9 tiles -> 16 tile ids each.
       The plan runs both UNSPLIT (0 + 16 x 1): tile ids come in eights, so with 8 planned CUs every launch is whole rounds and the
       two-phase plan (8 unsplit + the last round split) costs what the unsplit one does plus its planes -- i8_plan never picks it.  (The
       issue expected "8 unsplit, then the half tile split" here; the expectation asserted is what i8_plan computes.  The two-phase
       regime with a half tile in phase B is the FPCA_I8_NCU=16 group below.)
     FPCA_I8_NCU=8 and FPCA_I8_SPLITS=2, N 2700 x P 2700: X'B rows 2816 = 5.5 tiles, plain split-K 0 + 8 x 2 (6 of 12 chunks); X T rows
       3072 = 6 tiles, 11 chunks ragged (6 + 5).  (Without the forced split this launch too is one whole round, unsplit.)
     FPCA_I8_NCU=16, N 2700 x P 8300: X'B rows 8448 = 16.5 tiles -> 24 ids; 16 + 8 x 2 (6), phase B from row 8192 = the half tile alone
       (7 of the 8 phase-B ids idle); also on the sparse route (eplane on both sides of rowB0) and at S 4 (2-tile instance).  X T of the
       same contexts: rows 3072, plain split-K 0 + 8 x 2 (17 of 33 chunks, ragged).
     FPCA_I8_NCU=16, N 8300 x P 2700: X T rows 8704 = 17 tiles -> 24 ids; 16 + 8 x 2 (6 of 11, ragged), phase B from row 8192; band-tiled
       and row-major.
 * Selection: without FPCA_I8_ROWS the one-operand b 16 cases of test_gpu_i8_plan.py (at most 9 / 13 tiles of 512 for 16 / 24 planned
   CUs) keep their `tile 256x...` plans."""
import tempfile

import numpy as np
import pytest

from test_gpu_i8_plan import K2_NCU16, K3_NCU16, NCU24, _check_case, _run, _x

ALL3 = ["xt", "x", "xxt"]


def _tiles(launches, cid, op):
    return [(l["rows"], l["tile"], l["nA"], l["sB"], l["cps"], l["tiled"]) for l in launches[(cid, op)]]


# ---- the same bits at 256 and 512 rows ----
EQ = [dict(id="S%d-miss%g-%s" % (S, miss, "rm" if tiled == 0 else "tiled"), N=2500, P=2100, b=16, S=S, miss=miss, mode=(3 if miss else None), tiled=tiled, ops=ALL3)
      for S in (7, 4) for miss in (0.0, 0.001) for tiled in (None, 0)]


@pytest.mark.gpu
def test_same_bits_at_256_and_512_rows(built_lib):
    with tempfile.TemporaryDirectory() as tmp:
        r256, i256, l256 = _run(EQ, {"FPCA_I8_SPLITS": "2", "FPCA_I8_ROWS": "256"}, tmp, "rows256")
        r512, i512, l512 = _run(EQ, {"FPCA_I8_SPLITS": "2", "FPCA_I8_ROWS": "512"}, tmp, "rows512")
    for case in EQ:
        cid, cols = case["id"], 112 if case["S"] == 7 else 64
        assert i256[cid]["crc"] == i512[cid]["crc"] and i256[cid]["mode"] == i512[cid]["mode"] == (3 if case["miss"] else 2), (i256[cid], i512[cid])
        for op in ALL3:
            a, w = _tiles(l256, cid, op), _tiles(l512, cid, op)
            print(cid, op, w)
            assert len(a) == len(w) == (6 if op == "xxt" else 3), (cid, op, a, w)
            for (rows, tile, nA, sB, cps, tl), (rows2, tile2, nA2, sB2, cps2, tl2) in zip(a, w):
                assert tile == (256, cols) and tile2 == (512, cols), (cid, op, tile, tile2)
                assert rows == rows2 and rows in (2304, 2560) and tl == tl2 == (case["tiled"] is None), (cid, op)
                assert nA == nA2 == 0 and sB == sB2 == 2 and cps == cps2 == 5, (cid, op, a, w)  # the same K ranges
            A, W = r256[cid + "." + op], r512[cid + "." + op]
            assert i512[cid][op + "_finite"] and i512[cid][op + "_repeat"] and i256[cid][op + "_finite"] and i256[cid][op + "_repeat"], (cid, op)
            assert np.isfinite(W).all() and np.max(np.abs(W)) > 0
            assert np.array_equal(A, W), (cid, op, float(np.max(np.abs(A - W))), float(np.max(np.abs(A))))


# ---- plans with a half tile ----
def _w(rows, K, cols, ids, nA, sB, cps, op="x", **kw):
    return _x(rows, K, (512, cols), 1, ids, nA, sB, cps, 4 if cols == 112 else 2, half=cols == 112, op=op, **kw)


# N 4500 x P 4300 at 8 planned CUs: whole rounds, unsplit (module docstring) -- asserted here, the numbers by _check_case
NCU8 = [
    dict(id="w4500S7", N=4500, P=4300, miss=0.0, b=16, S=7, ops=ALL3),
    dict(id="w4500S4", N=4500, P=4300, miss=0.0, b=16, S=4, ops=["x"]),
]
# N 2700 x P 2700, forced plain split-K: the half tile of X'B split, 11 ragged chunks in X T
NCU8_SPLITS2 = [
    dict(id="w2700S7", N=2700, P=2700, miss=0.0, b=16, S=7, ops=ALL3,
         expect=[_w(2816, 3072, 112, 8, 0, 2, 6, op="xt", plain=True, tiled=True), _w(3072, 2816, 112, 8, 0, 2, 6, plain=True, tiled=True)]),
    dict(id="w2700S7rm", N=2700, P=2700, miss=0.0, b=16, S=7, tiled=0, ops=["xt", "x"],
         expect=[_w(2816, 3072, 112, 8, 0, 2, 6, op="xt", plain=True, tiled=False), _w(3072, 2816, 112, 8, 0, 2, 6, plain=True, tiled=False)]),
    dict(id="w2700S4", N=2700, P=2700, miss=0.0, b=16, S=4, ops=["x", "xxt"], expect=[_w(3072, 2816, 64, 8, 0, 2, 6, plain=True, tiled=True)]),
]
# two-phase: the half tile alone in phase B (X'B of N 2700 x P 8300), a full tile there (X T of N 8300 x P 2700)
NCU16 = [
    dict(id="k2halfS7", N=2700, P=8300, miss=0.0, b=16, S=7, ops=ALL3,
         expect=[_w(8448, 3072, 112, 24, 16, 2, 6, op="xt", tiled=True), _w(3072, 8448, 112, 8, 0, 2, 17, plain=True, tiled=True)]),
    dict(id="k2halfS4", N=2700, P=8300, miss=0.0, b=16, S=4, ops=["xt", "x"],
         expect=[_w(8448, 3072, 64, 24, 16, 2, 6, op="xt", tiled=True), _w(3072, 8448, 64, 8, 0, 2, 17, plain=True, tiled=True)]),
    dict(id="k2halfS7sparse", N=2700, P=8300, miss=0.001, mode=3, b=16, S=7, ops=["xt"], expect=[_w(8448, 3072, 112, 24, 16, 2, 6, op="xt", tiled=True)]),
    dict(id="k3S7", N=8300, P=2700, miss=0.0, b=16, S=7, ops=["x", "xxt"], expect=[_w(8704, 2816, 112, 24, 16, 2, 6, tiled=True)]),
    dict(id="k3S7rm", N=8300, P=2700, miss=0.0, b=16, S=7, tiled=0, ops=["x"], expect=[_w(8704, 2816, 112, 24, 16, 2, 6, tiled=False)]),
]


def _group(cases, env):
    with tempfile.TemporaryDirectory() as tmp:
        res, info, launches = _run(cases, dict(env, FPCA_I8_ROWS="512"), tmp, "wide")
    for case in cases:
        _check_case(case, res, info, launches)
    return launches


@pytest.mark.gpu
def test_half_tile_in_whole_rounds(built_lib):
    launches = _group(NCU8, {"FPCA_I8_NCU": "8"})
    for case in NCU8:
        cols = 112 if case["S"] == 7 else 64
        for op in case["ops"]:
            ls = launches[(case["id"], op)]
            assert len(ls) == (6 if op == "xxt" else 3), (case["id"], op, ls)
            for l in ls:
                chunks = {4352: 18, 4608: 17}[l["rows"]]
                assert l["tile"] == (512, cols) and l["ids"] == 16 and l["tiled"] and l["kmode"] == 2 and not l["two"], (case["id"], l)  # 8.5 resp. 9 tiles of 512
                assert (l["nA"], l["nB"], l["sB"], l["cps"], l["chunks"], l["grid"]) == (0, 16, 1, chunks, chunks, 16), (case["id"], l)


@pytest.mark.gpu
def test_half_tile_plain_split_k(built_lib):
    _group(NCU8_SPLITS2, {"FPCA_I8_NCU": "8", "FPCA_I8_SPLITS": "2"})


@pytest.mark.gpu
def test_half_tile_behind_phase_a(built_lib):
    launches = _group(NCU16, {"FPCA_I8_NCU": "16"})
    for l in launches[("k2halfS7", "xt")]:
        assert l["nA"] == 16 and l["rowB0"] == 8192 and l["rows"] - l["rowB0"] == 256, l  # phase B = the half tile


# ---- the selection leaves the small shapes alone ----
@pytest.mark.gpu
@pytest.mark.parametrize("ncu,group", [(16, K3_NCU16 + K2_NCU16), (24, NCU24)], ids=["ncu16", "ncu24"])
def test_small_shapes_keep_their_256_row_tiles(ncu, group, built_lib):
    cases = []
    for c in group:
        e = c["expect"][0]
        if c["b"] == 16 and not e["two"] and e["kmode"] == 2:  # the shapes with an 8-wave instance
            cases.append(dict(c, ops=[e["op"]]))
    assert len(cases) >= (5 if ncu == 16 else 1)
    with tempfile.TemporaryDirectory() as tmp:
        res, info, launches = _run(cases, {"FPCA_I8_NCU": str(ncu)}, tmp, "default")
    for c in cases:
        e = c["expect"][0]
        ls = [l for l in launches[(c["id"], e["op"])] if l["rows"] == e["rows"]]
        assert len(ls) == 3, (c["id"], launches[(c["id"], e["op"])])
        for l in ls:
            assert l["tile"] == tuple(e["tile"]) and l["tile"][0] == 256 and (l["nA"], l["sB"], l["cps"]) == (e["nA"], e["sB"], e["cps"]), (c["id"], l)
