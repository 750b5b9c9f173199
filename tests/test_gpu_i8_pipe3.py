"""The three-buffer main loop of the 8-wave int8 GEMM instances (csrc/kernels_i8.hip: I8Cfg::NBUF = 3 for WR = 8) at small shapes.

With three stage buffers a wave fetches the first operand fragments of chunk c + 1, and decodes its first genotype fragment, BEFORE
the barrier that ends chunk c; chunk c + 2 is staged meanwhile, clamped to the last chunk of the unit.  What can go wrong is the
buffer rotation at the ends of a unit: the prologue (two chunks staged, the second one clamped), the clamped re-stages of the last two
chunks, the dropped fetch behind the last chunk, and the staging-only waves of a half tile, which must hit the same barriers and the
same buffers.  So the units here are 1, 2, 3 and 4-5 chunks long.  The children, the marks, the plan / launch lines, the poison and the
references are those of test_gpu_i8_plan.py; the contexts those of test_gpu_i8_wide.py.

 * Bit-equality with the 4-wave kernel, which keeps two buffers and the code it had: the EQ contexts of test_gpu_i8_wide.py (N 2500 x
   P 2100, b 16, S 7 and S 4, missing 0 and 0.001, band-tiled and FPCA_I8_TILED=0) under FPCA_I8_ROWS=512 and =256 with equal forced
   splits.  X T has 2560 rows = 5 tiles of 512 and 9 chunks, X'B 2304 rows = 4.5 tiles (the last one half a tile: waves 4..7 only
   stage) and 10 chunks.  FPCA_I8_SPLITS -> chunks per unit (X T | X'B):
       9 -> 1 | 2        5 -> 2 (the last unit 1) | 2        3 -> 3 | 4 (the last unit 2)        2 -> 5 (the last unit 4) | 5
   The plan lines must report exactly these `cps` at both heights; X'B, X T and X X'B are np.array_equal.
 * A half tile alone in phase B, split (FPCA_I8_NCU=16, N 2700 x P 8300: X'B rows 8448 = 16.5 tiles -> 16 unsplit + 8 ids x 2 splits of
   6 chunks, 7 of the 8 idle): finite under the poison, repeatable, and equal to the exact integer reference (_check_case).

(The 2-tile 4-wave instance of the eigensolver's cheap passes keeps two buffers: no case for it here.)"""
import tempfile

import numpy as np
import pytest

from test_gpu_i8_plan import _check_case, _run
from test_gpu_i8_wide import ALL3, EQ, NCU16, _tiles

# FPCA_I8_SPLITS -> {rows of the launch: (chunks, chunks per unit, units)}; rows 2560 = X T (K 2304), rows 2304 = X'B (K 2560)
UNITS = {
    9: {2560: (9, 1, 9), 2304: (10, 2, 5)},
    5: {2560: (9, 2, 5), 2304: (10, 2, 5)},
    3: {2560: (9, 3, 3), 2304: (10, 4, 3)},
    2: {2560: (9, 5, 2), 2304: (10, 5, 2)},
}


def test_unit_table():
    """The table itself (no GPU): cps = ceil(chunks / splits), units = ceil(chunks / cps); units of 1, 2, 3 and 4-5 chunks in X T,
    ragged last units of 1, 2 and 4 chunks."""
    for s, by_rows in UNITS.items():
        for rows, (chunks, cps, units) in by_rows.items():
            assert cps == -(-chunks // min(s, chunks)) and units == -(-chunks // cps), (s, rows)
    assert [UNITS[s][2560][1] for s in (9, 5, 3, 2)] == [1, 2, 3, 5]
    assert sorted({chunks - (units - 1) * cps for by_rows in UNITS.values() for chunks, cps, units in by_rows.values()}) == [1, 2, 3, 4, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("splits", sorted(UNITS, reverse=True))
def test_three_buffers_same_bits_as_two(splits, built_lib):
    with tempfile.TemporaryDirectory() as tmp:
        r256, i256, l256 = _run(EQ, {"FPCA_I8_SPLITS": str(splits), "FPCA_I8_ROWS": "256"}, tmp, "rows256")
        r512, i512, l512 = _run(EQ, {"FPCA_I8_SPLITS": str(splits), "FPCA_I8_ROWS": "512"}, tmp, "rows512")
    for case in EQ:
        cid, cols = case["id"], 112 if case["S"] == 7 else 64
        assert i256[cid]["crc"] == i512[cid]["crc"] and i256[cid]["mode"] == i512[cid]["mode"] == (3 if case["miss"] else 2), (i256[cid], i512[cid])
        for op in ALL3:
            a, w = _tiles(l256, cid, op), _tiles(l512, cid, op)
            print(cid, op, w)
            assert len(a) == len(w) == (6 if op == "xxt" else 3), (cid, op, a, w)
            for (rows, tile, nA, sB, cps, tl), (rows2, tile2, nA2, sB2, cps2, tl2) in zip(a, w):
                assert tile == (256, cols) and tile2 == (512, cols), (cid, op, tile, tile2)
                assert rows == rows2 and rows in UNITS[splits] and tl == tl2 == (case["tiled"] is None), (cid, op)
                assert rows == (2560 if op == "x" else 2304) or op == "xxt", (cid, op, rows)
                chunks, want_cps, units = UNITS[splits][rows]
                assert nA == nA2 == 0 and cps == cps2 == want_cps and sB == sB2 == units, (cid, op, a, w)  # the intended units, the same K ranges
            if op == "xxt":
                assert sorted({t[0] for t in w}) == [2304, 2560], (cid, w)
            A, W = r256[cid + "." + op], r512[cid + "." + op]
            assert i512[cid][op + "_finite"] and i512[cid][op + "_repeat"] and i256[cid][op + "_finite"] and i256[cid][op + "_repeat"], (cid, op)
            assert np.isfinite(W).all() and np.max(np.abs(W)) > 0
            assert np.array_equal(A, W), (cid, op, float(np.max(np.abs(A - W))), float(np.max(np.abs(A))))


@pytest.mark.gpu
def test_half_tile_alone_in_phase_b(built_lib):
    cases = [c for c in NCU16 if c["id"] == "k2halfS7"]
    assert len(cases) == 1 and cases[0]["ops"] == ALL3
    with tempfile.TemporaryDirectory() as tmp:
        res, info, launches = _run(cases, {"FPCA_I8_NCU": "16", "FPCA_I8_ROWS": "512"}, tmp, "wide")
    _check_case(cases[0], res, info, launches)
    for l in launches[("k2halfS7", "xt")]:
        assert l["tile"] == (512, 112) and l["nA"] == 16 and l["sB"] == 2 and l["cps"] == 6, l
        assert l["rowB0"] == 8192 and l["rows"] - l["rowB0"] == 256, l  # phase B = the half tile
