"""Exact tests of k_gemm_i8 with the slice-columns on the MFMAs' first operand and the genotypes on the second: the accumulators hold the
TRANSPOSE of a tile of partials, and the epilogue (dump to LDS, recombination by column, lane li writes row li) puts it back.

X'B (apply_xt) and X T (apply_x) must be np.array_equal to the int64 references of tests/i8_planes_yardstick.py, whose data make every
product an exact fp64 number.  What these cases add to tests/test_gpu_i8_planes.py is the property asserted in `_distinct`: inside every
32-row band of a result every (row, column) cell holds a different number (the rows that the statistics zero apart), so a 32 x 32 tile
that comes back transposed, mirrored or rotated, or a half tile of the 16-column remainder that lands in the other row half, cannot pass.

Shapes: 701 samples x 523 SNPs -- X'B has 768 rows, so under FPCA_I8_ROWS=512 the last 512-row tile is half idle -- and 1,100 x 1,300.
b = 16 with S = 7 (3 tiles + the 16-column remainder) and S = 4 (2 tiles), b = 32 with S = 7 (7 tiles); routes 2 (nothing missing), 3 (lists)
and 0 (both matrices, forced); 4-wave tiles and FPCA_I8_ROWS=512; one case under FPCA_I8_SPLITS=4.  Three children (test-hook build: the
knobs are read once per process), each started once, under a time limit of 60 s.

Measured on the MI355X (not asserted): 3 items in 2.6 s -- the 4-wave child 1.0 s, FPCA_I8_ROWS=512 0.9 s, FPCA_I8_SPLITS=4 0.3 s; every
comparison passed.
"""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8_planes_yardstick as PY  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((PY.N, PY.P), (1100, 1300))
WIDTHS = ((16, 7), (16, 4), (32, 7))
ROUTES = (("D0", None, 2), ("D1", None, 3), ("D1", 0, 0))  # data set, forced mode, the route it must take


def _runs(child):
    if child == "splits4":
        return [dict(ds="D0", mode=None, want=2, b=16, S=7, n=1100, p=1300)]
    return [dict(ds=ds, mode=mode, want=want, b=b, S=S, n=n, p=p) for n, p in SHAPES for ds, mode, want in ROUTES for b, S in WIDTHS]


CHILD_ENV = {"waves4": {}, "rows512": {"FPCA_I8_ROWS": "512"}, "splits4": {"FPCA_I8_SPLITS": "4"}}


def _rid(r):
    return "%s-m%s-b%d-S%d-%dx%d" % (r["ds"], "d" if r["mode"] is None else r["mode"], r["b"], r["S"], r["n"], r["p"])


_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import flashpca_amd as fp
import i8_planes_yardstick as PY
runs = json.loads(sys.argv[2])
out, modes = {}, {}
with fp.test_hooks():
    ctx, ckey = None, None
    try:
        for r in runs:
            ds, S, b, n, P = r["ds"], r["S"], r["b"], r["n"], r["p"]
            if (ds, S, n) != ckey:
                if ctx is not None:
                    ctx.close()
                os.environ.pop("FPCA_I8_MODE", None)
                ctx = fp.Context.from_packed(PY.pack(PY.genotypes(ds, n, P)), n, P, stand="binom", accum="i8x%d" % S)
                ckey = (ds, S, n)
            if r["mode"] is None:
                os.environ.pop("FPCA_I8_MODE", None)
            else:
                os.environ["FPCA_I8_MODE"] = str(r["mode"])
            modes[r["rid"]] = ctx.missing_mode(b)
            for op, f in (("xt", ctx.apply_xt), ("x", ctx.apply_x)):
                out[r["rid"] + "." + op] = f(PY.host_block(ds, PY.case_operand(ds, S, b, op, 0, n, P), op, n, P))
    finally:
        if ctx is not None:
            ctx.close()
np.savez(sys.argv[3], **out)
print("CHILD " + json.dumps(modes))
"""

_DONE = {}


def _child(name):
    """Child `name`, started once per session whatever became of it."""
    if name not in _DONE:
        env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
        env.update(CHILD_ENV[name])
        env["FPCA_DEBUG_I8_POISON"] = "1"
        runs = [dict(r, rid=_rid(r)) for r in _runs(name)]
        try:
            with tempfile.TemporaryDirectory() as tmp:
                out = os.path.join(tmp, name + ".npz")
                r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(runs), out], capture_output=True, text=True, env=env, timeout=60)
                if r.returncode != 0:
                    raise AssertionError("child %s ended with status %d: %s" % (name, r.returncode, r.stdout[-2000:] + r.stderr[-3000:]))
                modes = json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
                _DONE[name] = (dict(np.load(out)), modes)
        except Exception as e:
            _DONE[name] = AssertionError("child %s: %r" % (name, e))
    if isinstance(_DONE[name], Exception):
        raise _DONE[name]
    return _DONE[name]


@functools.lru_cache(maxsize=None)
def _reference(ds, S, b, op, n, p):
    ref = PY.reference(ds, PY.case_operand(ds, S, b, op, 0, n, p), op, n, p)
    ref.setflags(write=False)
    return ref


def _distinct(ref, ds, op, n, p):
    """Every cell of a 32-row band differs from every other one of the band (all b columns: for b = 16 that covers both 16-row halves of the
    remainder tile and both 16-column halves of a full tile).  X'B: the row of the SNP whose sd is zero is zero by its statistics, and the
    yardstick's two pin SNPs (X T: its two pin samples) hold the same genotypes, so the second repeats its neighbour's row and is left out."""
    live = PY.live_snps(PY.meansd(ds, n, p)) if op == "xt" else np.ones(ref.shape[0], dtype=bool)
    live[(PY.PIN_SNP if op == "xt" else PY.PIN_SAMPLE) + 1] = False
    for r0 in range(0, ref.shape[0], 32):
        band = ref[r0:r0 + 32][live[r0:r0 + 32]]
        assert np.unique(band).size == band.size, (op, r0)
    assert int((~live).sum()) <= 2


def _check(name):
    res, modes = _child(name)
    for r in _runs(name):
        rid = _rid(r)
        ds, S, b, n, p = r["ds"], r["S"], r["b"], r["n"], r["p"]
        assert modes[rid] == r["want"], (rid, modes[rid])
        if r["mode"] is None:
            GM, M = PY.dosage_called(PY.genotypes(ds, n, p))
            assert PY.route((M == 0).sum(axis=1), n, S, b) == r["want"], rid
        for op in ("xt", "x"):
            ref = _reference(ds, S, b, op, n, p)
            _distinct(ref, ds, op, n, p)
            R = res[rid + "." + op]
            assert R.shape == ref.shape and np.isfinite(R).all(), (rid, op)  # the poison: an unwritten partial is a NaN
            bad = np.argwhere(R != ref)
            assert np.array_equal(R, ref), (name, rid, op, "%d of %d cells differ, first %s" % (len(bad), R.size, bad[:4].tolist()))


def test_four_wave_tiles(built_lib):
    """The default plan: 256-row workgroups, routes 2, 3 and 0, both shapes."""
    _check("waves4")


def test_eight_wave_tiles(built_lib):
    """FPCA_I8_ROWS=512: 768 rows are one and a half tiles (the second half of the last one is idle), 1,280 and 1,536 two and a half and three."""
    _check("rows512")


def test_one_chunk_partial_planes(built_lib):
    """FPCA_I8_SPLITS=4: the partial planes beyond plane 0 are written by the same epilogue."""
    _check("splits4")
