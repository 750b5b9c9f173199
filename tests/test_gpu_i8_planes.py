"""Exact tests of the int8 GEMM (csrc/kernels_i8.hip: k_slice -> k_gemm_i8 -> k_i8_combine, and the missing-call routes of
csrc/missing_routes.hip around them) that reach every digit plane and every kernel instance.

The earlier exact checks multiply integer blocks in [-4, 4], which have digits in the top plane only, and every other comparison allows
1e-11 of the column maximum -- wider than planes 5, 6, 7 at S = 7 / 8 (tests/test_i8_planes_cpu.py shows both).  Here the operands live
in the low planes on purpose and every product is an exact fp64 number (tests/i8_planes_yardstick.py: genotypes of mean 1, sd 1/2 exactly;
full-random operands up to S = 5, digit windows with a cancelling pin pair from S = 6; int64 references), so EVERY comparison is
np.array_equal: X'B (apply_xt) and X T (apply_x), S = 2 .. 8, 16 / 32 / 48 / 64 columns, on
  D0 route 2 (nothing missing) | D1 routes 3 (lists; 16 / 32 / 64 columns), 0 and 1 (forced) | D2 route 4 (hybrid; 16 / 32 / 64 columns) |
  D3 mode 0 with per-SNP dyadic mean / sd (fpca_set_meansd),
each with the band-tiled copies and with FPCA_I8_TILED=0.  fpca_missing_mode is asserted for every case; every output is finite under
FPCA_DEBUG_I8_POISON and unchanged when its operand is applied again after a different one (the other block of the window rotation, itself
compared).  The one documented approximation of the path -- fp32 rows for the gathers at S <= 4, which hold 24 significant bits -- is
respected by the data, not by a tolerance: on the list routes the operands are full ones of 13 bits at S = 2 and 21 bits at S = 3, and
three-plane windows of 21-bit entries at S = 4 (the pins are powers of two).

Children (test-hook build; the knobs are read once per process), one pytest item each, started once whatever becomes of it (a failed
start is remembered and raised again, never repeated -- the census included), under a time limit of 60 s:
  main2 .. main8   the default plan at S slices: all of the above (44 runs x 2 products x 3 applies)
  splits4          FPCA_I8_SPLITS=4: partial planes of ONE chunk each; S 3 / 7 / 8, b 16 / 64, routes 2 and 0
  rows512          FPCA_I8_ROWS=512: the 8-wave instances; (b 16, S 4), (b 16, S 7), (b 32, S 2), routes 2 and 3, both layouts
  ncu24            FPCA_I8_NCU=24 on 2301 samples x 2099 SNPs: phase A non-empty, phase B split in two; S 7, b 16 / 32 / 64, routes 2 and 0
                   (at 523 SNPs X T has three K chunks, and i8_plan splits only into parts of four chunks or more.  With 8 CUs every count
                   of tile ids is a whole number of rounds: i8_plan then offers a phase B of the last 8 tiles, nA = ids - 8, but s
                   splits of it are s whole rounds, which never beat the one unsplit round, and the tie with nA = 0 does not pass its
                   0.995 rule -- so FPCA_I8_NCU=8 never yields a split phase B, at any shape)
Census: the key (two operands, mode, nt, half tile, tile rows, band-tiled) of every launch is rebuilt from the FPCA_I8_VERBOSE log (parser
of tests/test_gpu_i8_plan.py); the union over the children must hold every tuple of fpca_debug_i8_instances -- an instance of I8Instances
that no case launches fails test_census by name.

Measured on the MI355X (profiles/i8_planes_test_figures.txt; not asserted): 11 items in 9.1 s -- main2 .. main8 0.8 - 1.1 s each (0.4 - 0.6 s
inside the child, the rest its start and the parent's references), splits4 0.5 s, rows512 0.6 s, ncu24 1.3 s; 51 of 51 instances launched.
Every comparison passed: no defect of k_gemm_i8 or k_i8_combine in the low planes was found.  (A library whose epilogue drops plane 6 of
a 32-column block passes test_gpu_i8_plan / _tiled / _wide / _pipe3 and fails test_default_plan[7] here: same file.)"""
import functools
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import i8_planes_yardstick as PY  # noqa: E402
from test_gpu_i8_plan import _launches  # noqa: E402  (the plan / launch line parser)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import flashpca_amd as fp
import i8_planes_yardstick as PY
runs = PY.child_runs(sys.argv[2])
out, info = {}, {}

def mark(s):
    sys.stderr.write("MARK " + s + "\n")
    sys.stderr.flush()

def setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = str(v)

t0 = time.time()
with fp.test_hooks():
    ctx, ckey = None, None
    try:
        for r in runs:
            ds, S, b = r["ds"], r["S"], r["b"]
            n, P = PY.dims(r["tall"])
            key = (ds, S, r["tiled"], n)
            if key != ckey:  # (FPCA_I8_TILED is read per context, FPCA_I8_MODE on every call)
                if ctx is not None:
                    ctx.close()
                setenv("FPCA_I8_TILED", r["tiled"])
                setenv("FPCA_I8_MODE", None)
                ctx = fp.Context.from_packed(PY.pack(PY.genotypes(ds, n, P)), n, P, stand="binom", accum="i8x%d" % S)
                if ds == "D3":
                    ctx.set_meansd(PY.meansd("D3", n, P))
                ckey = key
            setenv("FPCA_I8_MODE", r["mode"])
            rid = PY.run_id(r)
            i = {"mode": ctx.missing_mode(b)}
            for op, f in (("xt", ctx.apply_xt), ("x", ctx.apply_x)):
                A0, A1 = (PY.host_block(ds, PY.case_operand(ds, S, b, op, k, n, P), op, n, P) for k in (0, 1))
                mark(rid + " " + op)
                R1 = f(A0)
                R2 = f(A1)
                R3 = f(A0)
                out[rid + "." + op + ".0"], out[rid + "." + op + ".1"] = R1, R2
                i[op + "_repeat"] = bool(np.array_equal(R1, R3))
            mark(rid + " end")
            info[rid] = i
    finally:
        if ctx is not None:
            ctx.close()
info["seconds"] = time.time() - t0
np.savez(sys.argv[3], **out)
print("CHILD " + json.dumps(info))
"""

_DONE = {}
CHILD_TIMEOUT = 60  # seconds; a child runs for about one (module docstring)


class ChildFailed(AssertionError):
    pass


def _start(name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    env.update(PY.CHILD_ENV.get(name, {}))
    env.update({"FPCA_I8_VERBOSE": "1", "FPCA_DEBUG_I8_POISON": "1"})
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, name + ".npz")
        t0 = time.time()
        try:
            r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, out], capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            raise ChildFailed("child %s did not finish within %d s: %s" % (name, CHILD_TIMEOUT, str(e.stderr or "")[-2000:]))
        secs = time.time() - t0
        if r.returncode != 0:
            raise ChildFailed("child %s ended with status %d: %s" % (name, r.returncode, r.stdout[-2000:] + r.stderr[-3000:]))
        info = json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
        return dict(np.load(out)), info, _launches(r.stderr), secs


def _child(name):
    """Child `name`, started ONCE per session whatever became of it: (results, info, launches, seconds of the whole process), or the
    failure of its one start raised again -- a child that faulted, aborted or ran into its time limit is never started a second time, by
    its own item or by the census."""
    if name not in _DONE:
        try:
            _DONE[name] = _start(name)
        except Exception as e:  # (a truncated log or result file too)
            _DONE[name] = e if isinstance(e, ChildFailed) else ChildFailed("child %s: %r" % (name, e))
    if isinstance(_DONE[name], Exception):
        raise _DONE[name]
    return _DONE[name]


@functools.lru_cache(maxsize=None)
def _reference(ds, S, b, op, block, tall):
    n, P = PY.dims(tall)
    ref = PY.reference(ds, PY.case_operand(ds, S, b, op, block, n, P), op, n, P)
    ref.setflags(write=False)
    return ref


def _key(l):
    """The I8Key of a launch: the launch line gives operands, mode, nt, half and layout, the plan line the tile rows."""
    return (l["two"], l["kmode"], l["nt"], l["half"], l["tile"][0], l["tiled"])


def _explain(R, ref, o):
    """Where an output differs, in units of the column's lowest digit: which planes' weight the error has."""
    bad = np.argwhere(R != ref)
    i, c = bad[0]
    with np.errstate(invalid="ignore"):
        d = (R[i, c] - ref[i, c]) / 2.0 ** float(o.unit[c] - 2)
    return "%d of %d entries differ, columns %s; first (%d, %d): got %r want %r, difference %r quarter units (lowest digit %d of S %d)" % (
        len(bad), R.size, sorted(set(bad[:, 1].tolist()))[:8], i, c, R[i, c], ref[i, c], d, int(o.digit0[c]), o.S)


def _check_child(name):
    res, info, launches, secs = _child(name)
    runs = PY.child_runs(name)
    keys = set()
    for r in runs:
        rid = PY.run_id(r)
        n, P = PY.dims(r["tall"])
        assert info[rid]["mode"] == PY.expected_mode(r), (rid, info[rid])
        for op in ("xt", "x"):
            ls = launches[(rid, op)]
            assert len(ls) >= 3, (rid, op, ls)  # one GEMM per apply at least (the hybrid route: the dense SNPs' indicator GEMM too)
            keys |= {_key(l) for l in ls}
            want_two = op == "x" and info[rid]["mode"] in (0, 1)
            want_kmode = info[rid]["mode"] if info[rid]["mode"] in (0, 1) else 2
            assert all(l["two"] == want_two and l["kmode"] == want_kmode for l in ls), (rid, op, ls)
            assert all(l["tiled"] is False for l in ls) or r["tiled"] is None, (rid, op)
            assert info[rid][op + "_repeat"], (rid, op)  # the same operand again after another one: the same bits
            for block in (0, 1):
                R = res["%s.%s.%d" % (rid, op, block)]
                ref = _reference(r["ds"], r["S"], r["b"], op, block, r["tall"])
                assert R.shape == ref.shape and np.isfinite(R).all(), (rid, op, block)  # the poison: an unwritten plane is a NaN
                assert np.array_equal(R, ref), (name, rid, op, block, sorted(_key(l) for l in ls),
                                                _explain(R, ref, PY.case_operand(r["ds"], r["S"], r["b"], op, block, n, P)))
    print("i8 planes child %s: %d runs x 2 products x 3 applies, %d instances, %.1f s in the child, %.1f s with its start" % (
        name, len(runs), len(keys), info["seconds"], secs))
    for k in sorted(keys):
        print("   instance two=%d mode=%d nt=%d half=%d rows=%d tiled=%d" % tuple(int(v) for v in k))
    return launches


@pytest.mark.parametrize("S", range(2, 9))
def test_default_plan(built_lib, S):
    """All four widths on routes 2, 3, 0, 1, 4 and the two-matrix kernels with dyadic statistics, both layouts, at S slices."""
    _check_child("main%d" % S)


def test_one_chunk_partial_planes(built_lib):
    """FPCA_I8_SPLITS=4: every split is one chunk (X'B: 4 chunks, 4 planes; X T: 3 chunks, 3 planes)."""
    launches = _check_child("splits4")
    ls = [l for v in launches.values() for l in v]
    assert ls and all(l["nA"] == 0 and l["cps"] == 1 and l["sB"] == l["chunks"] and l["sB"] in (3, 4) for l in ls), ls
    assert {l["sB"] for l in ls} == {3, 4}


def test_eight_wave_instances(built_lib):
    """FPCA_I8_ROWS=512: the 512-row workgroups, 2 tiles and 3.5 tiles, both layouts, routes 2 and 3."""
    launches = _check_child("rows512")
    ls = [l for v in launches.values() for l in v]
    assert {(l["nt"], l["half"], l["tiled"]) for l in ls if l["tile"][0] == 512} == {(2, False, False), (2, False, True), (4, True, False), (4, True, True)}


def test_two_phase(built_lib):
    """FPCA_I8_NCU=24 on 2301 x 2099: with two column blocks (one operand b 64, two operands b 32) there are 32 tile ids -- 24 run unsplit
    (phase A), 8 are split in two along K from row 2048 on (phase B); nA / 8 = 3 is odd, so row tiles 8 and 9 have one column block in each
    phase.  X'B b 64, X T b 64 (G.M alone) and X T b 32 (both matrices)."""
    launches = _check_child("ncu24")
    ls = [l for v in launches.values() for l in v]
    two_phase = [l for l in ls if l["nA"] > 0 and l["sB"] >= 2 and 0 < l["rowB0"] < l["rows"]]
    assert {(l["two"], l["rows"]) for l in two_phase} == {(False, 2304), (False, 2560), (True, 2560)}, ls
    assert all((l["ids"], l["nA"], l["sB"], l["cps"], l["rowB0"], l["zb"]) == (32, 24, 2, 5, 2048, 2) for l in two_phase), two_phase
    print("i8 planes two-phase launches:", sorted({(_key(l), l["nA"], l["sB"], l["rowB0"]) for l in two_phase}))


def test_census(built_lib):
    """Every member of I8Instances is launched by some case above (each of which is compared exactly)."""
    import flashpca_amd as fp

    table = fp.api.debug_i8_instances()
    assert len(table) == len(set(table)) == 51
    reached = set()
    failed = [name for name in PY.CHILDREN if isinstance(_DONE.get(name), Exception)]
    assert not failed, "no census: children %s did not complete (their own items say why); nothing is started again" % failed
    for name in PY.CHILDREN:
        launches = _child(name)[2]  # (run alone, the census starts the children itself -- each once, and none after a failure)
        reached |= {_key(l) for v in launches.values() for l in v}
    missing = [k for k in table if k not in reached]
    assert not missing, "instances (two operands, mode, nt, half, rows, tiled) no case launches: %s" % missing
    assert reached <= set(table), sorted(reached - set(table))
    print("i8 planes census: %d of %d instances launched" % (len(reached & set(table)), len(table)))
