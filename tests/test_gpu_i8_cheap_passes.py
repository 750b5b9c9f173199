"""Exact tests of the passes the eigensolver makes on FEWER slices than its context holds (fpca_ctx::i8_Sc: the cheap passes, nine block
applies in ten of a long solve), and of the chained product X X' B it runs them through.

That state is reachable through fpca_pca alone, where a wrong cheap pass costs convergence and never an assertion (solver.cpp verifies
every Ritz block through the exact operator).  Every other exact int8 test makes its context with accum="i8x<S>" and multiplies on S
slices: what exists for i8_Sc < i8_S only -- Q buffers sized for S and read over gemm_i8_nsc_pad(Sc, b) rows, the pad rows' and the
workspace's keys in ensure_i8 / ensure_hybrid, the route that changes per pass (i8_mode: the two-matrix kernels for a pass on at most 4
slices between the two break-evens), the gathers' one operand buffer holding fp32 rows in one pass and fp64 rows in the next -- was
compared with nothing.  Here fpca_debug_set_pass_slices (test-hook build) sets the very field HipBackend::set_cheap sets, and
tests/i8_planes_yardstick.py supplies the operands of tests/test_gpu_i8_planes.py made for Sc slices: exact at Sc, so EVERY comparison is
np.array_equal with an int64 reference that does not know the context's slice count.

  cheap7           one context of 7 slices per data set and layout (band-tiled copies; FPCA_I8_TILED=0) runs a whole schedule of passes
  cheap8, cheap6   the same in contexts of 8 and 6 slices, default layout
                   D0 route 2 | D1 route 3 | D2 route 4 | D3 two-matrix kernels, mode 0, dyadic mean / sd | D4 (0.424 % missing: between
                   the break-evens) route 3 on 5 slices and more, the two-matrix kernels on 4 and fewer; 16 / 32 / 48 / 64 columns (48 not
                   on the list routes).  Default layout: the pass is the outer loop, the width the inner one; FPCA_I8_TILED=0: the other
                   way round, shortened.  tests/test_i8_planes_cpu.py holds every context's sequence to the transitions that matter: exact
                   <-> cheap, <= 4 slices <-> 5 / 6 (fp32 <-> fp64 gather rows), two different (Sc, b) of one Sc b, a ragged Sc b after a
                   larger one, a width change alone, first and last run exact.
                   Per run and product X'B / X T: both blocks of the window rotation equal their references, everything finite under
                   FPCA_DEBUG_I8_POISON, block 0 again after block 1 gives the same bits, the launch lines show the kernels of
                   pass_route(...) (D4: two operands on <= 4 slices, G.M alone from 5; D1: G.M alone always), and fpca_missing_mode goes
                   on reporting the exact passes' route.  After a context's last run its first operand is applied once more: the same bits.
                   THE WITNESS (D0, D1, D2, D4) shows that the pass ran on Sc slices and no other count -- operands exact at Sc are exact
                   at S too, a hook that did nothing would pass all of the above: block 0 with a quarter of the Sc quantum in a few entries
                   must give block 0's bits when Sc < S (on S slices the quarter is a digit); on an exact pass block 0 on a grid three bits
                   finer must equal ITS reference and not block 0's.  (D3's second operand x k / 4 breaks that grid: no witness.)
  chain7           fpca_apply_xxt = apply_xxt_dev -> xt_i8(chain) -> x_i8(have_max), what the solver runs: the K2 combine leaves the column
                   maxima of the two K3 operands, which are cut on the pass's slices and DO round on 4 and 3.  Context of 7 slices, passes
                   7, 4, 7, 3, 7 on D0, D1, D2, D4, b 16 / 32 / 64, three applies (B0, B1, B0) each.  The reference restates the path in
                   int64 (yardstick, `chain_model`): T = X'B exact, T / sd and mean T / sd cut by the slicer's model with the exponents of
                   their own maxima, the gathered rows through fp32 at <= 4 slices -- the documented approximation, modelled, not
                   tolerated.  Mean 1, sd 1/2 make the two K3 operands equal: WHICH maximum the combine leaves for which operand cannot
                   show here (it would take per-SNP means, whose chain has no exact model yet).
Children as in tests/test_gpu_i8_planes.py: test-hook build, FPCA_I8_VERBOSE=1 and FPCA_DEBUG_I8_POISON=1, one after another, each started
ONCE per session whatever becomes of it (a failed start is remembered and raised again, never repeated), 60 s limit.
The hook itself: refuses Sc = 1, Sc = S, an fp64 and a dense context; in the product build it returns FPCA_EINVAL and changes nothing;
fpca_pca clears the setting.

Measured on the MI355X: profiles/i8_cheap_pass_test_figures.txt (seconds per item and child; not asserted)."""
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
from test_gpu_i8_planes import CHILD_TIMEOUT, ROOT, ChildFailed, _explain, _key  # noqa: E402

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import flashpca_amd as fp
import i8_planes_yardstick as PY
chain = sys.argv[2] == "chain7"
runs = PY.chain_runs() if chain else PY.cheap_runs(sys.argv[2])
out, info = {}, {"last": {}}

def mark(s):
    sys.stderr.write("MARK " + s + "\n")
    sys.stderr.flush()

def setenv(k, v):
    if v is None:
        os.environ.pop(k, None)
    else:
        os.environ[k] = str(v)

def again(ctx, ckey, first):  # after the last run of a context: an exact apply of its first operand once more
    ctx.debug_pass_slices(0)
    mark("%s-%s-last all" % ckey)
    info["last"]["%s-%s" % ckey] = {op: bool(np.array_equal(f(A), R)) for op, (f, A, R) in first.items()}

t0 = time.time()
with fp.test_hooks():
    ctx, ckey, first = None, None, {}
    try:
        for r in runs:
            ds, S, Sc, b = r["ds"], r["S"], r["Sc"], r["b"]
            n, P = PY.dims(r["tall"])
            key = (ds, "tl" if r["tiled"] is None else "rm")
            if key != ckey:  # (FPCA_I8_TILED is read per context, FPCA_I8_MODE on every call)
                if ctx is not None:
                    again(ctx, ckey, first)
                    ctx.close()
                setenv("FPCA_I8_TILED", r["tiled"])
                setenv("FPCA_I8_MODE", None)
                ctx = fp.Context.from_packed(PY.pack(PY.genotypes(ds, n, P)), n, P, stand="binom", accum="i8x%d" % S)
                if ds == "D3":
                    ctx.set_meansd(PY.meansd("D3", n, P))
                ckey, first = key, {}
            setenv("FPCA_I8_MODE", r["mode"])
            rid = PY.pass_run_id(r)
            ctx.debug_pass_slices(0 if Sc == S else Sc)
            i = {"mode": ctx.missing_mode(b)}
            if chain:
                B0, B1 = (PY.chain_block(ds, b, k, n, P).x for k in (0, 1))
                mark(rid + " xxt")
                R1 = ctx.apply_xxt(B0)
                R2 = ctx.apply_xxt(B1)
                R3 = ctx.apply_xxt(B0)
                out[rid + ".xxt.0"], out[rid + ".xxt.1"] = R1, R2
                i["xxt_repeat"] = bool(np.array_equal(R1, R3))
                first.setdefault("xxt", (ctx.apply_xxt, B0, R1))
            else:
                for op, f in (("xt", ctx.apply_xt), ("x", ctx.apply_x)):
                    A0, A1 = (PY.host_block(ds, PY.case_operand(ds, Sc, b, op, k, n, P), op, n, P) for k in (0, 1))
                    mark(rid + " " + op)
                    R1 = f(A0)
                    R2 = f(A1)
                    R3 = f(A0)
                    out[rid + "." + op + ".0"], out[rid + "." + op + ".1"] = R1, R2
                    i[op + "_repeat"] = bool(np.array_equal(R1, R3))
                    if ds in PY.WITNESS_SETS:
                        RW = f(PY.host_block(ds, PY.witness_operand(ds, S, Sc, b, op, n, P), op, n, P))
                        i[op + "_witness_is_block0"] = bool(np.array_equal(RW, R1))
                        i[op + "_witness_finite"] = bool(np.isfinite(RW).all())
                        if Sc == S:
                            out[rid + "." + op + ".w"] = RW
                    first.setdefault(op, (f, A0, R1))
            i["mode_after"] = ctx.missing_mode(b)
            mark(rid + " end")
            info[rid] = i
        if ctx is not None:
            again(ctx, ckey, first)
    finally:
        if ctx is not None:
            ctx.close()
info["seconds"] = time.time() - t0
np.savez(sys.argv[3], **out)
print("CHILD " + json.dumps(info))
"""

_DONE = {}
CHILDREN = sorted(PY.CHEAP_CHILDREN) + ["chain7"]


def _start(name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
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
    """Child `name`, started ONCE per session whatever became of it: its results, or the failure of its one start raised again."""
    if name not in _DONE:
        try:
            _DONE[name] = _start(name)
        except Exception as e:  # (a truncated log or result file too)
            _DONE[name] = e if isinstance(e, ChildFailed) else ChildFailed("child %s: %r" % (name, e))
    if isinstance(_DONE[name], Exception):
        raise _DONE[name]
    return _DONE[name]


@functools.lru_cache(maxsize=None)
def _reference(ds, Sc, b, op, block):
    ref = PY.reference(ds, PY.case_operand(ds, Sc, b, op, block), op)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _chain_reference(ds, Sc, b, block):
    ref = PY.chain_model(ds, PY.chain_block(ds, b, block), PY.CHAIN_S, Sc).Y
    ref.setflags(write=False)
    return ref


def _want_kernels(cur, op):
    """(two operands, the kernels' mode) of the GEMMs of a pass on route `cur`."""
    return op == "x" and cur in (0, 1), cur if cur in (0, 1) else 2


def _contexts(runs):
    return sorted({"%s-%s" % (r["ds"], "tl" if r["tiled"] is None else "rm") for r in runs})


def _check_cheap(name):
    res, info, launches, secs = _child(name)
    runs = PY.cheap_runs(name)
    keys, d4 = set(), set()
    for r in runs:
        rid, ds, S, Sc, b = PY.pass_run_id(r), r["ds"], r["S"], r["Sc"], r["b"]
        ctx_mode, cur = PY.expected_pass_modes(r)
        assert info[rid]["mode"] == ctx_mode == info[rid]["mode_after"], (rid, info[rid])  # the exact passes' route, throughout
        for op in ("xt", "x"):
            ls = launches[(rid, op)]
            witness = ds in PY.WITNESS_SETS
            assert len(ls) >= (4 if witness else 3), (rid, op, ls)  # one GEMM per apply at least
            keys |= {_key(l) for l in ls}
            two, kmode = _want_kernels(cur, op)
            assert all(l["two"] == two and l["kmode"] == kmode for l in ls), (rid, op, cur, ls)
            assert all(l["tiled"] is False for l in ls) or r["tiled"] is None, (rid, op)
            if ds == "D4":
                d4 |= {(Sc <= 4, op, l["two"], l["kmode"]) for l in ls}
            assert info[rid][op + "_repeat"], (rid, op)  # the same operand again after another one: the same bits
            for block in (0, 1):
                R = res["%s.%s.%d" % (rid, op, block)]
                ref = _reference(ds, Sc, b, op, block)
                assert R.shape == ref.shape and np.isfinite(R).all(), (rid, op, block)  # the poison: an unwritten plane is a NaN
                assert np.array_equal(R, ref), (name, rid, op, block, sorted(_key(l) for l in ls), _explain(R, ref, PY.case_operand(ds, Sc, b, op, block)))
            if not witness:
                continue
            assert info[rid][op + "_witness_finite"], (rid, op)
            if Sc < S:  # the quarter of the Sc quantum rounds away on Sc slices -- and on no larger count
                assert info[rid][op + "_witness_is_block0"], (name, rid, op, "the pass did not run on %d slices" % Sc)
            else:
                w = PY.witness_operand(ds, S, Sc, b, op)
                RW, ref = res["%s.%s.w" % (rid, op)], PY.reference(ds, w, op)
                assert np.array_equal(RW, ref), (name, rid, op, "witness", _explain(RW, ref, w))
                assert not info[rid][op + "_witness_is_block0"], (rid, op)
    # D4 lies between the break-evens: the two-matrix kernels on <= 4 slices, G.M alone (and the gathers) from 5 on
    assert d4 == {(True, "xt", False, 0), (True, "x", True, 0), (False, "xt", False, 2), (False, "x", False, 2)}, d4
    assert sorted(info["last"]) == _contexts(runs) and all(v == {"xt": True, "x": True} for v in info["last"].values()), info["last"]
    print("i8 cheap passes child %s: %d runs x 2 products x 3 applies (+ witness), %d contexts, %d instances, %.1f s in the child, %.1f s with its start" % (
        name, len(runs), len(info["last"]), len(keys), info["seconds"], secs))


@pytest.mark.parametrize("name", sorted(PY.CHEAP_CHILDREN))
def test_passes_on_fewer_slices(built_lib, name):
    """A whole schedule of exact and cheap passes in one context per data set and layout: every product exact, the witness, the kernels."""
    _check_cheap(name)


def test_chained_product(built_lib):
    """fpca_apply_xxt on 7, 4, 7, 3, 7 slices in one context of 7 against the int64 model of the chain."""
    res, info, launches, secs = _child("chain7")
    runs = PY.chain_runs()
    n_pad, p_pad = 1024, 768
    differ = set()
    for r in runs:
        rid, ds, Sc, b = PY.pass_run_id(r), r["ds"], r["Sc"], r["b"]
        ctx_mode, cur = PY.expected_pass_modes(r)
        assert info[rid]["mode"] == ctx_mode == info[rid]["mode_after"], (rid, info[rid])
        ls = launches[(rid, "xxt")]
        k2 = [l for l in ls if (l["rows"], l["K"]) == (p_pad, n_pad)]
        k3 = [l for l in ls if (l["rows"], l["K"]) == (n_pad, p_pad)]
        assert len(k2) == 3 and len(k3) == 3, (rid, ls)
        for op, group in (("xt", k2), ("x", k3)):
            two, kmode = _want_kernels(cur, op)
            assert all(l["two"] == two and l["kmode"] == kmode for l in group), (rid, op, cur, group)
        assert all(l["two"] is False and l["kmode"] == 2 for l in ls if l not in k2 and l not in k3), (rid, ls)  # the hybrid route's small GEMMs
        assert info[rid]["xxt_repeat"], rid
        for block in (0, 1):
            R, ref = res["%s.xxt.%d" % (rid, block)], _chain_reference(ds, Sc, b, block)
            assert R.shape == ref.shape and np.isfinite(R).all(), (rid, block)
            bad = np.argwhere(R != ref)
            assert not len(bad), ("chain7", rid, block, "%d of %d entries differ, columns %s; first %s: got %r want %r" % (
                len(bad), R.size, sorted(set(bad[:, 1].tolist()))[:8], tuple(bad[0]), R[tuple(bad[0])], ref[tuple(bad[0])]))
            if Sc < PY.CHAIN_S:
                differ.add((ds, Sc, b, bool((ref != _chain_reference(ds, PY.CHAIN_S, b, block)).mean() > 0.5)))
    assert differ and all(d[3] for d in differ)  # (what a pass on 7 slices would have given is another matrix: test_i8_planes_cpu.py)
    assert sorted(info["last"]) == _contexts(runs) and all(v == {"xxt": True} for v in info["last"].values()), info["last"]
    print("i8 cheap passes child chain7: %d runs x 3 applies, %.1f s in the child, %.1f s with its start" % (len(runs), info["seconds"], secs))


# ---- the hook itself -------------------------------------------------------------------------------------------------------------------
def _ctx(fp, ds, accum):
    return fp.Context.from_packed(PY.pack(PY.genotypes(ds)), PY.N, PY.P, stand="binom", accum=accum)


def test_hook_refusals(built_lib):
    import flashpca_amd as fp

    with fp.test_hooks() as L:
        with _ctx(fp, "D0", "i8x7") as ctx:
            for Sc, ok in ((1, False), (7, False), (8, False), (-1, False), (2, True), (6, True), (0, True)):
                rc = L.fpca_debug_set_pass_slices(ctx.h, Sc)
                assert (rc == 0) == ok, (Sc, rc)
                assert ok or (rc == -1 and b"Sc must be" in L.fpca_last_error())
        with _ctx(fp, "D0", "fp64") as ctx:
            assert L.fpca_debug_set_pass_slices(ctx.h, 4) == -1 and b"exact-integer" in L.fpca_last_error()
            assert L.fpca_debug_set_pass_slices(ctx.h, 0) == -1
        X = np.random.default_rng(1).integers(0, 3, size=(64, 48)).astype(np.float64)
        with fp.Context.from_dense(X, stand="binom") as ctx:
            assert L.fpca_debug_set_pass_slices(ctx.h, 4) == -1 and b"exact-integer" in L.fpca_last_error()
        assert L.fpca_debug_set_pass_slices(None, 4) == -1 and b"NULL" in L.fpca_last_error()


def test_product_build_has_no_such_switch(built_lib):
    """In the product build the hook answers FPCA_EINVAL, says why, and the next product is what it was."""
    import flashpca_amd as fp

    L = fp.lib()
    S, Sc, b = 7, 4, 16
    o, w = PY.case_operand("D0", Sc, b, "xt", 0), PY.witness_operand("D0", S, Sc, b, "xt")
    with _ctx(fp, "D0", "i8x7") as ctx:
        R0, RW = ctx.apply_xt(o.x), ctx.apply_xt(w.x)
        assert np.array_equal(R0, _reference("D0", Sc, b, "xt", 0)) and not np.array_equal(RW, R0)
        assert L.fpca_debug_set_pass_slices(ctx.h, Sc) == -1 and b"product build" in L.fpca_last_error()
        with pytest.raises(fp.FpcaError):
            ctx.debug_pass_slices(Sc)
        assert np.array_equal(ctx.apply_xt(o.x), R0) and np.array_equal(ctx.apply_xt(w.x), RW)  # still on 7 slices: the quarter is a digit


def test_pca_clears_the_setting(built_lib):
    """fpca_pca drives the field itself and leaves it at 0: after it the witness of a 4-slice pass behaves as on an exact pass."""
    import flashpca_amd as fp

    S, Sc, b = 7, 4, 16
    o, w = PY.case_operand("D1", Sc, b, "xt", 0), PY.witness_operand("D1", S, Sc, b, "xt")
    with fp.test_hooks():
        with _ctx(fp, "D1", "i8x7") as ctx:
            exact = ctx.apply_xt(w.x)
            ctx.debug_pass_slices(Sc)
            R0, RW = ctx.apply_xt(o.x), ctx.apply_xt(w.x)
            assert np.array_equal(R0, _reference("D1", Sc, b, "xt", 0)) and np.array_equal(RW, R0) and not np.array_equal(exact, R0)
            r = ctx.pca(ndim=3, tol=1e-3, maxiter=50, allow_unconverged=True)
            assert r["info"]["block_applies"] > 0
            assert np.array_equal(ctx.apply_xt(o.x), R0) and np.array_equal(ctx.apply_xt(w.x), exact)
