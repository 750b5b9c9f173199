"""The two-phase split-K plan of the int8 GEMM (csrc/kernels_i8.hip: i8_plan, k_gemm_i8, k_i8_combine) at small shapes.

Phase A -- whole rounds of #CU tile ids, unsplit -- needs more tile ids than the device has CUs, i.e. tens of thousands of rows; below
that every launch is plain split-K (nA = 0) and the partial planes of all rows are laid out alike.  FPCA_I8_NCU (test build) makes
i8_plan plan for 16 / 24 / 32 / 64 CUs instead, so that a few thousand rows reach the regime in which phase B writes its extra planes
for the rows >= rowB0 only, indexed by row - rowB0, and the combine decides per tile how many planes it adds.  The kernel does not
depend on the CU count; the workspace is sized by the same plan.

Every child process (the knobs are read once per process) runs several contexts with FPCA_I8_VERBOSE=1 and FPCA_DEBUG_I8_POISON=1:
the workspace extent the plan uses is NaN before every launch, so a plane nobody writes cannot pass for the previous launch's value
-- every output must be finite.  The plan of every launch is read from stderr (`int8 GEMM plan:` followed by `int8 GEMM launch:`, the
latter only for a plan that is launched -- the workspace sizing prints plans too) and each case ASSERTS the regime it is about: tile ids,
nA > 0, sB, a ragged last split, rowB0 > 0, and the kernel instance.  The expected numbers come from a Python port of i8_shape /
i8_plan run on the CPU; they do not depend on the device, because the CU count is given.

Checks:
 * X'B (K2) on an integer block B in [-4, 4]: the column scale of the slicing is a power of two (k_slice: 2^e from frexp of the column
   maximum, m = rn(x 2^(8S-2-e)) -- exact for small integers at any S), so G.M'B and M'B are exact integers in every partial whatever
   the split, and the result is a function of (g, m, mean, sd) alone: bit-identical to the default plan's (nA = 0, a child without the
   CU override) and within 4 u (|g| + |mean m|) / sd of (g - mean m) / sd in longdouble with g, m from int64 numpy (one rounding each
   for the product, the difference and the quotient, one of slack for a contracted multiply-add), exactly 0 where sd <= 1e-9.
 * X T (K3) and X X'B on normal operands against the oracle's dense matrix at the tolerance of test_i8_mode_operator_parity for the
   same S (10 x 1e-12 at S = 7, 1e-11 for 48 columns, 3e-6 at S = 4).  S = 3 has no entry there; its X T is held to the rounding of
   the slicing itself: an operand entry is off by at most colmax 2^-(8S-2) (half an ulp of 2^(e-8S+2), 2^e <= 2 colmax), the integer
   sums are exact, so |dY[i, c]| <= 2^-(8S-2) (sum_j (G.M)[i, j] colmax_c(T/sd) + sum_j M[i, j] colmax_c(mean T/sd)), plus 1e-12 of
   the column maximum for the fp64 combine and the reference's own sums.
 * every product is called with a first operand, a different one, and the first again: the third result equals the first bit for bit.

Instances reached with nA > 0, and the plan line of each (rows / K padded; "a + b x s (c)" = a unsplit + b tiles x s splits of c chunks):
 NCU 16, N 4500, P 2700 (X T: rows 4608, K 2816 = 11 chunks; 18 row tiles -> 24 tile ids, 6 of the 8 phase-B ids idle):
   one operand I8_NO_MISSING b 16 S 7 (half tile, nt 4)   tile 256x112 zb 1 -> 24 ids; 16 + 8 x 2 (6), phase B from row 4096
   the same with FPCA_I8_TILED=0 (row-major copies)        the same plan
   one operand b 16 S 4 (nt 2)                             tile 256x64  zb 1 -> 24 ids; 16 + 8 x 2 (6)
   one operand b 16 S 3 (half tile, nt 2; accum="i8x3")    tile 256x48  zb 1 -> 24 ids; 16 + 8 x 2 (6)
   one operand b 32 S 7 (nt 7), band-tiled and row-major   tile 256x224 zb 1 -> 24 ids; 16 + 8 x 2 (6)
   sparse route (mode 3) b 16 S 7: eplane on both sides of rowB0      the plan of the first line
   two operands I8_FULL b 16 S 7 (half tile)               tile 256x112 zb 1 -> 24 ids; 16 + 8 x 2 (6)
   K2 of both matrices, 128-row, b 32 S 7 I8_FULL (nt 7)   rows 2816 K 4608 tile 128x224 -> 24 ids; 16 + 8 x 2 (9), from row 2048
 NCU 16, N 2700, P 4500 (X'B: rows 4608, K 3072 = 12 chunks):
   K2 one operand b 16 S 7 (half), band-tiled third copy and row-major   tile 256x112 -> 24 ids; 16 + 8 x 2 (6)
   K2 one operand b 16 S 7 + sparse eplane (mode 3)                       the same plan
   K2 of both matrices, 256-row (nt 2), b 16 S 4 I8_FULL                  tile 256x64  -> 24 ids; 16 + 8 x 2 (6)
   K2 of both matrices, 128-row, b 32 S 7 I8_FULL / I8_SKIP_EMPTY         tile 128x224 -> 40 ids; 32 + 8 x 2 (6)
 NCU 32 (zb = 2), N 4500, P 2700: one operand b 64 S 7 (nt 7) and b 48 S 7 (nt 6, bw 96), two operands b 32 S 7 I8_FULL and
   I8_SKIP_EMPTY, sparse route b 64:                       tile 256x{224,192,128} zb 2 -> 48 ids; 32 + 16 x 2 (6)
   N 2700, P 4500: K2 one operand b 64 / b 48              rows 4608 K 3072 zb 2 -> 48 ids; 32 + 16 x 2 (6)
 NCU 64 (zb = 4), N 4500, P 3300: two operands b 64 S 7 I8_FULL / I8_SKIP_EMPTY   tile 256x128 zb 4 -> 96 ids; 64 + 32 x 2 (7 of 13)
 NCU 24 (three splits), N 6600, P 3300:
   one operand b 32 S 7, and sparse route b 16 S 7 (half)  rows 6656 K 3328 -> 32 ids; 24 + 8 x 3 (5 of 13), from row 6144
   K2 of both matrices, 128-row, b 32 S 7 I8_FULL          rows 3328 K 6656 tile 128x224 -> 32 ids; 24 + 8 x 3 (9 of 26), from row 3072
   N 2500, P 3300: one operand b 64 S 7, zb 2: nA / 8 = 3 is no multiple of zb -- row tiles 8 .. 9 have one column block in each
   phase                                                   rows 2560 K 3328 zb 2 -> 32 ids; 24 + 8 x 3 (5 of 13), from row 2048
 default CU count, FPCA_I8_SPLITS=3, N 4500, P 3300: plain split-K, 0 + 24 x 3 (5 of 13) and 0 + 16 x 3 (6 of 18).
(The issue's K2 shape 2560 x 2304 does not exist: N pads to 512, so K2 has an even number of chunks and two splits are never ragged;
the ragged K2 case is the three-way one at NCU 24.  Every row of its table reproduced otherwise.)"""
import json
import os
import re
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, os, sys, zlib
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
cases = json.loads(sys.argv[2])
out, info = {}, {}

def mark(s):
    sys.stderr.write("MARK " + s + "\n")
    sys.stderr.flush()

def thrice(f, A, A2):
    R1 = f(A)
    R2 = f(A2)
    R3 = f(A)
    return R1, bool(np.isfinite(R1).all() and np.isfinite(R2).all() and np.max(np.abs(R2)) > 0), bool(np.array_equal(R1, R3) and not np.array_equal(R1, R2))

with fp.test_hooks():
    for case in cases:
        cid, N, P, b, S = case["id"], case["N"], case["P"], case["b"], case["S"]
        for k, v in (("FPCA_I8_MODE", case.get("mode")), ("FPCA_I8_TILED", case.get("tiled"))):  # (both are read per context / per call)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        with fp.Context.synthetic(N, P, n_pop=6, missing_rate=case["miss"], accum="i8x%d" % S) as ctx:
            i = {"mode": ctx.missing_mode(b)}
            dkey = "packed_%d_%d_%g" % (N, P, case["miss"])
            if dkey not in out:
                out[dkey] = ctx.download_packed()
                out["meansd_%d_%d_%g" % (N, P, case["miss"])] = ctx.stats()[0]
            i["crc"] = zlib.crc32(out[dkey].tobytes())
            rng = np.random.default_rng(1000 * N + b)
            Bi, Bi2 = (rng.integers(-4, 5, size=(N, b)).astype(np.float64) for _ in range(2))
            Bn, Bn2 = rng.standard_normal((N, b)), rng.standard_normal((N, b))
            Tn, Tn2 = rng.standard_normal((P, b)), rng.standard_normal((P, b))
            for op, f, A, A2 in (("xt", ctx.apply_xt, Bi, Bi2), ("x", ctx.apply_x, Tn, Tn2), ("xxt", ctx.apply_xxt, Bn, Bn2)):
                if op in case["ops"]:
                    mark(cid + " " + op)
                    out[cid + "." + op], i[op + "_finite"], i[op + "_repeat"] = thrice(f, A, A2)
            mark(cid + " end")
            info[cid] = i
np.savez(sys.argv[3], **out)
print("CHILD " + json.dumps(info))
"""

_PLAN = re.compile(r"int8 GEMM plan: rows (\d+) K (\d+) tile (\d+)x(\d+) zb (\d+) -> (\d+) tile ids, (\d+) chunks; (\d+) unsplit \+ (\d+) tiles x (\d+) splits "
                   r"\((\d+) chunks each\), (\d+) workgroups")
_LAUNCH = re.compile(r"int8 GEMM launch: (one|two) operands?, mode (\d), nt (\d)( \(half tile\))?, (band-tiled|row-major)(, E alone)?; phase B from row (\d+)")


def _launches(stderr):
    """{(case id, op): [launch, ...]}: every launched plan (a plan line directly followed by a launch line) between two marks."""
    res, key, plan = {}, None, None
    for line in stderr.splitlines():
        if line.startswith("MARK "):
            cid, op = line[5:].split()
            key, plan = (cid, op), None
            res.setdefault(key, [])
            continue
        m = _PLAN.search(line)
        if m:
            plan = [int(x) for x in m.groups()]
            continue
        m = _LAUNCH.search(line)
        if m and key is not None:
            assert plan is not None, line
            rows, K, tr, tc, zb, ids, chunks, nA, nB, sB, cps, grid = plan
            res[key].append(dict(rows=rows, K=K, tile=(tr, tc), zb=zb, ids=ids, chunks=chunks, nA=nA, nB=nB, sB=sB, cps=cps, grid=grid,
                                 two=m.group(1) == "two", kmode=int(m.group(2)), nt=int(m.group(3)), half=bool(m.group(4)),
                                 tiled=m.group(5) == "band-tiled", rowB0=int(m.group(7))))
        plan = None
    return res


def _run(cases, env_extra, tmp, name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    env.update(env_extra)
    env.update({"FPCA_I8_VERBOSE": "1", "FPCA_DEBUG_I8_POISON": "1"})
    spec = [{k: v for k, v in c.items() if k != "expect"} for c in cases]
    out = os.path.join(tmp, name + ".npz")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(spec), out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
    return dict(np.load(out)), info, _launches(r.stderr)


def _pad(x, a):
    return (x + a - 1) // a * a


# ---- references, one per data set (the synthetic generator is seeded: every process builds the same matrix, checked by CRC) ----
_REF = {}


def _ref(res, N, P, miss):
    key = (N, P, miss)
    if key not in _REF:
        packed = res["packed_%d_%d_%g" % key]
        codes = packed.reshape(P, (N + 3) // 4)
        codes = np.stack([(codes >> (2 * s)) & 3 for s in range(4)], axis=2).reshape(P, -1)[:, :N]  # sample 4 i + s: bits 2 s .. 2 s + 1 of byte i
        GM = np.where(codes == 0, 2, np.where(codes == 2, 1, 0)).astype(np.int64)  # dosage, 0 where missing (code 1)
        M = (codes != 1).astype(np.int64)
        _REF[key] = dict(GM=GM, M=M, packed=packed, crc=zlib.crc32(packed.tobytes()), meansd=res["meansd_%d_%d_%g" % key])
    return _REF[key]


def _operands(N, P, b):
    rng = np.random.default_rng(1000 * N + b)  # as in the child
    Bi = rng.integers(-4, 5, size=(N, b)).astype(np.float64)
    rng.integers(-4, 5, size=(N, b))
    Bn = rng.standard_normal((N, b))
    rng.standard_normal((N, b))
    Tn = rng.standard_normal((P, b))
    return Bi, Bn, Tn


_TOL = {7: 1e-12, 4: 3e-6}  # test_i8_mode_operator_parity, per S (48 columns at S = 7: 1e-11)


def _check_case(case, res, info, launches, default=None):
    cid, N, P, b, S, miss = case["id"], case["N"], case["P"], case["b"], case["S"], case["miss"]
    i = info[cid]
    ref = _ref(res, N, P, miss)
    assert i["crc"] == ref["crc"], cid
    if case.get("mode") is not None:
        assert i["mode"] == case["mode"], (cid, i)
    elif miss == 0.0:
        assert i["mode"] == 2, (cid, i)
    # the regime the case is about
    for e in case.get("expect", []):
        ls = [l for l in launches[(cid, e["op"])] if l["rows"] == e["rows"]]
        assert len(ls) == 3, (cid, e, launches[(cid, e["op"])])  # one launch per call of the product
        for l in ls:
            print(cid, e["op"], l)
            assert l["nA"] == e["nA"] and (e["nA"] > 0 or e.get("plain")), (cid, l)
            assert l["ids"] == e["ids"] and l["sB"] == e["sB"] and l["sB"] >= 2 and l["cps"] == e["cps"] and l["chunks"] == e["chunks"], (cid, l, e)
            assert (l["sB"] * l["cps"] != l["chunks"]) == e.get("ragged", False), (cid, l)
            assert l["rowB0"] == e["rowB0"] and (e["nA"] == 0 or 0 < l["rowB0"] < l["rows"]), (cid, l)
            assert l["grid"] == l["nA"] + l["nB"] * l["sB"] and l["nA"] + l["nB"] == l["ids"], (cid, l)
            assert (l["two"], l["kmode"], l["nt"], l["half"], l["tile"], l["zb"]) == (e["two"], e["kmode"], e["nt"], e.get("half", False), tuple(e["tile"]),
                                                                                    e["zb"]), (cid, l, e)
            if "tiled" in e:
                assert l["tiled"] == e["tiled"], (cid, l)
    Bi, Bn, Tn = _operands(N, P, b)
    for op in case["ops"]:
        R = res[cid + "." + op]
        assert np.isfinite(R).all() and i[op + "_finite"], (cid, op)  # the poison: an unwritten plane shows as NaN
        assert i[op + "_repeat"], (cid, op)
    if "xt" in case["ops"]:  # integer operands: exact
        T = res[cid + ".xt"]
        Bint = Bi.astype(np.int64)
        assert np.array_equal(Bint, Bi)
        if ("gm", b) not in ref:  # (cases of one data set and width share B; M = 1 - E with few missing calls: M'B = 1'B - E'B)
            EB = np.zeros((P, b), dtype=np.int64)
            rows, cols = np.nonzero(ref["M"] == 0)
            np.add.at(EB, rows, Bint[cols])
            ref["gm", b] = ref["GM"] @ Bint, Bint.sum(axis=0)[None, :] - EB
        g, m = ref["gm", b]
        assert np.max(np.abs(g)) < 2 ** 53 and np.max(np.abs(m)) < 2 ** 53
        mean, sd = ref["meansd"][:, 0].astype(np.longdouble)[:, None], ref["meansd"][:, 1].astype(np.longdouble)[:, None]
        live = (ref["meansd"][:, 1] > 1e-9)[:, None]
        gl, ml = g.astype(np.longdouble), m.astype(np.longdouble)
        sd1 = np.where(live, sd, 1)
        want = np.where(live, (gl - mean * ml) / sd1, 0)
        bound = np.where(live, 4 * np.longdouble(2.0) ** -53 * (np.abs(gl) + np.abs(mean * ml)) / sd1, 0)
        err = np.abs(T.astype(np.longdouble) - want)
        print(cid, "xt: max error / bound", float(np.max(err / np.where(bound > 0, bound, 1))), "monomorphic SNPs", int((~live).sum()))
        assert np.all(err <= bound), (cid, float(np.max(err - bound)))
        assert np.all(T[~live[:, 0]] == 0.0)
        if default is not None:  # the default plan (nA = 0) on the same data: the same bits
            dres, dinfo, dl = default
            assert dinfo[cid]["crc"] == i["crc"]
            dls = [l for l in dl[(cid, "xt")] if l["rows"] == _pad(P, 256)]
            assert len(dls) == 3 and all(l["nA"] == 0 for l in dls), dls
            if case.get("expect"):
                assert any(e["op"] == "xt" for e in case["expect"]), cid  # (the case's own plan differs: asserted above)
            assert np.array_equal(T, dres[cid + ".xt"]), (cid, float(np.max(np.abs(T - dres[cid + ".xt"]))))
    if ("x" in case["ops"] or "xxt" in case["ops"]) and "X" not in ref:
        from oracle import oracle as O

        ref["X"] = O.OracleData(packed=ref["packed"], N=N, P=P, stand="binom2").dense()
    X = ref.get("X")
    if "x" in case["ops"]:
        Y, Yr = res[cid + ".x"], X @ Tn
        if S in _TOL:
            tol = 10 * (1e-11 if b == 48 else _TOL[S])
            e = np.max(np.abs(Y - Yr) / np.max(np.abs(Yr), axis=0))
            print(cid, "x: error", e, "tolerance", tol)
            assert e <= tol, (cid, e)
        else:  # S = 3: the rounding of the slicing itself (module docstring)
            mean, sd = ref["meansd"][:, 0], ref["meansd"][:, 1]
            inv = np.where(sd > 1e-9, 1.0 / np.where(sd > 1e-9, sd, 1.0), 0.0)
            a, c = Tn * inv[:, None], Tn * (mean * inv)[:, None]
            bound = 2.0 ** -(8 * S - 2) * (ref["GM"].sum(axis=0)[:, None] * np.max(np.abs(a), axis=0)[None, :]
                                           + ref["M"].sum(axis=0)[:, None] * np.max(np.abs(c), axis=0)[None, :]) + 1e-12 * np.max(np.abs(Yr), axis=0)
            e = np.abs(Y - Yr)
            print(cid, "x: max error / bound", np.max(e / bound), "bound / column maximum", np.max(bound / np.max(np.abs(Yr), axis=0)))
            assert np.all(e <= bound), (cid, np.max(e / bound))
    if "xxt" in case["ops"]:
        Z, Zr = res[cid + ".xxt"], X @ (X.T @ Bn)
        tol = 10 * (1e-11 if b == 48 else _TOL[S])
        e = np.max(np.abs(Z - Zr) / np.max(np.abs(Zr), axis=0))
        print(cid, "xxt: error", e, "tolerance", tol)
        assert e <= tol, (cid, e)


def _x(rows, K, tile, zb, ids, nA, sB, cps, nt, two=False, kmode=2, half=False, op="x", **kw):
    """Expected launch: X T (op x) or X'B (op xt) over `rows` x `K`; rowB0 = first row tile of phase B (i8_plan: qA = nA / 8 / zb)."""
    chunks = K // 256
    return dict(op=op, rows=rows, tile=tile, zb=zb, ids=ids, nA=nA, sB=sB, cps=cps, chunks=chunks, ragged=sB * cps != chunks, nt=nt, two=two, kmode=kmode,
                half=half, rowB0=min(nA // 8 // zb * 8 * tile[0], rows), **kw)


ALL3 = ["xt", "x", "xxt"]
# X T of N 4500 x P 2700: rows 4608, K 2816 (11 chunks, 2 x 6 ragged); 18 row tiles of 256 -> 24 ids, 16 in phase A, 6 of the other 8 idle
K3_NCU16 = [
    dict(id="b16S7", N=4500, P=2700, miss=0.0, b=16, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 112), 1, 24, 16, 2, 6, 4, half=True, tiled=True)]),
    dict(id="b16S7rm", N=4500, P=2700, miss=0.0, b=16, S=7, tiled=0, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 112), 1, 24, 16, 2, 6, 4, half=True, tiled=False)]),
    dict(id="b16S4", N=4500, P=2700, miss=0.0, b=16, S=4, ops=["x", "xxt"], expect=[_x(4608, 2816, (256, 64), 1, 24, 16, 2, 6, 2, tiled=True)]),
    dict(id="b16S3", N=4500, P=2700, miss=0.0, b=16, S=3, ops=["x"], expect=[_x(4608, 2816, (256, 48), 1, 24, 16, 2, 6, 2, half=True, tiled=True)]),
    dict(id="b32S7", N=4500, P=2700, miss=0.0, b=32, S=7, ops=["x", "xxt"], expect=[_x(4608, 2816, (256, 224), 1, 24, 16, 2, 6, 7, tiled=True)]),
    dict(id="b32S7rm", N=4500, P=2700, miss=0.0, b=32, S=7, tiled=0, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 224), 1, 24, 16, 2, 6, 7, tiled=False)]),
    dict(id="b16S7sparse", N=4500, P=2700, miss=0.001, mode=3, b=16, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 112), 1, 24, 16, 2, 6, 4, half=True, tiled=True)]),
    dict(id="b16S7full", N=4500, P=2700, miss=0.02, mode=0, b=16, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 112), 1, 24, 16, 2, 6, 4, two=True, kmode=0, half=True, tiled=True)]),
    # (X T of both matrices at b 32 has 48 ids = 3 whole rounds: unsplit.)  X'B: rows 2816, K 4608, 22 row tiles of 128 -> 24 ids
    dict(id="b32S7full", N=4500, P=2700, miss=0.02, mode=0, b=32, S=7, ops=ALL3,
         expect=[_x(2816, 4608, (128, 224), 1, 24, 16, 2, 9, 7, kmode=0, op="xt", tiled=False)]),
]
# X'B of N 2700 x P 4500: rows 4608, K 3072 (12 chunks)
K2_NCU16 = [
    dict(id="k2b16S7", N=2700, P=4500, miss=0.0, b=16, S=7, ops=ALL3,
         expect=[_x(4608, 3072, (256, 112), 1, 24, 16, 2, 6, 4, half=True, op="xt", tiled=True)]),
    dict(id="k2b16S7rm", N=2700, P=4500, miss=0.0, b=16, S=7, tiled=0, ops=ALL3,
         expect=[_x(4608, 3072, (256, 112), 1, 24, 16, 2, 6, 4, half=True, op="xt", tiled=False)]),
    dict(id="k2b16S7sparse", N=2700, P=4500, miss=0.001, mode=3, b=16, S=7, ops=ALL3,
         expect=[_x(4608, 3072, (256, 112), 1, 24, 16, 2, 6, 4, half=True, op="xt", tiled=True)]),
    dict(id="k2b16S4full", N=2700, P=4500, miss=0.02, mode=0, b=16, S=4, ops=ALL3,
         expect=[_x(4608, 3072, (256, 64), 1, 24, 16, 2, 6, 2, kmode=0, op="xt", tiled=False)]),
    dict(id="k2b32S7full", N=2700, P=4500, miss=0.02, mode=0, b=32, S=7, ops=ALL3,
         expect=[_x(4608, 3072, (128, 224), 1, 40, 32, 2, 6, 7, kmode=0, op="xt", tiled=False)]),
    dict(id="k2b32S7skip", N=2700, P=4500, miss=0.001, mode=1, b=32, S=7, ops=ALL3,
         expect=[_x(4608, 3072, (128, 224), 1, 40, 32, 2, 6, 7, kmode=1, op="xt", tiled=False)]),
]
# two column blocks: 18 row tiles x 2 -> 48 ids, 32 in phase A
NCU32 = [
    dict(id="b64S7", N=4500, P=2700, miss=0.0, b=64, S=7, ops=["x", "xxt"], expect=[_x(4608, 2816, (256, 224), 2, 48, 32, 2, 6, 7, tiled=True)]),
    dict(id="b64S7rm", N=4500, P=2700, miss=0.0, b=64, S=7, tiled=0, ops=["x"], expect=[_x(4608, 2816, (256, 224), 2, 48, 32, 2, 6, 7, tiled=False)]),
    dict(id="b48S7", N=4500, P=2700, miss=0.0, b=48, S=7, ops=["x", "xxt"], expect=[_x(4608, 2816, (256, 192), 2, 48, 32, 2, 6, 6, tiled=True)]),
    dict(id="b64S7sparse", N=4500, P=2700, miss=0.001, mode=3, b=64, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 224), 2, 48, 32, 2, 6, 7, tiled=True)]),
    dict(id="b32S7full", N=4500, P=2700, miss=0.02, mode=0, b=32, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 128), 2, 48, 32, 2, 6, 4, two=True, kmode=0, tiled=True)]),
    dict(id="b32S7skip", N=4500, P=2700, miss=0.001, mode=1, b=32, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 2816, (256, 128), 2, 48, 32, 2, 6, 4, two=True, kmode=1, tiled=True)]),
    dict(id="k2b64S7", N=2700, P=4500, miss=0.0, b=64, S=7, ops=["xt"], expect=[_x(4608, 3072, (256, 224), 2, 48, 32, 2, 6, 7, op="xt", tiled=True)]),
    dict(id="k2b48S7", N=2700, P=4500, miss=0.0, b=48, S=7, ops=["xt"], expect=[_x(4608, 3072, (256, 192), 2, 48, 32, 2, 6, 6, op="xt", tiled=True)]),
]
# four column blocks: 18 row tiles x 4 -> 96 ids, 64 in phase A; K 3328 = 13 chunks, 2 x 7 ragged
NCU64 = [
    dict(id="b64S7full", N=4500, P=3300, miss=0.02, mode=0, b=64, S=7, ops=["x", "xxt"],
         expect=[_x(4608, 3328, (256, 128), 4, 96, 64, 2, 7, 4, two=True, kmode=0, tiled=True)]),
    dict(id="b64S7skip", N=4500, P=3300, miss=0.001, mode=1, b=64, S=7, ops=["x"],
         expect=[_x(4608, 3328, (256, 128), 4, 96, 64, 2, 7, 4, two=True, kmode=1, tiled=True)]),
]
# three splits behind a phase A: 26 row tiles -> 32 ids, 24 in phase A; 13 chunks = 5 + 5 + 3; X'B: 26 chunks = 9 + 9 + 8
NCU24 = [
    dict(id="b32S7", N=6600, P=3300, miss=0.0, b=32, S=7, ops=["x", "xxt"], expect=[_x(6656, 3328, (256, 224), 1, 32, 24, 3, 5, 7, tiled=True)]),
    dict(id="b16S7sparse", N=6600, P=3300, miss=0.001, mode=3, b=16, S=7, ops=["x"],
         expect=[_x(6656, 3328, (256, 112), 1, 32, 24, 3, 5, 4, half=True, tiled=True)]),
    dict(id="k2b32S7full3", N=6600, P=3300, miss=0.02, mode=0, b=32, S=7, ops=["xt", "xxt"],
         expect=[_x(3328, 6656, (128, 224), 1, 32, 24, 3, 9, 7, kmode=0, op="xt", tiled=False)]),
    # 10 row tiles x 2 column blocks -> 32 ids; nA / 8 = 3 is odd: row tiles 8, 9 have column block 0 in phase A and 1 in phase B
    dict(id="b64S7", N=2500, P=3300, miss=0.0, b=64, S=7, ops=["x", "xxt"], expect=[_x(2560, 3328, (256, 224), 2, 32, 24, 3, 5, 7, tiled=True)]),
]
# FPCA_I8_SPLITS=3 at the device's own CU count: plain split-K, three ways
SPLITS3 = [
    dict(id="s3b32S7", N=4500, P=3300, miss=0.0, b=32, S=7, ops=ALL3,
         expect=[_x(4608, 3328, (256, 224), 1, 24, 0, 3, 5, 7, plain=True), _x(3328, 4608, (256, 224), 1, 16, 0, 3, 6, 7, op="xt", plain=True)]),
]


@pytest.fixture(scope="module")
def default_plan(built_lib):
    """X'B of every integer-operand case under the default plan (the device's CU count: at most 80 tile ids, nA = 0)."""
    cases = [dict(c, ops=["xt"]) for group in (K3_NCU16, K2_NCU16, NCU32, NCU24, SPLITS3) for c in group if "xt" in c["ops"]]
    assert len({c["id"] for c in cases}) == len(cases)
    with tempfile.TemporaryDirectory() as tmp:
        return _run(cases, {}, tmp, "default")


def _group(cases, env, default):
    with tempfile.TemporaryDirectory() as tmp:
        res, info, launches = _run(cases, env, tmp, "plan")
    for case in cases:
        _check_case(case, res, info, launches, default)


@pytest.mark.gpu
def test_two_phase_one_column_block_xt(default_plan):
    """X T behind a phase A, one column block: every one-operand instance (half tiles, 2 / 7 tiles, both layouts), the sparse route's
    eplane on both sides of rowB0, both matrices at b 16; X'B of both matrices in 128-row tiles.  Ragged last split, 6 idle ids."""
    _group(K3_NCU16, {"FPCA_I8_NCU": "16"}, default_plan)


@pytest.mark.gpu
def test_two_phase_x_transposed_b(default_plan):
    """X'B behind a phase A on integer operands: bit-identical to the default plan and within 4 u of the longdouble reference."""
    _group(K2_NCU16, {"FPCA_I8_NCU": "16"}, default_plan)


@pytest.mark.gpu
def test_two_phase_two_column_blocks(default_plan):
    _group(NCU32, {"FPCA_I8_NCU": "32"}, default_plan)


@pytest.mark.gpu
def test_two_phase_four_column_blocks(default_plan):
    _group(NCU64, {"FPCA_I8_NCU": "64"}, default_plan)


@pytest.mark.gpu
def test_two_phase_three_splits(default_plan):
    _group(NCU24, {"FPCA_I8_NCU": "24"}, default_plan)


@pytest.mark.gpu
def test_forced_plain_split_k(default_plan):
    """FPCA_I8_SPLITS=3: no phase A, three splits (ragged for X T) -- and the same bits as the plan the device chooses."""
    _group(SPLITS3, {"FPCA_I8_SPLITS": "3"}, default_plan)


def test_expected_plans_are_two_phase():
    """The table itself (no GPU): every case but the forced plain split-K expects a phase A, at least two splits and 0 < rowB0 < rows;
    the ragged ones are the 11- and 13-chunk X T and the 26-chunk X'B."""
    for group in (K3_NCU16, K2_NCU16, NCU32, NCU64, NCU24):
        for c in group:
            for e in c["expect"]:
                assert e["nA"] > 0 and e["nA"] % 8 == 0 and e["sB"] >= 2 and 0 < e["rowB0"] < e["rows"] and e["ids"] > e["nA"], c["id"]
                assert e["ragged"] == (e["chunks"] in (11, 13, 26)), c["id"]
                assert e["rows"] == _pad(c["N"], 512) if e["op"] == "x" else e["rows"] == _pad(c["P"], 256), c["id"]
    assert any(e["sB"] == 3 for c in NCU24 for e in c["expect"])
