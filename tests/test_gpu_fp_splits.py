"""The split-K plans of the fp64 / fp32 kernels (csrc/kernels.hip: k_xt_b / k_x_t, the dense pair k_xt_b_dense / k_x_t_dense and the
combine reduce_sum) at the smallest shapes at which each regime exists, on data for which the result is EXACT.

What the other operator tests launch (a Python port of pick_splits / xt_b_splits / x_t_splits and of the launchers' chunk arithmetic,
below, run over their shapes): 1 to 12 splits of exactly 4 chunks each.  Never a ragged last split, never an empty one, never a split
that starts on a chunk index that is no multiple of 4 (the fp32 fold), never reduce_sum's leftover planes or k_reduce_tall.
FPCA_XT_SPLITS / FPCA_X_SPLITS (test build) force the number of splits; they are read once per process, so every pair of values runs
in a child process of its own, and one more child runs the same data under the plan the library chooses.

Exact data.  Under stand="binom" a SNP with as many dosage-2 as dosage-0 calls among its real samples has mean 1.0, sd 0.5 and the
table {2, 0, 0, -2} exactly (asserted through stats() first), so the standardised matrix is an integer matrix over {-2, 0, 2}.  With
integer operands in [-4, 4] every product and every partial sum is an integer far below 2^53 -- and, in fp32 mode, below 2^24 inside a
fold of four chunks (K2: 512 samples x 2 x 4; K3: 256 SNPs x 2 x max|T|, asserted as 512 max|T| < 2^24) -- so X'B, X T and X X'B must
equal int64 numpy with np.array_equal under EVERY plan, chunk order and combine association, and equal each other between plans.
Each SNP set also holds an all-het SNP, an all-missing one (NaN mean) and a monomorphic one (every byte 0xFF); rows 0 and N - 1 of B,
each alone in an otherwise zero block, are operands of their own for X'B and X X'B.

Every product is called with an operand A, a different A2, and A again after fpca_debug_poison_partials has filled the partial
planes and T with NaNs: a plane or tile nobody writes shows as NaN instead of the first call's value.  The plan of every context and
width comes from fpca_debug_fp_plan -- the host helpers the launchers themselves call -- and must equal the port's and show the regime
the case is named for, so that a case that fell back to another plan fails.

Plans (chunks per split; K2 at 16 / 32 columns has 128-sample chunks in super-chunks of two, 64-sample chunks at 48 / 64; K3 has
64-SNP chunks, 32 in fp32 mode at 48 / 64 columns):
  child XT=3 X=5,  N 1001 (N_pad 1024) x P 513 (P_pad 768):   K2 [4, 4, 0] | [6, 6, 4]            K3 [3, 3, 3, 3, 0] | [5, 5, 5, 5, 4]
  child XT=3 X=6,  N 2307 (2560) x P 1280 (= P_pad):          K2 [8, 8, 4] | [14, 14, 12]         K3 [4 x 5, 0] | [7 x 5, 5]
  child XT=5 X=3,  N 1536 (= N_pad) x P 1100 (1280):          K2 [4, 4, 4, 0, 0] | [5, 5, 5, 5, 4] K3 [7, 7, 6] | [14, 14, 12]
                   the same matrix through from_dense:        K2d [5, 5, 5, 5, 4]                 K3d [7, 7, 6]
  child XT=7 X=7,  N 1999 (2048) x P 700 (768):               K2 [4, 4, 4, 4, 0, 0, 0] | [5 x 6, 2] K3 [2 x 6, 0] | [4 x 6, 0]
  child XT=64 X=64, N 8190 (8192) x P 201 (256):              K2 32 x 2 + 32 empty | 64 x 2, combined by k_reduce_tall; dense 64 x 2
                    N 509 (512) x P 4000 (4096):              K3 64 x 1 | 64 x 2, k_reduce_tall; dense 64 x 1
  default plan,    N 5001 (5120) x P 3300 (3328), fp64, 16 columns: K2 [6, 6, 6, 6, 6, 6, 4, 0] -- the smallest shape (by N_pad x P_pad,
                   searched with the port up to 8192 x 8192) whose DEFAULT plan has an empty split (N_pad 3072 needs P_pad 5632).
Widths 16, 32, 48, 64 and the non-multiples 5 and 37, in fp64 and fp32: every instance of both templates under a ragged or empty plan.

General data (a handful): ordinary genotypes under binom2 with normal operands, under the K2 [4, 4, 0] / [6, 6, 4] and K3 [3, 3, 3, 3, 0] /
[7, 7, 6] plans, against np.longdouble products of the float64 tables rebuilt from the context's own stats() with make_lut's operations.
fp64: |error| <= 2 (n + 4) u |X|'|B| entrywise (n = padded inner dimension, u = 2^-53: the forward bound of a sum of n products in any
order, doubled as in test_gpu_k4_shapes.py); for X X'B the two bounds compose, (g1 + g2 + g1 g2) |X| (|X|'|B|).  fp32: 2e-6 of the
output scale, as test_fp32_mode_operator_tolerance.  Exact data cannot tell het from missing (both standardise to 0); this can.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
WIDTHS = [16, 32, 48, 64, 5, 37]
NCOL = 64


# ---------------------------------------------------------------------------------------------------------------------------
# Python port of the plan arithmetic (csrc/kernels.hip: pick_splits, xt_b_splits / x_t_splits and their dense twins, xt_b_chunks /
# x_t_chunks / dense_chunks).  Its agreement with fpca_debug_fp_plan on every case is the test of those host helpers.
def pick_splits(tiles, chunks, min_chunks, max_splits, slots):
    best_t, best, s = None, 1, 1
    while s <= max_splits and s <= chunks:
        cps = (chunks + s - 1) // s
        if s > 1 and cps < min_chunks:
            break
        seff = (chunks + cps - 1) // cps
        wgs = tiles * seff
        per_cu = (wgs + 255) // 256
        t = per_cu * (cps * 64 + 96)
        if wgs > slots:
            t += (cps * 64 + 96) // 2
        if per_cu < 2:
            t = t * 7 // 5
        if seff > 1:
            t += seff * 24 * ((tiles + 255) // 256)
        if best_t is None or t < best_t:
            best_t, best = t, seff
        s += 1
    return best


def k2_plan(N_pad, P_pad, b, fp32, forced=0, dense=False):
    """(splits, chunks per split handed to the kernel, chunks in all) of X'B"""
    if dense:
        kc = 64
        ns = min(forced, N_pad // kc) if forced > 0 else pick_splits(P_pad // 128, N_pad // 64, 8, 64, 768)
    else:
        kc = 128 if b <= 32 else 64
        tile = 128 if ((fp32 and b >= 48) or (not fp32 and b == 16)) else 256
        ns = min(forced, N_pad // kc) if forced > 0 else pick_splits(P_pad // tile, N_pad // kc, 4, 64, 768 if (not fp32 and b <= 32) else 512)
    chunks = N_pad // kc
    cps = (chunks + ns - 1) // ns
    if kc == 128:
        cps += cps & 1
    return ns, cps, chunks


def k3_plan(N_pad, P_pad, b, fp32, forced=0, dense=False):
    if dense:
        kc = 64
        ns = min(forced, P_pad // kc) if forced > 0 else pick_splits(N_pad // 256, P_pad // 64, 8, 64, 768)
    else:
        kc = 32 if (fp32 and b >= 48) else 64
        mt = 4 if fp32 else (8 if b <= 32 else 4)
        ns = min(forced, P_pad // kc) if forced > 0 else pick_splits(N_pad // (64 * mt), P_pad // kc, 4, 64, 512)
    chunks = P_pad // kc
    return ns, (chunks + ns - 1) // ns, chunks


def split_chunks(plan):
    ns, cps, chunks = plan
    return [max(0, min(chunks, (i + 1) * cps) - i * cps) for i in range(ns)]


def n_pad(N):
    return 4 * (-(-(-(-N // 4)) // 128) * 128)


def p_pad(P):
    return -(-P // 256) * 256


def pad16(b):
    return -(-b // 16) * 16


# ---------------------------------------------------------------------------------------------------------------------------
# data (host, seeded) and references (computed once per data set, never changed)
def _pack(codes, pad_code):
    """codes [P][N] in 0..3 -> PLINK records: sample 4 i + s in bits 2 s, 2 s + 1 of byte i; pad_code[P] fills the last byte"""
    P, N = codes.shape
    c = np.concatenate([codes, np.repeat(pad_code[:, None], (-N) % 4, axis=1)], axis=1).astype(np.uint8).reshape(P, -1, 4)
    return np.ascontiguousarray(c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6))


def _exact_data(N, P, seed):
    """Codes 0 (dosage 2), 1 (missing, ~2 %), 2 (het, ~30 %), 3 (dosage 0), every SNP repaired to as many 0s as 3s; SNP 1 all het,
    SNP P // 2 all missing, SNP P - 1 monomorphic 0xFF."""
    rng = np.random.default_rng([N, P, seed])
    codes = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), size=(P, N), p=[0.34, 0.02, 0.30, 0.34])
    for j in range(P):
        r = codes[j]
        i0, i3 = np.flatnonzero(r == 0), np.flatnonzero(r == 3)
        big, small_code = (i0, 3) if len(i0) >= len(i3) else (i3, 0)
        d = abs(len(i0) - len(i3))
        pick = rng.permutation(big)[:(d + 1) // 2]
        r[pick[:d // 2]] = small_code
        if d & 1:
            r[pick[-1]] = 2
    special = {"het": 1, "missing": P // 2, "mono": P - 1}
    codes[special["het"]] = 2
    codes[special["missing"]] = 1
    codes[special["mono"]] = 3
    pad = np.zeros(P, dtype=np.uint8)  # pad bits "dosage 2": the upload must rewrite them, or the SNP's mean is no longer 1
    pad[special["mono"]] = 3
    X = np.where(codes == 0, 2, np.where(codes == 3, -2, 0)).astype(np.int64)
    X[special["mono"]] = 0
    assert np.all((codes == 0).sum(axis=1)[:-1] == (codes == 3).sum(axis=1)[:-1])
    return dict(kind="exact", N=N, P=P, codes=codes, packed=_pack(codes, pad), special=special, Xt=X, X=np.ascontiguousarray(X.T))


def _general_data(N, P, seed):
    rng = np.random.default_rng([N, P, seed, 7])
    maf = rng.uniform(0.05, 0.5, size=P)
    g = rng.binomial(2, maf[:, None], size=(P, N))
    codes = np.array([3, 2, 0], dtype=np.uint8)[g]
    codes[rng.random((P, N)) < 0.02] = 1
    return dict(kind="general", N=N, P=P, codes=codes, packed=_pack(codes, np.ones(P, dtype=np.uint8)))


def _operands(d, integer):
    rng = np.random.default_rng([d["N"], d["P"], 99])
    if integer:
        mk = lambda rows: rng.integers(-4, 5, size=(rows, NCOL)).astype(np.float64)
    else:
        mk = lambda rows: rng.standard_normal((rows, NCOL))
    d["B"], d["B2"], d["T"], d["T2"] = mk(d["N"]), mk(d["N"]), mk(d["P"]), mk(d["P"])
    if integer:  # the rows that are used alone must not vanish by chance
        for r in (0, d["N"] - 1):
            d["B"][r] = np.where(d["B"][r] == 0, 3, d["B"][r])


# name -> (maker, N, P, seed); N inside the N_pad step and no multiple of 4 except D3 (N = N_pad); P = P_pad in D2, P_pad - 255 in D1
DATASETS = {
    "D1": (_exact_data, 1001, 513, 1), "D2": (_exact_data, 2307, 1280, 2), "D3": (_exact_data, 1536, 1100, 3),
    "D4": (_exact_data, 1999, 700, 4), "D5": (_exact_data, 8190, 201, 5), "D6": (_exact_data, 509, 4000, 6),
    "D7": (_exact_data, 5001, 3300, 7), "G1": (_general_data, 1001, 513, 8), "G3": (_general_data, 700, 1030, 9),
}
_DATA = {}


def _data(name):
    if name not in _DATA:
        mk, N, P, seed = DATASETS[name]
        d = mk(N, P, seed)
        _operands(d, d["kind"] == "exact")
        _DATA[name] = d
    return _DATA[name]


def _exact_ref(d, ncol):
    """int64 X'B, X T and X X'B for the first ncol operand columns (a narrower block is a column slice of them)"""
    if d.get("ref_ncol", 0) < ncol:
        Bi, Ti = d["B"][:, :ncol].astype(np.int64), d["T"][:, :ncol].astype(np.int64)
        assert np.array_equal(Bi, d["B"][:, :ncol]) and np.array_equal(Ti, d["T"][:, :ncol])
        d["xt"] = d["Xt"] @ Bi
        d["x"] = d["X"] @ Ti
        d["xxt"] = d["X"] @ d["xt"]
        for k in ("xt", "x", "xxt"):
            assert np.max(np.abs(d[k])) < 2 ** 53
        d["ref_ncol"] = ncol
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the child process: runs the contexts of one (FPCA_XT_SPLITS, FPCA_X_SPLITS) setting through the test build
def _child_main(root, in_path, spec_json, out_path):
    import ctypes as C

    sys.path.insert(0, root)
    import flashpca_amd as fp
    from flashpca_amd._lib import check

    data = np.load(in_path)
    out, info = {}, {}
    with fp.test_hooks() as L:
        for c in json.loads(spec_json):
            cid, ds = c["id"], c["data"]
            N, P = int(data[ds + ".shape"][0]), int(data[ds + ".shape"][1])
            if c["dense"]:
                ctx = fp.Context.from_dense(data[ds + ".X"].astype(np.float64), stand="none")
            else:
                ctx = fp.Context.from_packed(data[ds + ".packed"], N, P, stand=c["stand"], accum=c["accum"])
            with ctx:
                out[cid + ".stats"] = ctx.stats()[0]
                B, B2, T, T2 = (data[ds + "." + k] for k in ("B", "B2", "T", "T2"))
                for b in c["widths"]:
                    plan = (C.c_int * 6)()
                    check(L.fpca_debug_fp_plan(ctx.h, b, plan))
                    i = {"plan": list(plan)}
                    for op, f, A, A2 in (("xt", ctx.apply_xt, B, B2), ("x", ctx.apply_x, T, T2), ("xxt", ctx.apply_xxt, B, B2)):
                        R1 = f(A[:, :b])
                        R2 = f(A2[:, :b])
                        check(L.fpca_debug_poison_partials(ctx.h))
                        R3 = f(A[:, :b])
                        out["%s.%d.%s" % (cid, b, op)] = R1
                        i[op + "_finite"] = bool(np.isfinite(R1).all() and np.isfinite(R2).all() and np.isfinite(R3).all())
                        i[op + "_repeat"] = bool(R1.tobytes() == R3.tobytes() and not np.array_equal(R1, R2))
                    if c["rows"]:  # rows 0 and N - 1 of B alone
                        for tag, r in (("r0", 0), ("rl", N - 1)):
                            Br = np.zeros((N, b))
                            Br[r] = B[r, :b]
                            out["%s.%d.xt_%s" % (cid, b, tag)] = ctx.apply_xt(Br)
                            out["%s.%d.xxt_%s" % (cid, b, tag)] = ctx.apply_xxt(Br)
                    info["%s.%d" % (cid, b)] = i
    np.savez(out_path, **out)
    print("CHILD " + json.dumps(info))


_ABNORMAL = []  # a child that died: no further child is started in this session of the module


def _ctx(cid, data, accum="fp64", stand="binom", dense=False, widths=WIDTHS, rows=True):
    return dict(id=cid, data=data, accum=accum, stand=stand, dense=dense, widths=widths, rows=rows)


def _run(contexts, xt_splits, x_splits):
    if _ABNORMAL:
        pytest.fail("not started: an earlier child process of this module died (%s)" % _ABNORMAL[0])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    if xt_splits:
        env["FPCA_XT_SPLITS"] = str(xt_splits)
    if x_splits:
        env["FPCA_X_SPLITS"] = str(x_splits)
    inp = {}
    for name in sorted({c["data"] for c in contexts}):
        d = _data(name)
        inp[name + ".shape"] = np.array([d["N"], d["P"]])
        inp[name + ".packed"] = d["packed"]
        for k in ("B", "B2", "T", "T2"):
            inp[name + "." + k] = d[k]
        if any(c["dense"] and c["data"] == name for c in contexts):
            inp[name + ".X"] = d["X"].astype(np.int8)
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), **inp)
        cmd = [sys.executable, os.path.abspath(__file__), ROOT, os.path.join(tmp, "in.npz"), json.dumps(contexts), os.path.join(tmp, "out.npz")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
        except subprocess.TimeoutExpired as e:
            _ABNORMAL.append("XT=%s X=%s: no result after %d s" % (xt_splits, x_splits, e.timeout))
            pytest.fail(_ABNORMAL[0])
        if r.returncode != 0:
            _ABNORMAL.append("XT=%s X=%s: exit status %d" % (xt_splits, x_splits, r.returncode))
            pytest.fail(_ABNORMAL[0] + "\n" + r.stdout[-2000:] + r.stderr[-3000:])
        info = json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
        with np.load(os.path.join(tmp, "out.npz")) as z:
            res = {k: z[k] for k in z.files}
    print("child XT=%s X=%s: %d contexts, %.1f s" % (xt_splits, x_splits, len(contexts), time.time() - t0))
    return res, info


# ---------------------------------------------------------------------------------------------------------------------------
# checks
def _check_plan(c, info, xt_splits, x_splits, expect):
    """hook == port for every width; expect: {"k2": (narrow list, wide list), "k3": (64-SNP list, 32-SNP list), "tall2"/"tall3": bool}"""
    d = _data(c["data"])
    Np, Pp, fp32 = n_pad(d["N"]), p_pad(d["P"]), c["accum"] == "fp32"
    for b in c["widths"]:
        bw = pad16(b)
        plan = info["%s.%d" % (c["id"], b)]["plan"]
        port2, port3 = k2_plan(Np, Pp, bw, fp32, xt_splits, c["dense"]), k3_plan(Np, Pp, bw, fp32, x_splits, c["dense"])
        assert tuple(plan[:3]) == port2 and tuple(plan[3:]) == port3, (c["id"], b, plan, port2, port3)
        c2, c3 = split_chunks(tuple(plan[:3])), split_chunks(tuple(plan[3:]))
        assert sum(c2) == plan[2] and sum(c3) == plan[5], (c["id"], b, plan)  # the splits cover every chunk
        if expect is None:
            continue
        if "k2" in expect:
            want = expect["k2"][0 if (c["dense"] or bw <= 32) else 1]
            assert c2 == want, (c["id"], b, c2, want)
            assert 0 in c2 or c2[-1] < c2[0] or expect.get("tall2"), (c["id"], b, c2)  # empty or ragged
        if "k3" in expect:
            want = expect["k3"][1 if (fp32 and bw >= 48 and not c["dense"]) else 0]
            assert c3 == want, (c["id"], b, c3, want)
            assert 0 in c3 or c3[-1] < c3[0] or expect.get("tall3"), (c["id"], b, c3)
        if expect.get("tall2"):  # reduce_sum takes k_reduce_tall: nsplit >= 64 and at most 65,536 pairs per plane
            assert plan[0] >= 64 and Pp * bw // 2 <= 65536, (c["id"], b, plan)
        if expect.get("tall3"):
            assert plan[3] >= 64 and Np * bw // 2 <= 65536, (c["id"], b, plan)


def _check_flags(c, info):
    for b in c["widths"]:
        i = info["%s.%d" % (c["id"], b)]
        for op in ("xt", "x", "xxt"):
            assert i[op + "_finite"], (c["id"], b, op, "a NaN: a partial plane or tile of T that nobody wrote")
            assert i[op + "_repeat"], (c["id"], b, op, "the call after the poison differs from the first")


def _check_exact(c, res, info, default=None):
    d = _exact_ref(_data(c["data"]), max(c["widths"]))
    N, P, sp = d["N"], d["P"], d["special"]
    if not c["dense"]:  # the premise: mean 1, sd 0.5 exactly
        ms = res[c["id"] + ".stats"]
        plain = np.ones(P, dtype=bool)
        plain[[sp["missing"], sp["mono"]]] = False
        assert np.all(ms[plain, 0] == 1.0) and np.all(ms[plain, 1] == 0.5), c["id"]
        assert np.isnan(ms[sp["missing"], 0]) and ms[sp["mono"], 0] == 0.0 and ms[sp["mono"], 1] == 0.0, (c["id"], ms[sp["missing"]], ms[sp["mono"]])
    _check_flags(c, info)
    for b in c["widths"]:
        key = "%s.%d." % (c["id"], b)
        if c["accum"] == "fp32":  # the fp32 partial sums of a fold stay exact
            assert 512 * np.max(np.abs(d["xt"][:, :b])) < 2 ** 24 and 512 * np.max(np.abs(d["T"][:, :b])) < 2 ** 24
        for op in ("xt", "x", "xxt"):
            R = res[key + op]
            assert R.shape == d[op][:, :b].shape
            assert np.array_equal(R, d[op][:, :b]), (c["id"], b, op, "max |difference| %g" % np.max(np.abs(R - d[op][:, :b])))
            if default is not None:
                D = default[0][key + op]
                assert R.tobytes() == D.tobytes(), (c["id"], b, op, "differs from the default plan's result")
        if c["rows"]:
            for tag, r in (("r0", 0), ("rl", N - 1)):
                Br = d["B"][r, :b].astype(np.int64)
                want = np.outer(d["X"][r], Br)  # X'B = (row r of X)' (row r of B)
                assert np.any(want != 0)
                assert np.array_equal(res[key + "xt_" + tag], want), (c["id"], b, tag)
                assert np.array_equal(res[key + "xxt_" + tag], np.outer(d["X"] @ d["X"][r], Br)), (c["id"], b, tag)


def _general_ref(d, ms, ncol):
    if "ld" not in d:
        mean, sd = ms[:, 0], ms[:, 1]
        live = sd > 1e-9
        tab = np.zeros((d["P"], 4))
        with np.errstate(invalid="ignore", divide="ignore"):  # make_lut, indexed by raw code
            for code, dosage in ((0, 2.0), (2, 1.0), (3, 0.0)):
                tab[:, code] = np.where(live, (dosage - mean) / np.where(live, sd, 1.0), 0.0)
        Xt = tab[np.arange(d["P"])[:, None], d["codes"]].astype(np.longdouble)  # [P][N]
        X = np.ascontiguousarray(Xt.T)
        B, T = d["B"][:, :ncol].astype(np.longdouble), d["T"][:, :ncol].astype(np.longdouble)
        aXt, aX = np.abs(Xt), np.abs(X)
        xt, axt = Xt @ B, aXt @ np.abs(B)
        d["ld"] = dict(ms=ms, xt=xt, axt=axt, x=X @ T, ax=aX @ np.abs(T), xxt=X @ xt, axxt=aX @ axt)
    assert np.array_equal(d["ld"]["ms"], ms, equal_nan=True)  # every context of this data set has the same statistics
    return d["ld"]


def _check_general(c, res, info):
    d = _data(c["data"])
    ref = _general_ref(d, res[c["id"] + ".stats"], max(c["widths"]))
    _check_flags(c, info)
    g1, g2 = 2.0 * (n_pad(d["N"]) + 4) * U, 2.0 * (p_pad(d["P"]) + 4) * U
    for b in c["widths"]:
        for op, g, a in (("xt", g1, "axt"), ("x", g2, "ax"), ("xxt", g1 + g2 + g1 * g2, "axxt")):
            R = res["%s.%d.%s" % (c["id"], b, op)].astype(np.longdouble)
            want = ref[op][:, :b]
            err = np.abs(R - want)
            if c["accum"] == "fp64":
                bound = g * ref[a][:, :b]
                print("%s b %d %s: max error / bound %.3g" % (c["id"], b, op, float(np.max(err / np.where(bound > 0, bound, 1)))))
                assert np.all(err <= bound), (c["id"], b, op, float(np.max(err - bound)))
            else:
                e = float(np.max(err) / np.max(np.abs(want)))
                print("%s b %d %s: error / output scale %.3g" % (c["id"], b, op, e))
                assert e <= 2e-6, (c["id"], b, op, e)


def _both(cid, data, **kw):
    return [_ctx(cid + "-fp64", data, "fp64", **kw), _ctx(cid + "-fp32", data, "fp32", **kw)]


GEN = dict(stand="binom2", widths=[16, 48], rows=False)
E = [0]
# (FPCA_XT_SPLITS, FPCA_X_SPLITS) -> [(context, expected regime)]
CHILDREN = {
    (3, 5): [(c, dict(k2=([4, 4, 0], [6, 6, 4]), k3=([3, 3, 3, 3, 0], [5, 5, 5, 5, 4]))) for c in _both("D1", "D1") + _both("G1", "G1", **GEN)],
    (3, 6): [(c, dict(k2=([8, 8, 4], [14, 14, 12]), k3=([4] * 5 + E, [7] * 5 + [5]))) for c in _both("D2", "D2")],
    (5, 3): [(c, dict(k2=([4, 4, 4, 0, 0], [5, 5, 5, 5, 4]), k3=([7, 7, 6], [14, 14, 12]))) for c in _both("D3", "D3")]
            + [(_ctx("D3-dense", "D3", dense=True, widths=[16, 32, 48, 64], rows=False), dict(k2=([5, 5, 5, 5, 4],), k3=([7, 7, 6],)))]
            + [(c, dict(k3=([7, 7, 6], [14, 14, 12]))) for c in _both("G3", "G3", **GEN)],
    (7, 7): [(c, dict(k2=([4] * 4 + E * 3, [5] * 6 + [2]), k3=([2] * 6 + E, [4] * 6 + E))) for c in _both("D4", "D4")],
    (64, 64): [(c, dict(k2=([2] * 32 + E * 32, [2] * 64), tall2=True)) for c in _both("D5", "D5")]
              + [(c, dict(k3=([1] * 64, [2] * 64), tall3=True)) for c in _both("D6", "D6")]
              + [(_ctx("D5-dense", "D5", dense=True, widths=[16, 32, 48, 64], rows=False), dict(k2=([2] * 64,), tall2=True)),
                 (_ctx("D6-dense", "D6", dense=True, widths=[16, 32, 48, 64], rows=False), dict(k3=([1] * 64,), tall3=True))],
}
D7 = _ctx("D7-fp64", "D7", "fp64", widths=[16])


@pytest.fixture(scope="module")
def default_plan(built_lib):
    """Every exact context under the plan the library chooses (no override), plus D7, whose default K2 plan has an empty split."""
    ctxs = [c for group in CHILDREN.values() for c, _ in group if _data(c["data"])["kind"] == "exact"] + [D7]
    assert len({c["id"] for c in ctxs}) == len(ctxs)
    res, info = _run(ctxs, 0, 0)
    for c in ctxs:
        _check_plan(c, info, 0, 0, None)
    return res, info


def _forced(xt_splits, x_splits, default):
    group = CHILDREN[(xt_splits, x_splits)]
    res, info = _run([c for c, _ in group], xt_splits, x_splits)
    for c, expect in group:
        _check_plan(c, info, xt_splits, x_splits, expect)
        if _data(c["data"])["kind"] == "exact":
            _check_exact(c, res, info, default)
        else:
            _check_general(c, res, info)


@pytest.mark.gpu
def test_k2_empty_split_k3_empty_split(default_plan):
    """XT=3 / X=5: K2 [4, 4, 0] and [6, 6, 4], K3 [3, 3, 3, 3, 0] and [5, 5, 5, 5, 4]; exact data and the general family."""
    _forced(3, 5, default_plan)


@pytest.mark.gpu
def test_k2_ragged_even_split_k3_six_ways(default_plan):
    """XT=3 / X=6: K2 [8, 8, 4] (ragged, even chunks per split) and [14, 14, 12], K3 [4 x 5, 0] and [7 x 5, 5]; P = P_pad."""
    _forced(3, 6, default_plan)


@pytest.mark.gpu
def test_k2_two_empty_splits_k3_ragged_and_dense(default_plan):
    """XT=5 / X=3: K2 [4, 4, 4, 0, 0] and [5, 5, 5, 5, 4], K3 [7, 7, 6] and [14, 14, 12]; N = N_pad; the dense pair under
    [5, 5, 5, 5, 4] / [7, 7, 6]; the general family under K3 [7, 7, 6]."""
    _forced(5, 3, default_plan)


@pytest.mark.gpu
def test_k2_three_empty_splits_k3_seven_ways(default_plan):
    """XT=7 / X=7: K2 [4, 4, 4, 4, 0, 0, 0] and [5 x 6, 2], K3 [2 x 6, 0] and [4 x 6, 0]: reduce_sum's 3 leftover planes."""
    _forced(7, 7, default_plan)


@pytest.mark.gpu
def test_64_splits_reduce_tall(default_plan):
    """XT=64 / X=64: 64 planes (half of them empty for K2 at 16 / 32 columns) combined by k_reduce_tall; packed and dense."""
    _forced(64, 64, default_plan)


@pytest.mark.gpu
def test_default_plan_with_an_empty_k2_split(default_plan):
    """N_pad 5120 x P_pad 3328, fp64, 16 columns: the plan the library picks by itself is [6, 6, 6, 6, 6, 6, 4, 0] (40 chunks, 8 splits,
    5 -> 6 chunks per split).  The other default-plan contexts are checked against int64 as well."""
    res, info = default_plan
    plan = info["D7-fp64.16"]["plan"]
    assert split_chunks(tuple(plan[:3])) == [6] * 6 + [4, 0], plan
    _check_exact(D7, res, info)
    for group in CHILDREN.values():
        for c, _ in group:
            if _data(c["data"])["kind"] == "exact":
                _check_exact(c, res, info)


def test_plan_port_reproduces_the_tables():
    """No GPU: the port gives the chunk lists the cases are named for, every forced case is ragged, empty or tall, the other operator
    tests' shapes are neither, and D7 is the smallest shape whose default K2 plan has an empty split."""
    for (xs, ks), group in CHILDREN.items():
        for c, expect in group:
            d = DATASETS[c["data"]]
            Np, Pp, fp32 = n_pad(d[1]), p_pad(d[2]), c["accum"] == "fp32"
            for b in c["widths"]:
                bw = pad16(b)
                c2, c3 = split_chunks(k2_plan(Np, Pp, bw, fp32, xs, c["dense"])), split_chunks(k3_plan(Np, Pp, bw, fp32, ks, c["dense"]))
                if "k2" in expect:
                    assert c2 == expect["k2"][0 if (c["dense"] or bw <= 32) else 1], (c["id"], b, c2)
                if "k3" in expect:
                    assert c3 == expect["k3"][1 if (fp32 and bw >= 48 and not c["dense"]) else 0], (c["id"], b, c3)
    # what the other operator tests reach (test_ragged_shapes_vs_oracle, the synthetic 3000 x 700; test_gpu_dense.py): every split has
    # exactly 4 chunks (dense: 8)
    for N, P in ((3000, 700), (1, 3), (5, 7), (64, 1), (257, 300), (1000, 513), (2051, 129)):
        for b in (16, 32, 48, 64):
            for fp32 in (False, True):
                for pl in (k2_plan(n_pad(N), p_pad(P), b, fp32), k3_plan(n_pad(N), p_pad(P), b, fp32)):
                    assert set(split_chunks(pl)) == {4}, (N, P, b, fp32, pl)
    for N, P in ((700, 300), (500, 1000)):
        for pl in (k2_plan(n_pad(N), p_pad(P), 16, False, 0, True), k3_plan(n_pad(N), p_pad(P), 16, False, 0, True)):
            assert set(split_chunks(pl)) == {8}, (N, P, pl)
    # production: 50,000 x 20,000, K3 fp64: ragged last split
    assert split_chunks(k3_plan(n_pad(50000), p_pad(20000), 16, False))[-1] < split_chunks(k3_plan(n_pad(50000), p_pad(20000), 16, False))[0]
    assert split_chunks(k2_plan(3072, 25600, 32, False)) == [6, 6, 6, 6, 0]
    best = min((Np * Pp, Np, Pp, b, fp32) for Np in range(512, 8193, 512) for Pp in range(256, 8193, 256) for b in (16, 32) for fp32 in (False, True)
               if 0 in split_chunks(k2_plan(Np, Pp, b, fp32)))
    assert best == (5120 * 3328, 5120, 3328, 16, False) and (n_pad(DATASETS["D7"][1]), p_pad(DATASETS["D7"][2])) == (5120, 3328), best
    assert split_chunks(k2_plan(5120, 3328, 16, False)) == [6] * 6 + [4, 0]


if __name__ == "__main__":
    _child_main(*sys.argv[1:5])
