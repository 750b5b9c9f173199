"""The relationship matrix (fpca_grm_block / fpca_grm_tri / fpca_grm_pairs / fpca_grm_cutoff; Context.grm_block / grm_tri / grm_pairs /
grm_cutoff, grm(), rel_cutoff(), write_grm / read_grm) on the GPU against a numpy yardstick that never calls the feature.  The yardstick
unpacks the raw 2-bit codes, takes mean / sd from Context.stats() and restates include/fpca.h:
   t_s[code] = (x - mean_s) / sd_s at a call, 0 at a missing call, all four 0 when sd_s <= 1e-9 or NaN; a SNP is live when its table is not
   all zero; z_is = t_s[code_is]; S_ij = sum_s z_is z_js; n_ij = the live SNPs called in both; G = S / n (NaN when n == 0), S / P or S --
   ONE fp64 divide; a NaN is never above a threshold, comparisons are strict.
1. Bit for bit.  Data with as many dosage-2 as dosage-0 calls per SNP among the called samples has, under stand="binom", mean 1, sd 0.5 and
   the table {2, 0, 0, -2} (tests/test_gpu_fp_splits.py): S is an integer below 2^53 under any order of the sum, so every value must be
   array_equal (NaN = NaN) to int64 numpy divided once.
2. Ordinary genotypes (binom2) against np.longdouble sums: |S_gpu - S_ld| <= (4 pitch + 8) 2^-53 sum_s |z_is| |z_js| per pair -- the forward
   bound of a sum of 4 pitch terms in any order, the 8 for one rounding each in the table entries and the product -- and
   |G - G_ld| <= that / n + 2^-53 |G_ld|.  DIV_NONE against Context.apply_xxt of identity columns: two routes, each within the bound, so
   the difference is within twice the bound.
3. Lists and the rule: a pair whose longdouble value clears the threshold by more than its bound must be listed, one below by more must
   not; the thresholds were chosen on the CPU so that no pair lies inside the band, and the test asserts the band is empty.
4. Golden filesets against float64 BLAS sums at twice the bound (both sides within one bound of the truth).
5. Refusals.
Shapes (tests/test_gpu_king.py's): 70 x 300 one chunk, mostly pad slots, a ragged second tile; 130 x 1000; 257 x 2100 pitch rounded 576 ->
640, five chunks, five tiles.  The data holds duplicates, one sample without any call, missing rates 0 / 1 % / 20 % by 32-sample block (whole
blocks take the no-product count path), two monomorphic SNPs and one SNP without any call (not live).
Every test prints what it measured (pytest -s).
Measured on the MI355X (profiles/grm_test_figures.txt): the balanced data equals int64 numpy bit for bit -- the square, six rectangles, the
triangle and the counts on each of the three shapes under all three divisors -- and slabs of 64 / 128 rows and the forced count product
change no bit; ordinary genotypes: the largest error is 0.009 - 0.021 of the bound at every shape and divisor, apply_xxt of identity
columns within 0.021 of it (2 allowed); no pair inside the band at 0.025 / 0.3 / -0.08 (3 shapes x 2 divisors x {all, 30 % pre-cleared}),
every list, count and mask equal to the restatement's; hapmap3_data and data_chr1 within 0.008 / 0.016 of the bound (2 allowed),
diagonal means 1.0365 / 1.0332, the pair counts of GOLDEN; 7 - 12 scratch acquisitions per entry point, all given back on every injected
failure.  The 14 tests take 3.6 s together."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENOMEM = -4
U = 2.0 ** -53
DIVISORS = ("shared", "p", "none")


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


# ---- data ------------------------------------------------------------------------------------------------------
def pack_codes(codes):
    """codes: (P, N) raw PLINK 2-bit codes -> the packed records."""
    P, N = codes.shape
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    return (c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)).astype(np.uint8)


def unpack_codes(packed, N, P):
    packed = np.asarray(packed, dtype=np.uint8).reshape(P, -1)
    return np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(P, -1)[:, :N]


def read_bed_codes(prefix):
    N = open(prefix + ".fam", "rb").read().count(b"\n")
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:]
    P = raw.size // ((N + 3) // 4)
    return unpack_codes(raw, N, P), N, P


NOCALL = 44          # the sample without any call
SPECIAL = (3, 7, 11)  # SNPs: monomorphic (all dosage 0), monomorphic (all dosage 2), without any call


def missing_rate(N):
    """Sample s of an even 32-sample block has no missing call; in the odd blocks every fourth sample has 1 % and every eighth 20 %."""
    s = np.arange(N)
    odd = (s // 32) % 2 == 1
    rate = np.where(odd & (s % 4 == 0), 0.01, 0.0)
    return np.where(odd & (s % 8 == 4), 0.20, rate)


def pedigree_codes(N, P, seed):
    """(P, N) codes in the manner of tests/test_gpu_king.py: founders, a trio with a full sib, duplicates (one pair across the whole range,
    one of which one copy has missing calls), the missing rates above, sample 44 without any call; plus the three SPECIAL SNPs."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, P)
    d = rng.binomial(2, p[None, :], (N, P))

    def child(a, b):
        return rng.binomial(1, d[a] / 2.0) + rng.binomial(1, d[b] / 2.0)

    d[2], d[3] = child(0, 1), child(0, 1)
    d[40], d[41] = child(33, 36), child(33, 36)
    d[5] = d[4]
    d[N - 1] = d[6]
    d[48] = d[7]
    codes = np.array([3, 2, 0], dtype=np.uint8)[d]  # (N, P)
    codes[rng.random((N, P)) < missing_rate(N)[:, None]] = 1
    codes[NOCALL] = 1
    codes[:, SPECIAL[0]] = np.where(codes[:, SPECIAL[0]] == 1, 1, 3)
    codes[:, SPECIAL[1]] = np.where(codes[:, SPECIAL[1]] == 1, 1, 0)
    codes[:, SPECIAL[2]] = 1
    return np.ascontiguousarray(codes.T)


def balanced_codes(N, P, seed):
    """(P, N) codes in which every SNP but the SPECIAL three has as many dosage-2 as dosage-0 calls among its called samples: under
    stand="binom" mean 1, sd 0.5, table {2, 0, 0, -2}.  The same missing pattern; SNP 13 is all heterozygous (live, every z = 0)."""
    rng = np.random.default_rng(seed)
    codes = np.empty((P, N), dtype=np.uint8)
    miss = rng.random((P, N)) < missing_rate(N)[None, :]
    miss[:, NOCALL] = True
    for s in range(P):
        called = np.flatnonzero(~miss[s])
        rng.shuffle(called)
        pairs = rng.integers(0, called.size // 2 + 1)  # that many dosage-2 and as many dosage-0 calls; the rest heterozygous
        row = np.full(N, 1, dtype=np.uint8)
        row[called] = 2
        row[called[:pairs]] = 0
        row[called[pairs:2 * pairs]] = 3
        codes[s] = row
    codes[13] = np.where(miss[13], 1, 2)
    codes[SPECIAL[0]] = np.where(miss[SPECIAL[0]], 1, 3)
    codes[SPECIAL[1]] = np.where(miss[SPECIAL[1]], 1, 0)
    codes[SPECIAL[2]] = 1
    return codes


SHAPES = {"70x300": (70, 300, 1), "130x1000": (130, 1000, 2), "257x2100": (257, 2100, 3)}


def pitch_of(P):
    """Bytes of a record of the sample-major copy: round_up(P_pad / 4, 128), P_pad = round_up(P, 256)."""
    return ((P + 255) // 256 * 256 // 4 + 127) // 128 * 128


# ---- the yardstick -------------------------------------------------------------------------------------------------
def z_matrix(codes, ms):
    """(z, m): z[i][s] = the table entry of sample i at SNP s from mean / sd (float64, the formula of include/fpca.h), m = 1 where a live
    SNP is called."""
    mean, sd = ms[:, 0], ms[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = sd > 1e-9  # (NaN: False)
        table = np.stack([(2.0 - mean) / sd, np.zeros_like(mean), (1.0 - mean) / sd, (0.0 - mean) / sd], axis=1)  # by raw code
    table[~ok] = 0.0
    live = np.any(table != 0.0, axis=1)
    z = np.take_along_axis(table, codes.astype(np.int64), axis=1).T  # (N, P)
    m = ((codes != 1) & live[:, None]).T.astype(np.float64)
    return np.ascontiguousarray(z), m, live


def divide(S, n, P, divisor):
    """G from float64 S: ONE divide by the integer converted to double."""
    if divisor == "none":
        return S.copy()
    if divisor == "p":
        return S / float(P)
    with np.errstate(invalid="ignore", divide="ignore"):
        G = S / n.astype(np.float64)
    G[n == 0] = np.nan
    return G


def reference(codes, ms, longdouble):
    """S (longdouble or float64 BLAS sums), n (int64), the per-pair bound (4 pitch + 8) 2^-53 sum |z_i| |z_j|."""
    z, m, live = z_matrix(codes, ms)
    P = codes.shape[0]
    n = (m @ m.T).astype(np.int64)
    if longdouble:
        zl = z.astype(np.longdouble)
        S = zl @ zl.T
        A = np.abs(zl) @ np.abs(zl).T
    else:
        S = z @ z.T
        A = np.abs(z) @ np.abs(z).T
    bound = (4 * pitch_of(P) + 8) * U * A.astype(np.float64) * (1.0 + 1e-9)  # (the bound's own rounding is not counted against the device)
    return dict(z=z, S=S, n=n, bound=bound, live=live, P=P, N=codes.shape[1])


def g_reference(ref, divisor):
    """(G in the precision of ref["S"], its band: bound / divisor + 2^-53 |G|)."""
    S, n, P = ref["S"], ref["n"], ref["P"]
    one = S.dtype.type(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if divisor == "none":
            G, band = S, ref["bound"]
        elif divisor == "p":
            G = S / (one * P)
            band = ref["bound"] / P + U * np.abs(G).astype(np.float64)
        else:
            G = S / n.astype(S.dtype)
            band = ref["bound"] / n + U * np.abs(G).astype(np.float64)
            G = np.where(n == 0, np.nan, G)
            band = np.where(n == 0, 0.0, band)
    return G, band


def within(got, G, band, factor=1.0):
    """Every entry of got within factor x band of G, NaN exactly where G is; returns (ok, the largest error / band)."""
    nan_ok = np.array_equal(np.isnan(got), np.isnan(G.astype(np.float64)))
    err = np.abs(got.astype(G.dtype) - G).astype(np.float64)
    f = np.isfinite(err)
    ok = nan_ok and bool(np.all(err[f] <= factor * band[f]))
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(band > 0, err / band, 0.0))) if f.any() else 0.0
    return ok, worst


def classify(G, band, thr, keep=None, factor=1.0):
    """(must, band_count): must[i][j], i < j, for the pairs that clear thr by more than factor x band; the pairs of kept samples that are
    neither clearly above nor clearly below (NaN: below)."""
    N = G.shape[0]
    G64, b = G.astype(np.float64), factor * band
    with np.errstate(invalid="ignore"):
        above = (G - thr).astype(np.float64) > b
        below = ((thr - G).astype(np.float64) > b) | np.isnan(G64)
    up = np.triu(np.ones((N, N), dtype=bool), 1)
    if keep is not None:
        up &= keep[:, None] & keep[None, :]
    return above & up, int((up & ~above & ~below).sum())


def cutoff_rule(A, keep=None):
    """The rule of include/fpca.h on the edges A (any triangle): while an edge remains the sample of largest current degree goes, the
    largest index among equals."""
    N = A.shape[0]
    keep = np.ones(N, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    A = (A | A.T) & keep[:, None] & keep[None, :]
    deg = A.sum(axis=1)
    while deg.max() > 0:
        v = N - 1 - int(np.argmax(deg[::-1]))
        keep[v] = False
        deg -= A[:, v]
        A[v, :] = A[:, v] = False
        deg[v] = 0
    return keep


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def rectangles(N):
    """Six rectangles off the 64-sample tiles and the 32-sample blocks; three reach below the diagonal, one is a single pair."""
    return [(5, 40, 3, N - 10), (33, N - 33, 0, 31), (N - 7, 7, N - 10, 10), (0, 1, N - 1, 1), (N - 1, 1, 0, N), (31, 34, 31, 34)]


def pack_tri(M):
    return np.ascontiguousarray(M[np.tril_indices(M.shape[0])])


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------
_EXACT = {}


def exact_case(name):
    if name not in _EXACT:
        N, P, seed = SHAPES[name]
        codes = balanced_codes(N, P, seed + 10)
        plain = np.ones(P, dtype=bool)
        plain[list(SPECIAL)] = False
        Z = np.array([2, 0, 0, -2], dtype=np.int64)[codes].T * plain[None, :]  # (N, P)
        M = ((codes != 1).T & plain[None, :]).astype(np.int64)
        S, n = Z @ Z.T, M @ M.T
        assert np.abs(S).max() < 2 ** 53 and n[NOCALL].max() == 0 and n.max() == P - 3
        G = {d: divide(S.astype(np.float64), n, P, d) for d in DIVISORS}
        _EXACT[name] = dict(N=N, P=P, codes=codes, packed=pack_codes(codes), plain=plain, S=S, n=n.astype(np.uint32), G=G)
    return _EXACT[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_data_bit_for_bit(fp, name):
    c = exact_case(name)
    N, P = c["N"], c["P"]
    with fp.Context.from_packed(c["packed"], N, P, stand="binom") as ctx:
        ms = ctx.stats()[0]
        assert np.all(ms[c["plain"], 0] == 1.0) and np.all(ms[c["plain"], 1] == 0.5)  # the premise: table {2, 0, 0, -2}
        assert ms[SPECIAL[0], 1] == 0.0 and ms[SPECIAL[1], 1] == 0.0 and np.isnan(ms[SPECIAL[2], 0])
        for d in DIVISORS:
            got, cnt = ctx.grm_block(0, N, 0, N, divisor=d, counts=True)
            eq, eqn, sym = same(got, c["G"][d]), same(cnt, c["n"]), np.array_equal(got, got.T, equal_nan=True)
            print("%s binom grm_block(0, %d, 0, %d, %s): %d finite, %d NaN; equal to int64 numpy bit for bit: %s, shared equal: %s, equal to its "
                  "transpose: %s" % (name, N, N, d, np.isfinite(got).sum(), np.isnan(got).sum(), eq, eqn, sym))
            assert eq and eqn and sym, (name, d, np.argwhere(~((got == c["G"][d]) | (np.isnan(got) & np.isnan(c["G"][d]))))[:5])
            again = ctx.grm_block(0, N, 0, N, divisor=d)
            assert same(again, got), "two calls differ"
            assert same(ctx.grm_block(0, N, 0, N, divisor=d), got)  # (without the counts: the count kernel runs only under "shared")
            tri, tcnt = ctx.grm_tri(divisor=d, counts=True)
            assert same(tri, pack_tri(c["G"][d])) and same(tcnt, pack_tri(c["n"])), (name, d, "grm_tri")
            assert same(ctx.grm_tri(divisor=d), tri)
            for i0, ni, j0, nj in rectangles(N):
                got, cnt = ctx.grm_block(i0, ni, j0, nj, divisor=d, counts=True)
                eq = same(got, np.ascontiguousarray(c["G"][d][i0:i0 + ni, j0:j0 + nj])) and same(cnt, np.ascontiguousarray(c["n"][i0:i0 + ni, j0:j0 + nj]))
                print("%s binom grm_block(%d, %d, %d, %d, %s): equal to numpy bit for bit: %s" % (name, i0, ni, j0, nj, d, eq))
                assert eq, (name, d, i0, ni, j0, nj)
        # the sample without a call: NaN under "shared", 0 under the others; a diagonal entry is sum z^2 / its calls
        assert np.isnan(ctx.grm_block(NOCALL, 1, 0, N)).all() and np.all(ctx.grm_block(NOCALL, 1, 0, N, divisor="p") == 0.0)


_SLAB_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
d = np.load(sys.argv[2])
out = {}
with fp.test_hooks():
    with fp.Context.from_packed(d["packed"], int(d["N"]), int(d["P"]), stand="binom") as ctx:
        for rows in json.loads(sys.argv[3]):
            if rows:
                os.environ["FPCA_GRM_SLAB_ROWS"] = str(rows)
            else:  # 0: default slabs, the count kernel's product forced where the no-product path would run
                del os.environ["FPCA_GRM_SLAB_ROWS"]
                os.environ["FPCA_GRM_FORCE_GENERAL"] = "1"
            for div in ("shared", "p", "none"):
                tri, cnt = ctx.grm_tri(divisor=div, counts=True)
                blk, bcnt = ctx.grm_block(0, int(d["N"]), 0, int(d["N"]), divisor=div, counts=True)
                i, j, g, sh = ctx.grm_pairs(float(d["thr"]), divisor=div)
                for k, v in (("tri", tri), ("cnt", cnt), ("blk", blk), ("bcnt", bcnt), ("i", i), ("j", j), ("g", g), ("sh", sh)):
                    out["%d.%s.%s" % (rows, div, k)] = v
            out["%d.keep" % rows] = ctx.grm_cutoff(float(d["thr"]))
np.savez(sys.argv[4], **out)
print("CHILD ok")
"""


def test_slabs_change_no_bit(fp):
    """FPCA_GRM_SLAB_ROWS (test build) = 64 and 128 in a child process: slabs of one and two row tiles -- five and three launches over the
    257 samples where the default is one -- give the triangle, the square, the list and the mask of the default, bit for bit; so does
    FPCA_GRM_FORCE_GENERAL=1, the e.e product where the count kernel would store the live count without one (the even 32-sample blocks
    hold no missing call)."""
    c = exact_case("257x2100")
    N, P, thr = c["N"], c["P"], 0.0625
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(src, packed=c["packed"], N=N, P=P, thr=thr)
        r = subprocess.run([sys.executable, "-c", _SLAB_CHILD, ROOT, src, json.dumps([64, 128, 0]), out], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0 and "CHILD ok" in r.stdout, r.stderr[-2000:]
        res = dict(np.load(out))
    with fp.Context.from_packed(c["packed"], N, P, stand="binom") as ctx:
        for d in DIVISORS:
            tri, cnt = ctx.grm_tri(divisor=d, counts=True)
            lst = ctx.grm_pairs(thr, divisor=d)
            assert same(tri, pack_tri(c["G"][d])) and lst[0].size > 0
            for rows in (64, 128, 0):
                key = "%d.%s." % (rows, d)
                eq = (same(res[key + "tri"], tri) and same(res[key + "cnt"], cnt) and same(res[key + "blk"], c["G"][d]) and same(res[key + "bcnt"], c["n"])
                      and all(same(res[key + k], v) for k, v in zip(("i", "j", "g", "sh"), lst)))
                print("%s, divisor %s: triangle, square, counts and the %d pairs above %g equal to the default's bit for bit: %s" % (
                    "slabs of %d rows" % rows if rows else "default slabs with the count product forced", d, lst[0].size, thr, eq))
                assert eq, (rows, d)
        keep = ctx.grm_cutoff(thr)
        assert same(res["64.keep"], keep) and same(res["128.keep"], keep) and same(res["0.keep"], keep)


# ---- 2. ordinary genotypes -------------------------------------------------------------------------------------------
_CASE = {}


def case(fp, name):
    """One generated shape under binom2: codes, the context's own mean / sd, the longdouble sums -- computed once and left unchanged."""
    if name not in _CASE:
        N, P, seed = SHAPES[name]
        codes = pedigree_codes(N, P, seed)
        packed = pack_codes(codes)
        with fp.Context.from_packed(packed, N, P) as ctx:
            ms = ctx.stats()[0].copy()
        ref = reference(codes, ms, longdouble=True)
        assert not ref["live"][list(SPECIAL)].any() and ref["live"].sum() == P - 3
        _CASE[name] = dict(N=N, P=P, codes=codes, packed=packed, ms=ms, ref=ref)
    return _CASE[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_ordinary_genotypes_within_the_bound(fp, name):
    c = case(fp, name)
    N, P, ref = c["N"], c["P"], c["ref"]
    n32 = ref["n"].astype(np.uint32)
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        S_gpu = None
        for d in DIVISORS:
            G, band = g_reference(ref, d)
            got, cnt = ctx.grm_block(0, N, 0, N, divisor=d, counts=True)
            ok, worst = within(got, G, band)
            print("%s binom2 grm_block %s: largest |G - G_longdouble| / bound %.3f (bound: (4 x %d + 8) 2^-53 sum |z||z| / divisor + 2^-53 |G|); "
                  "shared equal: %s; symmetric bit for bit: %s" % (name, d, worst, pitch_of(P), same(cnt, n32), np.array_equal(got, got.T, equal_nan=True)))
            assert ok and same(cnt, n32), (name, d, worst)
            assert np.array_equal(got, got.T, equal_nan=True)
            if d == "shared":
                assert np.isnan(got[NOCALL]).all() and np.isnan(got[:, NOCALL]).all() and np.isfinite(np.delete(np.delete(got, NOCALL, 0), NOCALL, 1)).all()
                dg = np.delete(np.diag(got), NOCALL)
                print("%s: diagonal mean %.6f, duplicates G[4][5] %.6f G[6][N-1] %.6f, parent-offspring G[0][2] %.6f, founders G[0][1] %.6f" % (
                    name, dg.mean(), got[4, 5], got[6, N - 1], got[0, 2], got[0, 1]))
                assert got[4, 5] > 0.8 and got[6, N - 1] > 0.8 and 0.25 < got[0, 2] < 0.75 and abs(got[0, 1]) < 0.25
            else:
                assert np.all(got[NOCALL] == 0.0) and np.all(got[:, NOCALL] == 0.0)
            if d == "none":
                S_gpu = got
            tri = ctx.grm_tri(divisor=d)
            assert same(tri, pack_tri(got))  # the triangle is the square, bit for bit
            for i0, ni, j0, nj in rectangles(N):
                assert same(ctx.grm_block(i0, ni, j0, nj, divisor=d), np.ascontiguousarray(got[i0:i0 + ni, j0:j0 + nj])), (name, d, i0, ni, j0, nj)
        # the operator's own route to the same sums: X X' e_j for every j, 16 columns at a time
        Y = np.empty((N, N))
        for j0 in range(0, N, 16):
            B = np.zeros((N, min(16, N - j0)))
            B[np.arange(j0, j0 + B.shape[1]), np.arange(B.shape[1])] = 1.0
            Y[:, j0:j0 + B.shape[1]] = ctx.apply_xxt(B)
        diff = np.abs(Y - S_gpu)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = float(np.nanmax(np.where(ref["bound"] > 0, diff / ref["bound"], 0.0)))
        print("%s: DIV_NONE against apply_xxt of identity columns: largest difference / bound %.3f (allowed 2)" % (name, worst))
        assert np.all(diff <= 2.0 * ref["bound"])


# ---- 3. lists and the rule -------------------------------------------------------------------------------------------
# chosen on the CPU: no pair of the three shapes lies within its bound of one of these
THRESHOLDS = (0.025, 0.3, -0.08)


@pytest.mark.parametrize("name", list(SHAPES))
def test_pairs_and_cutoff(fp, name, monkeypatch):
    c = case(fp, name)
    N, P, ref = c["N"], c["P"], c["ref"]
    pre = np.random.default_rng(7).random(N) >= 0.3  # a pre-cleared random 30 %
    pre[[0, 2, 4, 5]] = True
    pre[3] = False
    counts = []
    with fp.Context.from_packed(c["packed"], N, P, accum="auto") as ctx:
        B = np.random.default_rng(4).standard_normal((N, 16))
        before = ctx.apply_xt(B)
        for d in ("shared", "p"):
            G, band = g_reference(ref, d)
            G64 = G.astype(np.float64)
            for thr in THRESHOLDS:
                for label, keep in (("all", None), ("70%", pre)):
                    must, inside = classify(G, band, thr, keep)
                    wi, wj = np.nonzero(must)  # row-major: sorted by (i, j)
                    i, j, g, sh = ctx.grm_pairs(thr, keep=keep, divisor=d)
                    eq = same(i, wi.astype(np.uint32)) and same(j, wj.astype(np.uint32))
                    val = eq and bool(np.all(np.abs(g - G64[wi, wj]) <= band[wi, wj])) and same(sh, ref["n"][wi, wj].astype(np.uint32))
                    wmask, gmask = cutoff_rule(must, keep), ctx.grm_cutoff(thr, keep=keep, divisor=d)
                    print("%s %s thr %g keep=%s: %d pairs inside the band; yardstick lists %d pairs, the device %d, lists equal: %s, values within the "
                          "bound and shared equal: %s; cutoff keeps %d and %d of %d, masks equal: %s" % (
                              name, d, thr, label, inside, wi.size, i.size, eq, val, wmask.sum(), gmask.sum(), N, np.array_equal(gmask, wmask)))
                    assert inside == 0, (name, d, thr, label)
                    assert eq and val, (name, d, thr, label)
                    assert gmask.dtype == np.bool_ and np.array_equal(gmask, wmask), (name, d, thr, label)
                    if keep is not None:
                        assert not gmask[~pre].any() and pre[i].all() and pre[j].all()  # a cleared sample never comes back
                        assert not ((i == 2) & (j == 3)).any()
                    elif d == "shared":
                        counts.append(wi.size)
        after = ctx.apply_xt(B)
        assert np.array_equal(before, after)  # the context computes what it computed
        # overflow: -4 with the count, in the message and in *n_pairs
        need = counts[0]
        assert need > 3
        with pytest.raises(fp.FpcaError, match="%d pairs are above the threshold, the arrays hold 3" % need) as e:
            ctx.grm_pairs(THRESHOLDS[0], max_pairs=3)
        assert e.value.code == ENOMEM
        import ctypes as C

        nn = C.c_uint64(0)
        a3, b3, g3 = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32), np.zeros(3)
        rc = fp.lib().fpca_grm_pairs(ctx.h, None, THRESHOLDS[0], 0, 3, a3.ctypes.data, b3.ctypes.data, g3.ctypes.data, None, C.byref(nn))
        assert rc == ENOMEM and nn.value == need
        a, b, g = np.zeros(need, dtype=np.uint32), np.zeros(need, dtype=np.uint32), np.zeros(need)
        rc = fp.lib().fpca_grm_pairs(ctx.h, None, THRESHOLDS[0], 0, need, a.ctypes.data, b.ctypes.data, g.ctypes.data, None, C.byref(nn))
        assert rc == 0 and nn.value == need  # exactly enough room, no counts asked for
        print("%s overflow: %d pairs needed against 3: refused with the count; served with room for %d" % (name, need, need))
    # the cutoff's own room (2^26 pairs; the test build takes another from FPCA_GRM_MAX_PAIRS): refused with the count, a shorter list served
    with fp.test_hooks():
        monkeypatch.setenv("FPCA_GRM_MAX_PAIRS", "20")
        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            with pytest.raises(fp.FpcaError, match="%d pairs are above the threshold, the call keeps room for 20" % need) as e:
                ctx.grm_cutoff(THRESHOLDS[0])
            assert e.value.code == ENOMEM
            must = classify(*g_reference(ref, "shared"), THRESHOLDS[1])[0]
            assert must.sum() <= 20 and np.array_equal(ctx.grm_cutoff(THRESHOLDS[1]), cutoff_rule(must))
        monkeypatch.delenv("FPCA_GRM_MAX_PAIRS")
    # the cases are not vacuous: the close relatives only; then more; then most pairs that have a value
    assert 3 <= counts[1] < counts[0] < counts[2], counts
    i, j = np.nonzero(classify(*g_reference(ref, "shared"), 0.3)[0])
    assert ((i == 4) & (j == 5)).any() and ((i == 0) & (j == 2)).any() and ((i == 6) & (j == N - 1)).any()


# ---- 4. golden filesets ----------------------------------------------------------------------------------------------
# pairs i < j above 0.025 / 0.05 / 0.125 under binom2 / "shared", recorded on the CPU from the restatement
GOLDEN = {
    "hapmap3_data": ((957, 14389), {0.025: 112289, 0.05: 70595, 0.125: 285}),
    "data_chr1": ((957, 1129), {0.025: 126103, 0.05: 74745, 0.125: 3856}),
}
_GOLD = {}


def golden(fp, name):
    if name not in _GOLD:
        codes, N, P = read_bed_codes(os.path.join(GOLD, name))
        with fp.Context.from_bed(os.path.join(GOLD, name + ".bed"), N) as ctx:
            ms = ctx.stats()[0].copy()
        _GOLD[name] = dict(codes=codes, N=N, P=P, ms=ms, ref=reference(codes, ms, longdouble=False))
    return _GOLD[name]


@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_filesets(fp, name, tmp_path):
    g = golden(fp, name)
    (N, P), table = GOLDEN[name]
    assert (g["N"], g["P"]) == (N, P)
    ref, prefix = g["ref"], os.path.join(GOLD, name)
    G, band = g_reference(ref, "shared")
    with fp.Context.from_bed(prefix + ".bed", N, accum="auto") as ctx:
        tri, cnt = ctx.grm_tri(counts=True)
        ok, worst = within(tri, pack_tri(G), pack_tri(band), factor=2.0)
        dg = tri[np.arange(N) * (np.arange(N) + 3) // 2]
        print("%s: %d x %d, %d live SNPs; triangle against float64 BLAS sums: largest error / bound %.3f (allowed 2); shared equal: %s; diagonal "
              "mean %.6f, off-diagonal mean %.3e" % (name, N, P, ref["live"].sum(), worst, same(cnt, pack_tri(ref["n"]).astype(np.uint32)), dg.mean(),
                                                  (tri.sum() - dg.sum()) / (tri.size - N)))
        assert ok and same(cnt, pack_tri(ref["n"]).astype(np.uint32)), (name, worst)
        assert 0.9 < dg.mean() < 1.1
        for thr, npairs in table.items():
            must, inside = classify(G, band, thr, factor=2.0)
            wi, wj = np.nonzero(must)
            i, j, gg, sh = ctx.grm_pairs(thr)
            gmask, wmask = ctx.grm_cutoff(thr), cutoff_rule(must)
            print("%s thr %g: %d pairs inside the band; yardstick %d pairs / %d kept, the device %d / %d" % (
                name, thr, inside, wi.size, wmask.sum(), i.size, gmask.sum()))
            assert inside == 0 and wi.size == npairs, (name, thr, wi.size)
            assert same(i, wi.astype(np.uint32)) and same(j, wj.astype(np.uint32)) and np.array_equal(gmask, wmask), (name, thr)
            assert same(gg, tri[wj.astype(np.int64) * (wj + 1) // 2 + wi]) and same(sh, cnt[wj.astype(np.int64) * (wj + 1) // 2 + wi])  # the list holds the triangle's own bits
    # rel_cutoff() after a MAF filter: the yardstick on the kept SNPs (their mean / sd are over all samples either way)
    maf = np.minimum(g["ms"][:, 0] / 2.0, 1.0 - g["ms"][:, 0] / 2.0)
    snps = ~(np.nan_to_num(maf, nan=0.0) < 0.05)
    sub = reference(g["codes"][snps], g["ms"][snps], longdouble=False)
    must, inside = classify(*g_reference(sub, "shared"), 0.025, factor=2.0)
    want = cutoff_rule(must)
    mask = fp.rel_cutoff(prefix, 0.025, maf=0.05)
    print("%s rel_cutoff(0.025, maf=0.05): %d of %d SNPs, %d pairs inside the band, %d pairs above; keeps %d of %d samples, the yardstick %d, masks equal: %s" % (
        name, snps.sum(), P, inside, must.sum(), mask.sum(), N, want.sum(), np.array_equal(mask, want)))
    assert inside == 0 and 0 < snps.sum() < P and mask.dtype == np.bool_ and np.array_equal(mask, want) and 0 < want.sum() < N
    r = fp.flashpca(prefix, ndim=3, keep=mask)  # the mask is what flashpca(keep=) takes
    assert r["vectors"].shape == (int(mask.sum()), 3) and r["projection_all"].shape == (N, 3)
    # grm() -> write_grm -> read_grm: GCTA's files hold the triangle rounded to float32
    res = fp.grm(prefix)
    assert same(res["tri"], tri) and same(res["shared"], cnt) and len(res["ids"]) == N
    out = str(tmp_path / name)
    fp.write_grm(out, res["ids"], res["tri"], res["shared"])
    back = fp.read_grm(out)
    assert back["ids"] == res["ids"] and same(back["tri"], tri.astype(np.float32)) and same(back["shared"], cnt.astype(np.float32))
    assert os.path.getsize(out + ".grm.bin") == 4 * N * (N + 1) // 2 == os.path.getsize(out + ".grm.N.bin")
    print("%s grm() -> write_grm -> read_grm: %d float32 entries and %d ids read back equal" % (name, back["tri"].size, len(back["ids"])))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(fp):
    c = case(fp, "70x300")
    N, P = c["N"], c["P"]

    def refused(call, msg, code=-1):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == code
        print("refused: %s" % str(e.value)[:120])

    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        ref = ctx.grm_block(0, N, 0, N)
        calls = ((lambda: ctx.grm_block(0, N, 0, N), "fpca_grm_block"), (lambda: ctx.grm_tri(), "fpca_grm_tri"),
                 (lambda: ctx.grm_pairs(0.025), "fpca_grm_pairs"), (lambda: ctx.grm_cutoff(0.025), "fpca_grm_cutoff"),
                 (lambda: ctx.bench_grm(1), "fpca_bench_grm"))
        refused(lambda: ctx.grm_block(0, N + 1, 0, N), "are not a non-empty rectangle")
        refused(lambda: ctx.grm_block(0, N, N, 1), "are not a non-empty rectangle")
        refused(lambda: ctx.grm_block(3, 0, 0, N), "are not a non-empty rectangle")
        refused(lambda: ctx.grm_pairs(float("nan")), "fpca_grm_pairs: the threshold is NaN")
        refused(lambda: ctx.grm_cutoff(float("nan")), "fpca_grm_cutoff: the threshold is NaN")
        for bad in (3, -1):
            refused(lambda: ctx.grm_block(0, N, 0, N, divisor=bad), "fpca_grm_block: divisor %d is none of" % bad)
            refused(lambda: ctx.grm_tri(divisor=bad), "fpca_grm_tri: divisor %d is none of" % bad)
            refused(lambda: ctx.grm_pairs(0.025, divisor=bad), "fpca_grm_pairs: divisor %d is none of" % bad)
            refused(lambda: ctx.grm_cutoff(0.025, divisor=bad), "fpca_grm_cutoff: divisor %d is none of" % bad)
        with pytest.raises(ValueError, match="divisor must be one of"):
            ctx.grm_tri(divisor="n1")
        L = fp.lib()
        assert L.fpca_grm_block(ctx.h, 0, N, 0, N, 0, None, None) == -1 and L.fpca_grm_tri(ctx.h, 0, None, None) == -1
        assert L.fpca_grm_cutoff(ctx.h, 0.025, 0, None, None) == -1 and L.fpca_grm_pairs(ctx.h, None, 0.1, 0, 5, None, None, None, None, None) == -1
        with pytest.raises(ValueError):
            ctx.grm_cutoff(0.025, keep=np.ones(N + 1, dtype=bool))
        mask = np.arange(N) % 3 != 0
        ctx.set_sample_mask(mask)
        for call, fn in calls:
            refused(call, fn + ": a sample mask is set")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        for call, fn in calls:
            refused(call, fn + ": this context is one shard of several")
        ctx.set_rank(1, 0)
        assert same(ctx.grm_block(0, N, 0, N), ref)  # the context is intact
        # a preloaded mean / sd is the caller's standardisation: it is what the matrix is made of
        ms = c["ms"].copy()
        ms[20] = (1.0, 0.5)
        ctx.set_meansd(ms)
        r2 = reference(c["codes"], ms, longdouble=True)
        ok, worst = within(ctx.grm_block(0, N, 0, N), *g_reference(r2, "shared"))
        print("after set_meansd with one row changed: largest error / bound %.3f" % worst)
        assert ok
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.grm_block(0, 50, 0, 50), "fpca_grm_block: this context holds a dense matrix")
        refused(lambda: dense.grm_tri(), "fpca_grm_tri: this context holds a dense matrix")
        refused(lambda: dense.grm_pairs(0.1), "fpca_grm_pairs: this context holds a dense matrix")
        refused(lambda: dense.grm_cutoff(0.1), "fpca_grm_cutoff: this context holds a dense matrix")
    # a block over 1 GiB, met through a wide context of few SNPs
    big_n = 2 ** 14 + 1
    with fp.Context.from_packed(np.full(((big_n + 3) // 4) * 2, 0xFF, dtype=np.uint8), big_n, 2) as wide:
        buf = np.zeros(1)
        assert fp.lib().fpca_grm_block(wide.h, 0, big_n, 0, big_n, 0, buf.ctypes.data, None) == -1
        msg = fp.lib().fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "16385 x 16385 doubles is over the limit of 1073741824 bytes" in msg


# ---- 6. every exit gives the scratch back ------------------------------------------------------------------------------
def test_scratch_is_freed_on_every_exit(fp):
    """The pattern of tests/test_gpu_scratch.py on the test build: the n-th acquisition of a call is made to fail (FPCA_ENOMEM before the
    runtime is asked for anything) for every n until the call succeeds; after each failure the counts of live device allocations and
    events are what they were, the message names the entry point, and the result after the failures is the result before them."""
    import ctypes as C

    c = case(fp, "257x2100")
    N, P = c["N"], c["P"]
    keep = np.random.default_rng(5).random(N) < 0.7
    with fp.test_hooks() as L:
        def live():
            out = (C.c_uint64 * 3)()
            assert L.fpca_debug_scratch_live(out) == 0
            return tuple(int(v) for v in out)

        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            ctx.stats()

            def bench():
                ms, flops = ctx.bench_grm(2)
                return np.all(ms > 0), flops

            for entry, call in (("fpca_grm_block", lambda: ctx.grm_block(3, 130, 60, 190, counts=True)),
                                ("fpca_grm_tri", lambda: ctx.grm_tri(counts=True)),
                                ("fpca_grm_pairs", lambda: ctx.grm_pairs(0.025, keep=keep)),
                                ("fpca_grm_cutoff", lambda: (ctx.grm_cutoff(0.025, keep=keep),)),
                                ("fpca_bench_grm", bench)):
                L.fpca_debug_scratch_fail_at(0)
                base = live()
                ref = call()
                assert live() == base, "%s leaks on the success path" % entry
                first_ok, out = None, None
                for n in range(1, 40):
                    assert L.fpca_debug_scratch_fail_at(n) == 0
                    try:
                        out = call()
                    except fp.FpcaError as e:
                        assert e.code == ENOMEM and entry in str(e), (entry, n, str(e))
                        assert live() == base, "%s leaks when acquisition %d fails" % (entry, n)
                        continue
                    finally:
                        L.fpca_debug_scratch_fail_at(0)
                    first_ok = n
                    break
                print("%s: %d acquisitions, all given back on every injected failure" % (entry, (first_ok or 0) - 1))
                assert first_ok is not None and first_ok >= 5 and live() == base
                assert all(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) for a, b in zip(out, ref)), entry
