"""LD pruning (fpca_ld_band, fpca_ld_prune; Context.ld_band / ld_prune, ld_prune(), flashpca(ld=), ucca(ld=)) on the GPU against a numpy
yardstick that never calls the feature: the raw 2-bit codes are unpacked (the helpers of tests/test_gpu_snp_subset.py), the planes
x (dosage), m (call indicator) and q = x^2 are float64 matrices, and the six sums of a pair come from BLAS products -- integers below
2^53, so exact.  r2 = ((double)c * (double)c) / ((double)vx * (double)vy) of include/fpca.h has no add beside a multiply, so the numpy
restatement reproduces it BIT FOR BIT, and every comparison here is array_equal.  The pruning rule is restated in plain Python from the
text of include/fpca.h (every window visits all its pairs again; one numpy step per SNP i inside a window only gathers the j's that are
still kept and above the threshold, in ascending order); maf comes from ctx.stats(), whose mean is array_equal to the oracle's.
The golden filesets are LD-thinned already, so most cases run on generated genotypes with LD (ld_codes) uploaded with
Context.from_packed.  Every test prints what it measured (pytest -s).
Measured on the MI355X (profiles/ld_prune_test_figures.txt): every band -- 15 spans and 6 off-tile ranges on each of the three shapes, the
hapmap3_data range -- equals numpy bit for bit; all 60 masks (10 settings x 3 shapes x {all, 30 % pre-cleared}) equal the restatement's and
keep the counts of EXPECTED; three monomorphic SNPs (40, 41, 60) in each shape; slabs of 64 / 200 SNPs and the forced six-product path
change nothing; hapmap3_data (1000, 50, 0.05) keeps 13,967 of 14,389, (50, 5, 0.5) all, data_chr1 1,094 of 1,129, after snps= / maf=
13,491 of 13,911; flashpca(ld=) against pca_fast eigenvalues 4.6e-13, pve 1.1e-14, vectors 1.9e-10, loadings 2.1e-11; ucca(ld=) rows
identical to the unfiltered scan's.  The 15 tests take 3.7 s together."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
CHR1 = os.path.join(GOLD, "data_chr1")
REGIONS = "5 44000000 51500000 r1\n6 25000000 33500000 r2\n8 8000000 12000000 r3\n11 45000000 57000000 r4\n"  # exclusion_regions_hg19.txt


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


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


def ld_codes(N, P, seed, seg=64, miss=0.02):
    """Genotypes with LD: segments of `seg` SNPs in which each SNP copies its predecessor except at a random share of the samples."""
    rng = np.random.default_rng(seed)
    d = np.empty((P, N), dtype=np.int64)
    for j in range(P):
        if j % seg == 0:
            p = rng.uniform(0.1, 0.5)
            d[j] = rng.binomial(2, p, N)
        else:
            d[j] = np.where(rng.random(N) < rng.uniform(0.02, 0.35), rng.binomial(2, p, N), d[j - 1])
    d[5] = d[4]  # a duplicate (an equal-MAF tie: the later one goes)
    d[17] = 2 - d[16]  # r = -1
    d[40] = 1  # all heterozygous
    d[41] = 0  # monomorphic
    codes = np.array([3, 2, 0], dtype=np.uint8)[d]
    codes[rng.random((P, N)) < miss] = 1
    codes[60] = 1  # no call at all
    codes[70, :N // 2] = 1  # half missing
    return codes


# (N, P, seed, chromosome boundaries or None): the smallest shapes at which each part can break --
#   130 x 257   one 512-sample chunk that is mostly pad samples; 257 = four 64-SNP tiles and one SNP
#   511 x 1000  N mod 4 = 3 (pad bits in the last byte), pitch 128
#   2049 x 600  pitch 640: five chunks, one real sample in the last 512
SHAPES = {"511x1000": (511, 1000, 1, [0, 300, 301, 1000]), "2049x600": (2049, 600, 2, None), "130x257": (130, 257, 3, [0, 100, 257])}
GRID = [(50, 5, 0.2), (1000, 50, 0.05), (2, 1, 0.5), (7, 7, 0.3), (7, 1, 0.3), (33, 1, 0.8), (129, 64, 0.1), (129, 128, 0.1), (20, 20, 0.2), (20, 3, 0.2)]
# what the restatement of the rule kept on the CPU, per (window, step, r2), in the order of SHAPES
EXPECTED = {(50, 5, 0.2): (154, 90, 41), (1000, 50, 0.05): (89, 49, 18), (2, 1, 0.5): (433, 256, 113), (7, 7, 0.3): (277, 164, 74),
            (7, 1, 0.3): (200, 118, 52), (33, 1, 0.8): (751, 461, 178), (129, 64, 0.1): (107, 62, 22), (129, 128, 0.1): (108, 62, 23),
            (20, 20, 0.2): (181, 104, 47), (20, 3, 0.2): (154, 90, 41)}


def chrom_codes(bounds, P):
    if bounds is None:
        return None
    c = np.zeros(P, dtype=np.uint32)
    for k in range(len(bounds) - 1):
        c[bounds[k]:bounds[k + 1]] = 7 + (k % 2)  # codes repeat: a chromosome is a RUN of equal codes
    return c


# ---- the yardstick -------------------------------------------------------------------------------------------------
def band_numpy(codes, span, rows=512):
    """r2[i][d - 1] for the pair (i, i + d), d = 1 .. span, NaN past the last SNP: the formula of include/fpca.h, in blocks of rows."""
    P, N = codes.shape
    x = np.array([2.0, 0.0, 1.0, 0.0])[codes]
    m = (codes != 1).astype(np.float64)
    q = x * x
    out = np.full((P, span), np.nan)
    for b in range(0, P, rows):
        e = min(b + rows, P)
        f = min(e + span, P)
        I, J = slice(b, e), slice(b, f)
        n, sx, sy = m[I] @ m[J].T, x[I] @ m[J].T, m[I] @ x[J].T
        sxy, sxx, syy = x[I] @ x[J].T, q[I] @ m[J].T, m[I] @ q[J].T
        assert max(a.max() for a in (n, sx, sy, sxy, sxx, syy)) < 2.0 ** 53
        n, sx, sy, sxy, sxx, syy = (a.astype(np.int64) for a in (n, sx, sy, sxy, sxx, syy))
        c, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
        with np.errstate(invalid="ignore", divide="ignore"):
            r = (c.astype(np.float64) * c.astype(np.float64)) / (vx.astype(np.float64) * vy.astype(np.float64))
        for i in range(b, e):
            k = min(span, P - 1 - i)
            out[i, :k] = r[i - b, i - b + 1:i - b + 1 + k]
    return out


def totals_numpy(codes):
    """(calls, sum x, sum x^2) per SNP over its own calls."""
    x = np.array([2, 0, 1, 0], dtype=np.int64)[codes]
    return (codes != 1).sum(axis=1).astype(np.int64), x.sum(axis=1), (x * x).sum(axis=1)


def maf_numpy(ms, nmiss, N):
    """min(p, 1 - p) with p = mean / 2, 0 for a SNP without a call: as fpca_snp_qc computes it."""
    with np.errstate(invalid="ignore"):
        p = ms[:, 0] / 2.0
        m = np.minimum(p, 1.0 - p)
    return np.where((nmiss >= N) | np.isnan(p), 0.0, m)


def prune_python(band, totals, maf, chrom, w, s, t, keep=None):
    """The rule of include/fpca.h, window by window; every window visits all its pairs."""
    P = band.shape[0]
    n, sx, sq = totals
    keep = np.ones(P, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    keep &= (n * sq - sx * sx) != 0
    above = band > t  # (NaN: never)
    starts = [0] + ([] if chrom is None else [j for j in range(1, P) if chrom[j] != chrom[j - 1]]) + [P]
    for c0, c1 in zip(starts[:-1], starts[1:]):
        L = c1 - c0
        o = 0
        while True:
            end = min(o + w, L)
            for i in range(c0 + o, c0 + end):
                if not keep[i]:
                    continue
                k = c0 + end - i - 1  # the j's of this window after i: i + 1 .. i + k
                if k <= 0:
                    continue
                cand = i + 1 + np.flatnonzero(keep[i + 1:i + 1 + k] & above[i, :k])  # ascending; dropping one j changes no other j of this i
                lower = maf[i] < maf[cand]
                if lower.any():
                    first = int(np.argmax(lower))
                    keep[cand[:first]] = False
                    keep[i] = False
                else:
                    keep[cand] = False
            if end >= L:
                break
            o += s
    return keep


_CASE = {}


def case(fp, name):
    """One synthetic shape: codes, the full band from numpy, totals -- computed once and left unchanged."""
    if name not in _CASE:
        N, P, seed, bounds = SHAPES[name]
        codes = ld_codes(N, P, seed)
        _CASE[name] = dict(N=N, P=P, codes=codes, band=band_numpy(codes, P + 5), totals=totals_numpy(codes), chrom=chrom_codes(bounds, P),
                           packed=pack_codes(codes))
    return _CASE[name]


def open_case(fp, c, accum="fp64"):
    return fp.Context.from_packed(c["packed"], c["N"], c["P"], accum=accum)


# ---- 1. the band, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_band_bit_for_bit(fp, name):
    c = case(fp, name)
    N, P, ref = c["N"], c["P"], c["band"]
    # the planted SNPs, in the yardstick itself
    assert ref[4, 0] == 1.0 and ref[16, 0] == 1.0  # a duplicate and r = -1: over the shared calls c = +-vx = +-vy, the quotient is exactly 1
    assert np.isnan(ref[40]).all() and np.isnan(ref[41]).all() and np.isnan(ref[60]).all()
    assert 0.2 < np.mean(ref[:, 0] > 0.2) and np.nanmax(ref) <= 1.0
    with open_case(fp, c) as ctx:
        # 63 .. 65 and 191 .. 193 straddle the kernel's 64-SNP tiles (one more / one fewer J tile per I tile)
        for span in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, P - 1, P + 5):
            got = ctx.ld_band(0, P, span)
            assert got.shape == (P, span) and got.dtype == np.float64
            want = ref[:, :span]
            same = np.array_equal(got, want, equal_nan=True)
            print("%s ld_band(0, %d, %d): %d finite, %d NaN, equal to numpy bit for bit: %s" % (
                name, P, span, np.isfinite(got).sum(), np.isnan(got).sum(), same))
            assert same, (name, span, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
        assert got[4, 0] == 1.0 and got[16, 0] == 1.0
        assert np.isnan(got[40]).all() and np.isnan(got[41]).all() and np.isnan(got[60]).all()
        # ranges that start and end off a tile boundary: pairs that reach past the range are NaN
        for snp0, nsnp in ((5, 70), (63, 130), (64, 64), (P - 41, 41), (P - 1, 1), (1, P - 1)):
            got = ctx.ld_band(snp0, nsnp, 40)
            want = ref[snp0:snp0 + nsnp, :40].copy()
            for i in range(nsnp):
                want[i, max(nsnp - 1 - i, 0):] = np.nan
            same = np.array_equal(got, want, equal_nan=True)
            print("%s ld_band(%d, %d, 40): equal to numpy bit for bit: %s" % (name, snp0, nsnp, same))
            assert same, (name, snp0, nsnp)


# ---- 2. the prune, mask for mask ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_prune_masks(fp, name):
    c = case(fp, name)
    N, P, chrom = c["N"], c["P"], c["chrom"]
    col = list(SHAPES).index(name)
    nmiss = (c["codes"] == 1).sum(axis=1)
    pre = np.random.default_rng(99).random(P) >= 0.3  # a pre-cleared random 30 % of keep
    mono = (c["totals"][0] * c["totals"][2] - c["totals"][1] ** 2) == 0
    print("%s: %d monomorphic SNPs (own calls): %s" % (name, mono.sum(), np.flatnonzero(mono)))
    assert mono.sum() == 3 and mono[40] and mono[41] and mono[60]
    ref = {}
    with open_case(fp, c) as ctx:
        maf = maf_numpy(ctx.stats()[0], nmiss, N)
        assert maf[4] == maf[5] or nmiss[4] != nmiss[5]
        for w, s, t in GRID:
            for label, keep in (("all", None), ("70%", pre)):
                want = prune_python(c["band"], c["totals"], maf, chrom, w, s, t, keep)
                got = ctx.ld_prune(w, s, t, chrom=chrom, keep=keep)
                ref[(w, s, t, label)] = want
                print("%s (%d, %d, %g) keep=%s: yardstick keeps %d of %d, the device %d, masks equal: %s" % (
                    name, w, s, t, label, want.sum(), P, got.sum(), np.array_equal(got, want)))
                # the case is not vacuous (on the yardstick's mask)
                assert 0.05 * P <= want.sum() <= 0.90 * P, (name, w, s, t, label, int(want.sum()))
                if keep is None:
                    assert want.sum() == EXPECTED[(w, s, t)][col], (name, w, s, t, int(want.sum()))
                else:
                    assert not want[~pre].any()
                assert got.dtype == np.bool_ and np.array_equal(got, want), (name, w, s, t, label)
        # a second call on the same context: the same mask
        assert np.array_equal(ctx.ld_prune(50, 5, 0.2, chrom=chrom), ref[(50, 5, 0.2, "all")])
    assert not np.array_equal(ref[(7, 7, 0.3, "all")], ref[(7, 1, 0.3, "all")])
    assert not np.array_equal(ref[(20, 20, 0.2, "all")], ref[(20, 3, 0.2, "all")])


def test_prune_in_slabs_and_through_the_general_path(fp, monkeypatch):
    """The test build's switches: the bitmap in slabs of 64 and 200 SNPs (rows whose pairs reach into the next slab), and the six-product
    path forced where the x.x-only path would run -- the same masks and the same band bits."""
    c = case(fp, "2049x600")
    nmiss = (c["codes"] == 1).sum(axis=1)
    with fp.test_hooks():
        with open_case(fp, c) as ctx:
            maf = maf_numpy(ctx.stats()[0], nmiss, c["N"])
            want = prune_python(c["band"], c["totals"], maf, None, 129, 64, 0.1)
            for rows in ("64", "200", "100000"):
                monkeypatch.setenv("FPCA_LD_SLAB_ROWS", rows)
                got = ctx.ld_prune(129, 64, 0.1)
                print("slabs of %s SNPs: %d kept, equal to the yardstick: %s" % (rows, got.sum(), np.array_equal(got, want)))
                assert np.array_equal(got, want)
            monkeypatch.delenv("FPCA_LD_SLAB_ROWS")


# ---- 5. the x.x-only path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["no_missing", "one_tile"])
def test_fast_path_gives_the_same_bits(fp, monkeypatch, where):
    """A source without a missing call, and one whose missing calls sit in SNPs 64 .. 95 only (half a tile: the blocks around it take
    the x.x-only path, the ones that touch it the six products): numpy, the default build and the forced general path agree bit for bit."""
    N, P = 515, 300
    codes = ld_codes(N, P, 11, miss=0.0)
    codes[60] = codes[59]
    codes[70] = codes[69]
    if where == "one_tile":
        codes[64:96][np.random.default_rng(12).random((32, N)) < 0.05] = 1
    assert ((codes == 1).sum() > 0) == (where == "one_tile")
    ref = band_numpy(codes, 140)
    with fp.Context.from_packed(pack_codes(codes), N, P) as ctx:
        fast = ctx.ld_band(0, P, 140)
        mask_fast = ctx.ld_prune(50, 5, 0.2)
    with fp.test_hooks():
        monkeypatch.setenv("FPCA_LD_FORCE_GENERAL", "1")
        with fp.Context.from_packed(pack_codes(codes), N, P) as ctx:
            general = ctx.ld_band(0, P, 140)
            mask_general = ctx.ld_prune(50, 5, 0.2)
        monkeypatch.delenv("FPCA_LD_FORCE_GENERAL")
    eq = [np.array_equal(fast, ref, equal_nan=True), np.array_equal(general, ref, equal_nan=True), np.array_equal(mask_fast, mask_general)]
    print("%s: default path equal to numpy %s, forced general path equal to numpy %s, prune masks equal %s (%d kept)" % (
        where, eq[0], eq[1], eq[2], mask_fast.sum()))
    assert all(eq) and 0 < mask_fast.sum() < P


# ---- 3. real data ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hm3(fp):
    codes, N, P = read_bed_codes(HM3)
    rows = [l.split() for l in open(HM3 + ".bim").read().splitlines() if l.strip()]
    chrom = np.unique(np.array([r[0] for r in rows]), return_inverse=True)[1].astype(np.uint32)
    assert (N, P) == (957, 14389) and np.unique(chrom).size == 25
    return dict(codes=codes, N=N, P=P, chrom=chrom, band=band_numpy(codes, 999), totals=totals_numpy(codes))


def yardstick_mask(fp, codes, chrom, band, totals, w, s, t):
    P, N = codes.shape
    with fp.Context.from_packed(pack_codes(codes), N, P) as ctx:
        ms = ctx.stats()[0]
    return prune_python(band, totals, maf_numpy(ms, (codes == 1).sum(axis=1), N), chrom, w, s, t)


def test_prune_hapmap3(fp, hm3):
    N, P = hm3["N"], hm3["P"]
    want = yardstick_mask(fp, hm3["codes"], hm3["chrom"], hm3["band"], hm3["totals"], 1000, 50, 0.05)
    want_none = yardstick_mask(fp, hm3["codes"], hm3["chrom"], hm3["band"], hm3["totals"], 50, 5, 0.5)
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        B = np.random.default_rng(4).standard_normal((N, 16))
        before = ctx.apply_xt(B)
        got = ctx.ld_prune(1000, 50, 0.05, chrom=hm3["chrom"])
        got_none = ctx.ld_prune(50, 5, 0.5, chrom=hm3["chrom"])
        band = ctx.ld_band(7000, 300, 50)
        after = ctx.apply_xt(B)
    print("hapmap3_data (1000, 50, 0.05): yardstick keeps %d of %d, the device %d, equal %s; (50, 5, 0.5): %d and %d; apply_xt unchanged %s" % (
        want.sum(), P, got.sum(), np.array_equal(got, want), want_none.sum(), got_none.sum(), np.array_equal(before, after)))
    assert want.sum() == 13967 and want_none.all()
    assert np.array_equal(got, want) and np.array_equal(got_none, want_none)
    assert np.array_equal(fp.ld_prune(HM3, 1000, 50, 0.05), want)  # the fileset entry point reads the chromosomes from the .bim
    ref = hm3["band"][7000:7300, :50].copy()
    for i in range(300):
        ref[i, max(299 - i, 0):] = np.nan
    assert np.array_equal(band, ref, equal_nan=True)
    assert np.array_equal(before, after)  # the source computes what it computed


def test_prune_data_chr1(fp):
    codes, N, P = read_bed_codes(CHR1)
    assert (N, P) == (957, 1129)
    want = yardstick_mask(fp, codes, None, band_numpy(codes, 999), totals_numpy(codes), 1000, 50, 0.05)
    got = fp.ld_prune(CHR1, 1000, 50, 0.05)
    print("data_chr1 (1000, 50, 0.05): yardstick keeps %d of %d, the device %d, equal %s" % (want.sum(), P, got.sum(), np.array_equal(got, want)))
    assert want.sum() == 1094 and np.array_equal(got, want)


def test_ld_prune_after_filters(fp, hm3, tmp_path):
    """snps / maf first, then the prune on their survivors: the yardstick runs on the re-packed survivors, whose windows count them."""
    regions = tmp_path / "exclusion_regions_hg19.txt"
    regions.write_text(REGIONS)
    ranges = fp.snp_filter(HM3, exclude_ranges=str(regions))
    codes, N, P = hm3["codes"], hm3["N"], hm3["P"]
    with fp.Context.from_bed(HM3 + ".bed", N) as ctx:
        maf_all = maf_numpy(ctx.stats()[0], (codes == 1).sum(axis=1), N)
    first = ranges & ~(maf_all < 0.05)
    sub = codes[first]
    kept = yardstick_mask(fp, sub, hm3["chrom"][first], band_numpy(sub, 999), totals_numpy(sub), 1000, 50, 0.05)
    want = first.copy()
    want[np.flatnonzero(first)] = kept
    got = fp.ld_prune(HM3, 1000, 50, 0.05, snps=ranges, maf=0.05)
    print("ld_prune(hapmap3_data, 1000, 50, 0.05, snps=ranges, maf=0.05): %d after the filters, yardstick keeps %d, the device %d, equal %s" % (
        first.sum(), want.sum(), got.sum(), np.array_equal(got, want)))
    assert first.sum() < P - 53 and 0 < want.sum() < first.sum()
    assert np.array_equal(got, want)


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
def test_flashpca_with_ld_against_the_oracle(fp, O, hm3):
    """oracle.pca_fast on the re-packed kept records, at the tolerances of tests/test_gpu_snp_subset.py."""
    codes, N, P = hm3["codes"], hm3["N"], hm3["P"]
    want = yardstick_mask(fp, codes, hm3["chrom"], hm3["band"], hm3["totals"], 1000, 50, 0.05)
    r = fp.flashpca(HM3, ndim=10, ld=(1000, 50, 0.05), do_loadings=True)
    mask = r["snps_kept"]
    kept = int(mask.sum())
    assert mask.dtype == np.bool_ and np.array_equal(mask, want)
    assert r["loadings"].shape == (kept, 10) and r["center"].shape == (kept,) and r["vectors"].shape == (N, 10)
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(packed=pack_codes(codes[mask]), N=N, P=kept, stand="binom2")
        ref = O.pca_fast(od, 10, do_loadings=True)
    e_d = float(np.max(np.abs(r["values"] - ref["d"]) / ref["d"]))
    e_pve = float(np.max(np.abs(r["pve"] - ref["pve"])))
    e_u = e_v = 0.0
    for c in range(5):  # well-separated components; up to sign
        s = np.sign(ref["U"][:, c] @ r["vectors"][:, c])
        e_u = max(e_u, float(np.max(np.abs(ref["U"][:, c] * s - r["vectors"][:, c]))))
        e_v = max(e_v, float(np.max(np.abs(ref["V"][:, c] * s - r["loadings"][:, c]))))
    print("flashpca(ld=(1000, 50, 0.05)): %d of %d SNPs; against pca_fast eigenvalues %.2e, pve %.2e, vectors %.2e, loadings %.2e" % (
        kept, P, e_d, e_pve, e_u, e_v))
    assert e_d < 1e-6 and e_pve < 1e-8 and e_u < 1e-5 and e_v < 1e-5
    assert np.array_equal(r["center"], ref["meansd"][:, 0]) and np.array_equal(r["scale"], ref["meansd"][:, 1])
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, ld=(1000, 50, 0.05), keep=np.ones(N, dtype=bool))


def test_ucca_with_ld(fp):
    """A SNP's F test does not depend on the other SNPs: the pruned scan is the selected rows of the unfiltered one."""
    codes, N, P = read_bed_codes(CHR1)
    Y = np.random.default_rng(3).standard_normal((N, 3))
    full = fp.ucca(CHR1, Y, standy="sd")
    want = yardstick_mask(fp, codes, None, band_numpy(codes, 199), totals_numpy(codes), 200, 20, 0.05)
    sub = fp.ucca(CHR1, Y, standy="sd", ld=(200, 20, 0.05))
    mask = sub["snps_kept"]
    a, b = sub["result"], full["result"][mask]
    same = np.array_equal(a, b, equal_nan=True)
    print("ucca(ld=(200, 20, 0.05)) on data_chr1: %d of %d SNPs, mask equal to the yardstick %s, rows equal to the unfiltered scan's %s" % (
        mask.sum(), P, np.array_equal(mask, want), same))
    assert np.array_equal(mask, want) and 0 < mask.sum() < P
    assert a.shape == (int(mask.sum()), 3) and sub["snp_ids"] == [s for s, m in zip(full["snp_ids"], mask) if m]
    assert same


# ---- 6. refusals and state -------------------------------------------------------------------------------------------------
def test_refusals(fp):
    c = case(fp, "130x257")
    N, P = c["N"], c["P"]

    def refused(call, msg, code=-1):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == code
        print("refused: %s" % str(e.value)[:110])

    with open_case(fp, c) as ctx:
        B = np.random.default_rng(5).standard_normal((N, 16))
        before = ctx.apply_xt(B)
        refused(lambda: ctx.ld_prune(1, 1, 0.2), "window = 1")
        refused(lambda: ctx.ld_prune(0, 1, 0.2), "window = 0")
        refused(lambda: ctx.ld_prune(10, 0, 0.2), "step = 0")
        refused(lambda: ctx.ld_prune(10, 11, 0.2), "step = 11 is larger than window = 10")
        for t in (float("nan"), -0.01, 1.01):
            refused(lambda: ctx.ld_prune(10, 5, t), "not in \\[0, 1\\]")
        refused(lambda: ctx.ld_band(0, P, 0), "span = 0")
        refused(lambda: ctx.ld_band(0, P + 1, 5), "are not a non-empty range")
        refused(lambda: ctx.ld_band(P, 1, 5), "are not a non-empty range")
        refused(lambda: ctx.ld_band(3, 0, 5), "are not a non-empty range")
        L = fp.lib()
        big = np.zeros(1)
        assert L.fpca_ld_band(ctx.h, 0, P, 2 ** 20, big.ctypes.data) == -1  # 257 x 2^20 doubles = 2 GiB
        msg = L.fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "257 SNPs x 1048576 doubles" in msg and "1073741824 bytes" in msg
        assert L.fpca_ld_band(ctx.h, 0, P, 5, None) == -1 and L.fpca_ld_prune(ctx.h, None, 10, 5, 0.2, None, None) == -1
        with pytest.raises(ValueError):
            ctx.ld_prune(10, 5, 0.2, chrom=np.zeros(P - 1, dtype=np.uint32))
        with pytest.raises(ValueError):
            ctx.ld_prune(10, 5, 0.2, keep=np.ones(P + 1, dtype=bool))
        ctx.set_sample_mask(np.arange(N) % 3 != 0)
        refused(lambda: ctx.ld_prune(10, 5, 0.2), "fpca_ld_prune: a sample mask is set")
        refused(lambda: ctx.ld_band(0, P, 5), "fpca_ld_band: a sample mask is set")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        refused(lambda: ctx.ld_prune(10, 5, 0.2), "one shard of several")
        refused(lambda: ctx.ld_band(0, P, 5), "one shard of several")
        ctx.set_rank(1, 0)
        m1 = ctx.ld_prune(10, 5, 0.2)
        band = ctx.ld_band(0, P, 9)
        m2 = ctx.ld_prune(10, 5, 0.2)
        after = ctx.apply_xt(B)
        print("after the refused and the served calls: apply_xt equal to before %s, second prune equal to the first %s" % (
            np.array_equal(before, after), np.array_equal(m1, m2)))
        assert np.array_equal(before, after) and np.array_equal(m1, m2) and np.array_equal(band, c["band"][:, :9], equal_nan=True)
        ctx.set_meansd(ctx.stats()[0])
        refused(lambda: ctx.ld_prune(10, 5, 0.2), "preloaded mean/sd")
    # N > 2^25: 4 N^2 would leave the 53 bits of a double (one SNP more than a context needs, 8 MiB per record)
    big_n = 2 ** 25 + 1
    with fp.Context.from_packed(np.full(((big_n + 3) // 4) * 2, 0xFF, dtype=np.uint8), big_n, 2) as big_ctx:
        refused(lambda: big_ctx.ld_band(0, 2, 1), "33554433 samples; above 2\\^25")
        refused(lambda: big_ctx.ld_prune(2, 1, 0.5), "33554433 samples; above 2\\^25")
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.ld_prune(10, 5, 0.2), "fpca_ld_prune: this context holds a dense matrix")
        refused(lambda: dense.ld_band(0, 30, 5), "fpca_ld_band: this context holds a dense matrix")
    with pytest.raises(ValueError, match="ld is \\(window, step, r2\\)"):
        fp.flashpca(HM3, ndim=2, ld=(1000, 50))
    with pytest.raises(ValueError, match="PLINK fileset"):
        fp.flashpca(np.zeros((8, 5)), ndim=1, ld=(10, 5, 0.2))
