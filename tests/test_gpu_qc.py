"""The genotype census, the HWE exact test and the two QC rules on the GPU (fpca_snp_counts / fpca_sample_counts / fpca_hwe_exact /
fpca_sample_qc / fpca_snp_qc_samples; Context.snp_counts / sample_counts / hwe_exact / sample_qc / snp_qc_samples, qc_filter(),
flashpca(mind=, hwe=)) against tests/qc_yardstick.py, which unpacks the raw 2-bit codes in numpy and never calls the feature.
  census     array_equal.  Shapes N x P: 70 x {1, 2, 3, 4, 14, 15, 16, 254, 255, 256, 257, 1,100} -- the per-sample pass widens its
             vertical counters after 3, 15 and 255 records, each period and its neighbours is a shape --, 513 x 1,100 (the second 128-byte
             pitch step), 4,100 x 600 (two strips of 256 words), 16,450 x 300 (five strips), 70 x 70,000 (counts past any 16-bit field);
             slabs of 1, 14, 15, 16, 254, 255, 256, 1,099, 1,100 and 1,101 SNPs through FPCA_QC_SLAB_SNPS.  Samples 0, 15, 16 and N - 1 are
             constant at codes 0, 1, 2 and 3.  SNP masks: all, alternating, first only, last only, 30 % random; sample masks of the per-SNP
             pass: all, 70 % random, one sample, the last sample only.
  HWE        every triple with a + b + c <= 12 against rational arithmetic; 1,000 random triples at n = 2,000 and all SNPs of the four
             golden filesets against the recurrence in longdouble.  Bound, from two roundings per step plus the sums:
             |p - p_ref| <= 8 n 2^-53 p_ref where p_ref >= 1e-280, 0 <= p <= 1e-279 below; never NaN, never above 1.  The yardstick itself
             asserts that no term of any SNP lies within 2^-30 (relative) of the tie boundary w(a) (1 + 2^-20).
  decisions  on the golden filesets the rules equal the restated masks, no SNP left out; the restated p-values keep 1.5e-3 relative
             distance from the thresholds; the drop counts are those of GOLDEN.
  end to end flashpca(mind=, geno=, hwe=, maf=) against qc_filter(), the yardstick and flashpca(snps=, keep=).
Every test prints what it measured (pytest -s)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qc_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
HM3 = os.path.join(Y.GOLD, "hapmap3_data")
MIND = (0.05, 0.01, 0.005)
HWE = (1e-2, 1e-3, 1e-4, 1e-6, 1e-10)
GOLDEN = {  # drops: samples at the three mind thresholds, SNPs (all samples) at the five hwe thresholds
    "hapmap3_data": ((0, 1, 47), (1729, 798, 347, 83, 80)),
    "data_chr1": ((1, 4, 63), (122, 50, 18, 0, 0)),
    "hm3_thinned": ((0, 1, 46), (1619, 702, 256, 0, 0)),
    "kg_thinned": ((0, 0, 0), (2267, 1120, 602, 204, 21)),
}


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


# ---- data ------------------------------------------------------------------------------------------------------------
_made = {}


def random_codes(N, P):
    """(P, N) raw codes: 3 % missing overall, a tenth of the SNPs with 30 %; samples 0, 15, 16, N - 1 constant at codes 0, 1, 2, 3."""
    if (N, P) not in _made:
        rng = np.random.default_rng(1000 * N + P)
        f = rng.uniform(0.02, 0.5, P)
        d = rng.binomial(2, f[:, None], (P, N))
        codes = np.array([3, 2, 0], dtype=np.uint8)[d]
        rate = np.where(rng.random(P) < 0.1, 0.3, 0.03)
        codes[rng.random((P, N)) < rate[:, None]] = 1
        for code, s in enumerate((0, 15, 16, N - 1)):
            codes[:, s] = code
        codes.setflags(write=False)
        _made[(N, P)] = codes
    return _made[(N, P)]


def snp_masks(P, rng):
    first, last = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    first[0] = last[-1] = True
    return {"all": None, "alternating": np.arange(P) % 2 == 0, "first": first, "last": last, "30%": rng.random(P) < 0.3}


def sample_masks(N, rng):
    one, last = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    one[N // 3] = last[-1] = True
    return {"all": None, "70%": rng.random(N) < 0.7, "one": one, "last": last}


def check_census(fp, ctx, codes, tag):
    P, N = codes.shape
    rng = np.random.default_rng(P + N)
    for name, m in snp_masks(P, rng).items():
        if m is not None and not m.any():
            continue
        got = ctx.sample_counts(m)
        assert got.dtype == np.uint32 and got.shape == (N, 4)
        assert np.array_equal(got, Y.sample_counts(codes, m)), (tag, "sample_counts", name)
        assert (got.sum(axis=1) == (P if m is None else int(m.sum()))).all()
    for name, m in sample_masks(N, rng).items():
        if m is not None and not m.any():
            continue
        got = ctx.snp_counts(m)
        assert got.dtype == np.uint32 and got.shape == (P, 4)
        assert np.array_equal(got, Y.snp_counts(codes, m)), (tag, "snp_counts", name)


SHAPES = [(70, P) for P in (1, 2, 3, 4, 14, 15, 16, 254, 255, 256, 257, 1100)] + [(513, 1100), (4100, 600), (16450, 300), (70, 70000)]


@pytest.mark.parametrize("N,P", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_census_equals_numpy(fp, N, P):
    codes = random_codes(N, P)
    with fp.Context.from_packed(Y.pack_codes(codes), N, P) as ctx:
        check_census(fp, ctx, codes, "%dx%d" % (N, P))
        # all samples: the missing column is K1's count, and (2 c0 + c2) / ngood is K1's mean bit for bit
        cnt = ctx.snp_counts()
        assert np.array_equal(cnt[:, 1], ctx.snp_missing())
        c = cnt.astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (2 * c[:, 0] + c[:, 2]).astype(np.float64) / (c[:, 0] + c[:, 2] + c[:, 3]).astype(np.float64)
        assert np.array_equal(mean, ctx.stats()[0][:, 0], equal_nan=True)
        # a repeat call is bit-identical
        m = np.arange(P) % 3 != 1
        assert np.array_equal(ctx.sample_counts(), ctx.sample_counts()) and np.array_equal(ctx.snp_counts(), cnt)
        if m.any():
            assert np.array_equal(ctx.sample_counts(m), ctx.sample_counts(m))
    smp = Y.sample_counts(codes)
    print("%d x %d: largest per-sample count %d, largest per-SNP count %d" % (N, P, smp.max(), cnt.max()))
    if P == 70000:
        assert smp.max() > 65535


@pytest.mark.parametrize("slab", (1, 14, 15, 16, 254, 255, 256, 1099, 1100, 1101))
def test_slab_edges_change_nothing(fp, monkeypatch, slab):
    from flashpca_amd import _lib

    N, P = 513, 1100
    codes = random_codes(N, P)
    rng = np.random.default_rng(slab)
    monkeypatch.setenv("FPCA_QC_SLAB_SNPS", str(slab))
    with _lib.test_hooks():
        with fp.Context.from_packed(Y.pack_codes(codes), N, P) as ctx:
            for name, m in snp_masks(P, rng).items():
                assert np.array_equal(ctx.sample_counts(m), Y.sample_counts(codes, m)), (slab, name)


def test_census_refusals(fp):
    N, P = 70, 16
    codes = random_codes(N, P)
    with fp.Context.from_packed(Y.pack_codes(codes), N, P) as ctx:
        with pytest.raises(ValueError):
            ctx.snp_counts(np.ones(N + 1, dtype=bool))
        with pytest.raises(ValueError):
            ctx.sample_counts(np.ones(P + 1, dtype=bool))
        with pytest.raises(ValueError):
            ctx.hwe_exact(np.zeros((3, 3), dtype=np.int64))
        with pytest.raises(fp.FpcaError, match="no SNP is counted"):
            ctx.sample_qc(0.05, snps=np.zeros(P, dtype=bool))
        with pytest.raises(fp.FpcaError, match="keeps 0 of"):
            ctx.snp_qc_samples(np.zeros(N, dtype=bool), maf=0.05)
        for kw in (dict(maf=float("nan")), dict(hwe=float("nan")), dict(hwe=1.5), dict(geno=-0.5), dict(maf=0.6)):
            with pytest.raises(fp.FpcaError):
                ctx.snp_qc_samples(None, **kw)
        for mind in (float("nan"), -0.5):
            with pytest.raises(fp.FpcaError):
                ctx.sample_qc(mind)
        before = ctx.stats()[0].copy()
        keep = np.arange(N) % 2 == 0
        ctx.set_sample_mask(keep)
        for call in (ctx.snp_counts, ctx.sample_counts, lambda: ctx.sample_qc(0.05), lambda: ctx.snp_qc_samples(None, maf=0.05),
                     lambda: ctx.hwe_exact(np.zeros((1, 4), dtype=np.uint32))):
            with pytest.raises(fp.FpcaError, match="pass the mask as"):
                call()
        ctx.set_sample_mask(None)
        assert np.array_equal(ctx.stats()[0], before, equal_nan=True)  # the context is as it was
        assert ctx.hwe_exact(np.zeros((0, 4), dtype=np.uint32)).shape == (0,)
    with fp.Context.from_dense(np.zeros((8, 5))) as dense:
        with pytest.raises(fp.FpcaError, match="dense matrix"):
            dense.snp_counts()
        with pytest.raises(fp.FpcaError, match="dense matrix"):
            dense.sample_counts()


# ---- HWE -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx(fp):
    codes = random_codes(70, 16)
    with fp.Context.from_packed(Y.pack_codes(codes), 70, 16) as ctx:
        yield ctx


def rows_from_triples(t):
    """(c0, c2, c3) triples -> counts rows; the missing column holds something that must not matter."""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    return np.stack([t[:, 0], np.full(len(t), 7), t[:, 1], t[:, 2]], axis=1).astype(np.uint32)


def check_against_longdouble(p, rows, tag):
    p_ref, margin = Y.hwe_longdouble(rows)
    assert float(margin.min()) >= 2.0 ** -30, (tag, float(margin.min()))  # the condition on the fixtures
    ok, units = Y.hwe_bound_ok(p, p_ref, rows)
    print("%s: %d rows, largest error %.3f x n 2^-53 p_ref (bound 8), %d rows below 1e-280, closest term to the tie boundary %.2e" % (
        tag, len(rows), units, int((p_ref < LD("1e-280")).sum()), float(margin.min())))
    assert ok.all(), (tag, rows[~ok][:5], p[~ok][:5], p_ref[~ok][:5])
    return p_ref


def test_hwe_every_small_triple_against_fractions(small_ctx):
    triples = [(c0, c2, c3) for c0 in range(13) for c2 in range(13) for c3 in range(13) if c0 + c2 + c3 <= 12]
    assert len(triples) == 455
    rows = rows_from_triples(triples)
    p = small_ctx.hwe_exact(rows)
    assert p.dtype == np.float64 and not np.isnan(p).any() and (p <= 1).all() and (p > 0).all()
    worst = Fraction(0)
    for (c0, c2, c3), v in zip(triples, p):
        ex, n = Y.hwe_fractions(c0, c2, c3), c0 + c2 + c3
        err = abs(Fraction(float(v)) - ex)
        assert err <= 8 * n * Fraction(1, 2 ** 53) * ex, ((c0, c2, c3), float(v), float(ex))
        if n:
            worst = max(worst, err / (n * Fraction(1, 2 ** 53) * ex))
    print("455 triples: largest error %.3f x n 2^-53 p (bound 8)" % float(worst))
    assert p[0] == 1.0  # n = 0
    check_against_longdouble(p, rows, "small triples against longdouble")


def test_hwe_random_triples_and_edges(small_ctx):
    rng = np.random.default_rng(2005)
    n = 2000
    f = rng.uniform(0.01, 0.5, 1000)
    F = rng.choice([0.0, 0.0, 0.05, 0.2, -0.05], 1000)  # equilibrium, inbreeding, excess heterozygotes
    het = np.clip(2 * f * (1 - f) * (1 - F), 0, 1)
    hom = np.clip(f * f + f * (1 - f) * F, 0, 1 - het)
    t = np.array([rng.multinomial(n, [hom[i], het[i], 1 - hom[i] - het[i]]) for i in range(1000)])
    assert (t.sum(axis=1) == n).all()
    rows = rows_from_triples(t)
    p = small_ctx.hwe_exact(rows)
    p_ref = check_against_longdouble(p, rows, "1,000 random triples at n = 2,000")
    assert (p_ref < 1e-6).sum() > 50 and (p_ref > 0.1).sum() > 50  # both ends of the range are in
    # edges: n = 0; monomorphic; all heterozygous; (a, b, c) = (0, 500, 500) and (0, 2000, 2000), which underflows to exactly 0
    edges = rows_from_triples([(0, 0, 0), (700, 0, 0), (0, 0, 700), (1, 0, 0), (0, 1, 0), (0, 700, 0), (500, 0, 500), (2000, 0, 2000), (1999, 2, 1999)])
    pe = small_ctx.hwe_exact(edges)
    print("edges:", list(pe))
    assert list(pe[:5]) == [1.0, 1.0, 1.0, 1.0, 1.0] and pe[7] == 0.0 and 0 < pe[6] < 1e-279
    check_against_longdouble(pe, edges, "edges")
    assert np.array_equal(small_ctx.hwe_exact(rows), p)  # a repeat call is bit-identical


_golden = {}


def golden(name):
    if name not in _golden:
        codes, N, P = Y.golden_codes(name)
        cnt = Y.snp_counts(codes)
        p_ref, margin = Y.hwe_longdouble(cnt)
        _golden[name] = dict(codes=codes, N=N, P=P, cnt=cnt, smp=Y.sample_counts(codes), p_ref=p_ref, margin=margin)
    return _golden[name]


@pytest.mark.parametrize("name", Y.FILESETS)
def test_golden_filesets_counts_pvalues_and_decisions(fp, name):
    g = golden(name)
    codes, N, P = g["codes"], g["N"], g["P"]
    with fp.Context.from_bed(os.path.join(Y.GOLD, name + ".bed"), N) as ctx:
        assert ctx.P == P
        cnt, smp = ctx.snp_counts(), ctx.sample_counts()
        assert np.array_equal(cnt, g["cnt"]) and np.array_equal(smp, g["smp"])
        p = ctx.hwe_exact(cnt)
        check_against_longdouble(p, cnt, name)
        # --mind
        drops = []
        for mind in MIND:
            want = Y.sample_rule(g["smp"], P, mind, np.ones(N, dtype=bool))
            got = ctx.sample_qc(mind)
            assert got.dtype == np.bool_ and np.array_equal(got, want), mind
            drops.append(N - int(got.sum()))
        # --hwe over all samples: the restated p-values keep their distance from the thresholds, so the decision is the yardstick's
        hdrops = []
        for thr in HWE:
            assert float(np.abs(g["p_ref"] / LD(thr) - 1).min()) >= 1.5e-3, thr
            want = ~(g["p_ref"] < thr)
            got = ctx.snp_qc_samples(None, hwe=thr)
            assert np.array_equal(got, want), thr
            assert np.array_equal(got, Y.snp_rule(cnt, N, 0.0, 1.0, thr, p, np.ones(P, dtype=bool)))
            hdrops.append(P - int(got.sum()))
        # the three SNP filters together over a subset of the samples, among a subset of the SNPs
        rng = np.random.default_rng(P)
        samples, keep = rng.random(N) < 0.6, rng.random(P) < 0.8
        sub = Y.snp_counts(codes, samples)
        p_sub, _ = Y.hwe_longdouble(sub)
        assert float(np.abs(p_sub / LD(1e-3) - 1).min()) >= 1e-6
        want = Y.snp_rule(sub, int(samples.sum()), 0.05, 0.01, 1e-3, p_sub, keep)
        got = ctx.snp_qc_samples(samples, maf=0.05, geno=0.01, hwe=1e-3, keep=keep)
        assert np.array_equal(got, want) and not got[~keep].any() and 0 < got.sum() < keep.sum()
        # all samples, hwe off: fpca_snp_qc's decision
        assert np.array_equal(ctx.snp_qc_samples(None, maf=0.05, geno=0.01), ctx.snp_qc(maf=0.05, geno=0.01))
    print("%s: %d x %d; dropped by mind %s: %s; by hwe %s: %s" % (name, N, P, MIND, drops, HWE, hdrops))
    assert (tuple(drops), tuple(hdrops)) == GOLDEN[name]


# ---- end to end --------------------------------------------------------------------------------------------------------
ARRAYS = ("values", "vectors", "projection", "projection_all", "loadings", "center", "scale", "pve")


def yardstick_masks(g, mind, geno, hwe, maf, keep=None):
    """flashpca()'s order on the unpacked codes: mind over all SNPs (among keep), then geno / hwe / maf over the survivors."""
    N, P = g["N"], g["P"]
    samples = Y.sample_rule(g["smp"], P, mind, np.ones(N, dtype=bool) if keep is None else keep)
    sub = Y.snp_counts(g["codes"], samples)
    p_sub, margin = Y.hwe_longdouble(sub)
    assert float(margin.min()) >= 2.0 ** -30 and float(np.abs(p_sub / LD(hwe) - 1).min()) >= 1e-6
    return samples, Y.snp_rule(sub, int(samples.sum()), maf, geno, hwe, p_sub, np.ones(P, dtype=bool))


def test_flashpca_with_the_four_filters(fp):
    g = golden("hapmap3_data")
    kw = dict(mind=0.005, geno=0.01, hwe=1e-4, maf=0.05)
    samples, snps = yardstick_masks(g, **kw)
    assert samples.sum() == 910
    qs, qp = fp.qc_filter(HM3, **kw)
    assert qs.dtype == np.bool_ and qp.dtype == np.bool_ and np.array_equal(qs, samples) and np.array_equal(qp, snps)
    r = fp.flashpca(HM3, ndim=5, do_loadings=True, **kw)
    assert np.array_equal(r["mind_kept"], samples) and np.array_equal(r["snps_kept"], snps)
    f = fp.flashpca(HM3, ndim=5, do_loadings=True, snps=snps, keep=samples)
    for key in ARRAYS:
        assert np.array_equal(f[key], r[key], equal_nan=True), key
    assert r["vectors"].shape == (910, 5) and r["projection_all"].shape == (g["N"], 5) and r["loadings"].shape == (int(snps.sum()), 5)
    print("flashpca(mind=0.005, geno=0.01, hwe=1e-4, maf=0.05): %d of %d samples, %d of %d SNPs" % (samples.sum(), g["N"], snps.sum(), g["P"]))
    # the same with unrelated=: the cutoff runs among the survivors, on the selected SNPs
    r = fp.flashpca(HM3, ndim=5, do_loadings=True, unrelated=0.0884, **kw)
    assert np.array_equal(r["mind_kept"], samples) and np.array_equal(r["snps_kept"], snps)
    un = r["unrelated_kept"]
    assert not un[~samples].any() and 2 <= un.sum() < samples.sum()
    f = fp.flashpca(HM3, ndim=5, do_loadings=True, snps=snps, keep=samples, unrelated=0.0884)
    assert np.array_equal(f["unrelated_kept"], un)
    for key in ARRAYS:
        assert np.array_equal(f[key], r[key], equal_nan=True), key
    print("   with unrelated=0.0884: %d samples" % un.sum())


def test_flashpca_mind_alone_and_with_keep(fp):
    g = golden("hapmap3_data")
    N, P = g["N"], g["P"]
    keep = np.random.default_rng(5).random(N) < 0.7
    want = Y.sample_rule(g["smp"], P, 0.005, keep)
    assert 2 <= want.sum() < keep.sum()
    r = fp.flashpca(HM3, ndim=5, do_loadings=True, keep=keep, mind=0.005)
    assert np.array_equal(r["mind_kept"], want) and "snps_kept" not in r
    f = fp.flashpca(HM3, ndim=5, do_loadings=True, keep=want)
    for key in ARRAYS:
        assert np.array_equal(f[key], r[key], equal_nan=True), key
    qs, qp = fp.qc_filter(HM3, mind=0.005, keep=keep)
    assert np.array_equal(qs, want) and qp.all()
    # qc_filter takes keep= with every filter: frequencies over the hand-picked samples
    samples, snps = yardstick_masks(g, 0.005, 0.01, 1e-4, 0.05, keep=keep)
    qs, qp = fp.qc_filter(HM3, mind=0.005, geno=0.01, hwe=1e-4, maf=0.05, keep=keep)
    assert np.array_equal(qs, samples) and np.array_equal(qp, snps)
    # a snps= list comes first: the missing rate is over the listed SNPs
    listed = np.arange(P) % 5 == 0
    want = Y.sample_rule(Y.sample_counts(g["codes"], listed), int(listed.sum()), 0.005, np.ones(N, dtype=bool))
    qs, qp = fp.qc_filter(HM3, mind=0.005, snps=listed)
    assert np.array_equal(qs, want) and np.array_equal(qp, listed)
    print("keep= (%d) plus mind=0.005: %d samples; mind over every fifth SNP: %d" % (keep.sum(), r["mind_kept"].sum(), want.sum()))
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, keep=keep, hwe=1e-4)
