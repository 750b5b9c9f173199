"""SNP subsets (fpca_snp_missing, fpca_snp_qc, fpca_create_snp_subset; snp_filter(), flashpca(snps=, maf=, geno=), ucca(snps=)) on the GPU
against the CPU oracle, which never sees the feature: the kept records of the raw 2-bit codes are RE-PACKED with numpy and given to
OracleData and to fpca_create -- the scheme of tests/test_gpu_subset.py, on the other axis.

A subset context must hold byte for byte what fpca_create builds from the re-packed records.  The download shows the np valid bytes of every
kept record only (fpca_download_packed clears the pad bits and sees neither the pitch padding nor the records [P_kept, P_pad)); the rest of
the contract is checked through what depends on it: statistics, missing counts, the route and every operator result array_equal to the
fpca_create context's.  So every result is compared twice: with
the oracle at the tolerance this project already holds the quantity to (tests/test_gpu_subset.py, tests/test_gpu_pca.py,
tests/test_gpu_ucca.py: statistics array_equal, trace 1e-12 relative, operator 1e-11 of the largest entry, fp32 2e-6; against
oracle.pca_fast eigenvalues 1e-6, pve 1e-8, the five leading vectors and loadings 1e-5; against dense eigh eigenvalues 1e-9, |u'u_ref|
within 1e-8 of 1, U'U within 1e-10 of I, pve 1e-11, held-out projections and loadings 1e-11; UCCA R 1e-10, F 4e-10, P 1e-8), and with the
same call on the fpca_create context, array_equal -- same bytes, same shape, same plan, fixed-order combines.
Every test prints what it measured (pytest -s).
Measured on the MI355X (profiles/snp_subset_test_figures.txt): the 30 (source, mask) downloads equal both yardsticks; mean / sd and the
missing counts array_equal everywhere, trace <= 9.1e-16; operator (apply_xt / apply_x / apply_xxt) 1.3e-15 / 1.0e-15 / 1.0e-15 (fp64),
1.1e-15 / 1.8e-15 / 1.0e-15 (exact-integer; routes 3 and 4), 6.0e-7 / 6.8e-7 / 6.4e-7 (fp32), every result array_equal to the fpca_create
context's; maf 0.05 drops 425 SNPs of hapmap3_data, geno 0.005 drops 1,473; end to end against pca_fast eigenvalues 2.1e-13, pve 1.7e-14,
vectors 2.5e-10, loadings 2.1e-11; with keep= against dense eigh eigenvalues 1.6e-15, |u'u_ref| - 1 1.8e-15, U'U - I 2.4e-15, pve 1.2e-17,
held-out Px 5.7e-16, V 1.0e-15; UCCA rows identical to the unfiltered scan's (0.0)."""
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


# ---- the yardstick (the helpers of tests/test_gpu_subset.py) --------------------------------------------------
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


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def oracle_of(O, codes, stand="binom2"):
    """The oracle on re-packed records: dense standardised matrix, mean / sd, trace."""
    P, N = codes.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(packed=pack_codes(codes), N=N, P=P, stand=stand)
        X, ms = od.dense(), od.meansd()
    return X, ms, float(np.sum(X * X))


def masks_for(P):
    rng = np.random.default_rng(20261018)
    ar = np.arange(P)
    m = {"all": ar >= 0, "first_only": ar == 0, "last_only": ar == P - 1, "first255": ar < 255, "first256": ar < 256, "first257": ar < 257,
         "all_but_last": ar < P - 1, "every_other": ar % 2 == 0, "random70": rng.random(P) < 0.7, "middle_run": (ar >= P // 3) & (ar < P // 3 + P // 4)}
    assert all(v.any() for v in m.values()) and 0.6 * P < m["random70"].sum() < 0.8 * P
    return m


SOURCES = {"data_chr1": (957, 1129, 256), "synthetic_511x1000": (511, 1000, 128), "synthetic_2049x600": (2049, 600, 640)}


def open_source(fp, name, accum="fp64"):
    N, P, _ = SOURCES[name]
    if name == "data_chr1":
        return fp.Context.from_bed(CHR1 + ".bed", N, accum=accum)
    return fp.Context.synthetic(N, P, n_pop=4, missing_rate=0.01, seed=N, accum=accum)


# ---- 1. bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SOURCES))
def test_subset_bytes(fp, name):
    N, P, pitch = SOURCES[name]
    npb = (N + 3) // 4
    assert (npb + 127) // 128 * 128 == pitch
    with open_source(fp, name) as src:
        assert (src.N, src.P) == (N, P)
        full = src.download_packed().reshape(P, npb)
        codes = unpack_codes(full, N, P)
        for mname, mask in masks_for(P).items():
            kept = int(mask.sum())
            with src.snp_subset(mask) as sub, fp.Context.from_packed(pack_codes(codes[mask]), N, kept) as ref:
                assert (sub.N, sub.P, sub.P_total) == (N, kept, kept) and sub.accum == src.accum
                got = sub.download_packed().reshape(kept, npb)
                same_src = np.array_equal(got, full[mask])
                same_ref = np.array_equal(got, ref.download_packed().reshape(kept, npb))
                print("%s %s: %d of %d records, pitch %d: equal to the source's records %s, to fpca_create of the re-packed records %s" % (
                    name, mname, kept, P, pitch, same_src, same_ref))
                assert same_src and same_ref, (name, mname)
        # index arrays: applied in ascending order, whatever order they come in
        idx = np.array([P - 1, 3, 77, 0, 256])
        with src.snp_subset(idx) as sub:
            assert np.array_equal(sub.download_packed().reshape(5, npb), full[np.sort(idx)])
        for bad in (np.array([1, 1]), np.array([P]), np.array([-1]), np.ones(P - 1, dtype=bool), np.array([0.5])):
            with pytest.raises(ValueError):
                src.snp_subset(bad)
        assert np.array_equal(src.download_packed().reshape(P, npb), full)  # the source is as it was


# ---- 2. statistics -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SOURCES))
@pytest.mark.parametrize("stand", ["binom2", "binom"])
def test_subset_statistics(fp, O, name, stand):
    N, P, _ = SOURCES[name]
    with (fp.Context.from_bed(CHR1 + ".bed", N, stand=stand) if name == "data_chr1" else
          fp.Context.synthetic(N, P, n_pop=4, missing_rate=0.01, seed=N, stand=stand)) as src:
        codes = unpack_codes(src.download_packed(), N, P)
        nm_all = (codes == 1).sum(axis=1).astype(np.uint32)
        assert nm_all.sum() > 0
        for mname in ("random70", "first257", "every_other", "last_only"):
            mask = masks_for(P)[mname]
            _, ms_ref, tr_ref = oracle_of(O, codes[mask], stand)
            with src.snp_subset(mask) as sub:  # (a fresh context: this is its first pass over the compacted matrix)
                ms, tr = sub.stats()
                nm = sub.snp_missing()
            e_tr = abs(tr - tr_ref) / tr_ref if tr_ref > 0 else abs(tr - tr_ref)
            print("%s %s %s: mean / sd equal %s, trace rel err %.2e, missing counts equal %s" % (
                name, stand, mname, np.array_equal(ms, ms_ref, equal_nan=True), e_tr, np.array_equal(nm, nm_all[mask])))
            assert np.array_equal(ms, ms_ref, equal_nan=True), (name, stand, mname)
            assert e_tr <= 1e-12
            assert nm.dtype == np.uint32 and np.array_equal(nm, nm_all[mask])
        assert np.array_equal(src.snp_missing(), nm_all)  # the source's own counts (K1 ran for this call)


# ---- 3. operator ---------------------------------------------------------------------------------------------
def check_operator(O, src, mask, accum, tol, label, fp, b=16):
    N = src.N
    codes = unpack_codes(src.download_packed(), N, src.P)[mask]
    X, _, _ = oracle_of(O, codes)
    kept = int(mask.sum())
    rng = np.random.default_rng(7)
    B, T = rng.standard_normal((N, b)), rng.standard_normal((kept, b))
    with src.snp_subset(mask, accum=accum) as sub, fp.Context.from_packed(pack_codes(codes), N, kept, accum=accum) as ref:
        assert sub.accum == ref.accum
        mode, mode_ref = sub.missing_mode(b), ref.missing_mode(b)
        got = [sub.apply_xt(B), sub.apply_x(T), sub.apply_xxt(B)]
        same = [ref.apply_xt(B), ref.apply_x(T), ref.apply_xxt(B)]
    t_ref = X.T @ B
    e = [relmax(got[0], t_ref), relmax(got[1], X @ T), relmax(got[2], X @ t_ref)]
    eq = [np.array_equal(g, s) for g, s in zip(got, same)]
    print("%s (%s, missing-call route %d): apply_xt %.2e, apply_x %.2e, apply_xxt %.2e; equal to the fpca_create context: %s" % (
        label, accum, mode, e[0], e[1], e[2], eq))
    assert max(e) <= tol, (label, e)
    assert mode == mode_ref and all(eq), (label, mode, mode_ref, eq)
    return e, mode


@pytest.mark.parametrize("accum,tol", [("fp64", 1e-11), ("auto", 1e-11), ("fp32", 2e-6)])
def test_subset_operator(fp, O, accum, tol):
    with open_source(fp, "data_chr1", accum=accum) as src:
        for mname in ("random70", "first257"):
            e, _ = check_operator(O, src, masks_for(src.P)[mname], accum, tol, "data_chr1 %s" % mname, fp)
            if accum == "fp32":
                assert max(e) > 1e-12  # (really fp32)


@pytest.mark.parametrize("accum,tol", [("fp64", 1e-11), ("auto", 1e-11), ("fp32", 2e-6)])
def test_subset_operator_with_concentrated_missing_calls(fp, O, accum, tol):
    """The realistic profile (missing_model 1: the missing calls sit in few SNPs).  Half of those SNPs and 70 % of the others are kept, so the
    subset's route -- hybrid or sparse -- follows from its own K1 counts, not from the source's."""
    N, P = 3000, 2000
    with fp.Context.synthetic(N, P, n_pop=3, realistic=True, accum=accum) as src:
        nm = src.snp_missing()
        dense_snps = nm > 20 * max(np.median(nm), 1)
        rng = np.random.default_rng(8)
        mask = np.where(dense_snps, rng.random(P) < 0.5, rng.random(P) < 0.7)
        print("source: %d SNPs hold %d of %d missing calls; kept %d of them, %d SNPs in all; source route %d" % (
            dense_snps.sum(), nm[dense_snps].sum(), nm.sum(), (mask & dense_snps).sum(), mask.sum(), src.missing_mode(16)))
        assert 10 <= (mask & dense_snps).sum() < dense_snps.sum()
        _, mode = check_operator(O, src, mask, accum, tol, "realistic profile", fp)
        assert mode in ((3, 4) if accum == "auto" else (-1,))


# ---- 4. QC ---------------------------------------------------------------------------------------------------
def qc_numpy(ms, nm, N, maf, geno):
    with np.errstate(invalid="ignore"):
        p = ms[:, 0] / 2.0
        m = np.minimum(p, 1.0 - p)
    m = np.where((nm >= N) | np.isnan(p), 0.0, m)
    out = np.ones(nm.size, dtype=bool)
    if maf > 0:
        out &= ~(m < maf)
    if geno < 1:
        out &= ~(nm.astype(np.float64) / np.float64(N) > geno)
    return out


def test_snp_qc_on_hapmap3(fp, O, tmp_path):
    codes, N, P = read_bed_codes(HM3)
    assert (N, P) == (957, 14389)
    nm = (codes == 1).sum(axis=1)
    assert nm.max() == 9
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(HM3 + ".bed", N, "binom2")
        od.dense()  # (the oracle takes its statistics while it reads the blocks)
        ms = od.meansd()
    regions = tmp_path / "regions.txt"
    regions.write_text(REGIONS)
    ranges = fp.snp_filter(HM3, exclude_ranges=str(regions))
    assert int((~ranges).sum()) == 53
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        by_maf = ctx.snp_qc(maf=0.05)
        by_geno = ctx.snp_qc(geno=0.005)
        both = ctx.snp_qc(maf=0.05, geno=0.005)
        composed = ctx.snp_qc(maf=0.05, geno=0.005, keep=ranges)
        by_index = ctx.snp_qc(maf=0.05, keep=np.flatnonzero(ranges))
        none = ctx.snp_qc()
        assert np.array_equal(ctx.snp_missing(), nm)
    print("hapmap3_data: maf 0.05 drops %d, geno 0.005 drops %d, both %d, with the 53 range SNPs %d of %d" % (
        (~by_maf).sum(), (~by_geno).sum(), (~both).sum(), (~composed).sum(), P))
    assert by_maf.dtype == np.bool_ and int((~by_maf).sum()) == 425
    assert np.array_equal(by_maf, qc_numpy(ms, nm, N, 0.05, 1.0))
    assert np.array_equal(by_geno, nm < 5) and 0 < int((~by_geno).sum()) < P  # 4 / 957 = 0.0042 stays, 5 / 957 = 0.0052 goes
    assert np.array_equal(by_geno, qc_numpy(ms, nm, N, 0.0, 0.005))
    assert np.array_equal(both, by_maf & by_geno)
    assert np.array_equal(composed, both & ranges) and np.array_equal(by_index, by_maf & ranges)
    assert none.all()


def test_snp_qc_refusals(fp):
    codes, N, P = read_bed_codes(CHR1)

    def refused(call, msg):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == -1

    with fp.Context.from_bed(CHR1 + ".bed", N, accum="auto") as ctx:
        ctx.set_sample_mask(np.arange(N) % 3 != 0)
        refused(lambda: ctx.snp_qc(maf=0.05), "fpca_snp_qc: a sample mask is set")
        refused(lambda: ctx.snp_missing(), "fpca_snp_missing: a sample mask is set")
        ctx.set_sample_mask(None)
        assert int(ctx.snp_qc(maf=0.05).sum()) > 0  # (cleared: the call runs)
        for maf, geno, msg in ((float("nan"), 1.0, "NaN"), (0.6, 1.0, "above 0.5"), (0.0, -0.1, "negative")):
            refused(lambda: ctx.snp_qc(maf=maf, geno=geno), msg)
        with pytest.raises(ValueError):
            ctx.snp_qc(maf=0.05, keep=np.ones(P + 1, dtype=bool))
        # the scripting entry point does not take a NaN threshold for "no filter"
        for kw in (dict(maf=float("nan")), dict(geno=float("nan"))):
            with pytest.raises(fp.FpcaError, match="NaN") as e:
                fp.flashpca(CHR1, ndim=2, **kw)
            assert e.value.code == -1
        ctx.set_meansd(ctx.stats()[0])
        refused(lambda: ctx.snp_qc(maf=0.05), "fpca_snp_qc: this context carries a preloaded mean/sd")
        refused(lambda: ctx.snp_missing(), "fpca_snp_missing: this context carries a preloaded mean/sd")
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.snp_qc(maf=0.05), "fpca_snp_qc: this context holds a dense matrix")
        refused(lambda: dense.snp_missing(), "fpca_snp_missing: this context holds a dense matrix")


# ---- 5. end to end -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hm3(fp, tmp_path_factory):
    codes, N, P = read_bed_codes(HM3)
    regions = tmp_path_factory.mktemp("regions") / "exclusion_regions_hg19.txt"
    regions.write_text(REGIONS)
    return dict(codes=codes, N=N, P=P, ranges=fp.snp_filter(HM3, exclude_ranges=str(regions)))


def test_flashpca_with_snp_filters_against_the_oracle(fp, O, hm3):
    """oracle.pca_fast (the restated reference path, Spectra-style IRLM at the reference's defaults) on the re-packed subset; the
    tolerances of tests/test_gpu_pca.py::test_pca_vs_oracle_reference_path, which compares the same two solvers at the same settings."""
    codes, N, P = hm3["codes"], hm3["N"], hm3["P"]
    r = fp.flashpca(HM3, ndim=10, snps=hm3["ranges"], maf=0.05, do_loadings=True)
    mask = r["snps_kept"]
    nm = (codes == 1).sum(axis=1)
    _, ms_all, _ = oracle_of(O, codes)
    assert mask.dtype == np.bool_ and np.array_equal(mask, hm3["ranges"] & qc_numpy(ms_all, nm, N, 0.05, 1.0))
    kept = int(mask.sum())
    assert kept == P - 53 - int((hm3["ranges"] & ~qc_numpy(ms_all, nm, N, 0.05, 1.0)).sum()) and kept < P - 53
    assert r["loadings"].shape == (kept, 10) and r["center"].shape == (kept,) and r["scale"].shape == (kept,) and r["vectors"].shape == (N, 10)
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(packed=pack_codes(codes[mask]), N=N, P=kept, stand="binom2")
        ref = O.pca_fast(od, 10, do_loadings=True)
    e_d = float(np.max(np.abs(r["values"] - ref["d"]) / ref["d"]))  # (divisor p = the kept count on both sides)
    e_pve = float(np.max(np.abs(r["pve"] - ref["pve"])))
    e_u = e_v = 0.0
    for c in range(5):  # well-separated components; up to sign
        s = np.sign(ref["U"][:, c] @ r["vectors"][:, c])
        e_u = max(e_u, float(np.max(np.abs(ref["U"][:, c] * s - r["vectors"][:, c]))))
        e_v = max(e_v, float(np.max(np.abs(ref["V"][:, c] * s - r["loadings"][:, c]))))
    U = r["vectors"]
    e_o = float(np.max(np.abs(U.T @ U - np.eye(10))))
    print("flashpca(snps=ranges, maf=0.05): %d of %d SNPs; against pca_fast eigenvalues %.2e, pve %.2e, vectors %.2e, loadings %.2e; U'U - I %.2e; "
          "%d block applies" % (kept, P, e_d, e_pve, e_u, e_v, e_o, r["info"]["block_applies"]))
    assert e_d < 1e-6 and e_pve < 1e-8 and e_u < 1e-5 and e_v < 1e-5 and e_o < 1e-10
    assert np.array_equal(r["center"], ref["meansd"][:, 0]) and np.array_equal(r["scale"], ref["meansd"][:, 1])
    assert np.allclose(r["projection"], U * np.sqrt(r["values"]), rtol=1e-14, atol=0)
    # an index array selects what the mask selects; without a filter the result is what it was
    r2 = fp.flashpca(HM3, ndim=10, snps=np.flatnonzero(mask)[::-1], do_loadings=True)
    assert np.array_equal(r2["snps_kept"], mask) and np.array_equal(r2["values"], r["values"]) and np.array_equal(r2["loadings"], r["loadings"])
    assert "snps_kept" not in fp.flashpca(HM3, ndim=3)
    # the dimension limit is that of the kept count
    few = np.zeros(P, dtype=bool)
    few[:9] = True
    with pytest.raises(fp.FpcaError, match="You asked for 5 dimensions, but only 4 allowed"):
        fp.flashpca(HM3, ndim=5, snps=few)


def test_flashpca_with_snps_and_a_sample_subset(fp, O, hm3):
    """keep= on the compacted context: kept samples x kept SNPs against dense eigh of the oracle's matrix, held-out samples projected -- the
    checks and tolerances of tests/test_gpu_subset.py::check_pca."""
    codes, N, P = hm3["codes"], hm3["N"], hm3["P"]
    mask = hm3["ranges"]
    keep = np.random.default_rng(20261017).random(N) < 0.7
    k, kept = 10, int(mask.sum())
    r = fp.flashpca(HM3, ndim=k, snps=mask, keep=keep, do_loadings=True, tol=1e-8)
    assert np.array_equal(r["snps_kept"], mask) and r["loadings"].shape == (kept, k)
    sub = codes[mask]
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(packed=pack_codes(sub[:, keep]), N=int(keep.sum()), P=kept, stand="binom2")
        Xs, ms = od.dense(), od.meansd()
        oh = O.OracleData(packed=pack_codes(sub[:, ~keep]), N=int((~keep).sum()), P=kept, stand="binom2")
        oh.set_preloaded_meansd(ms)
        Xh = oh.dense()
    tr = float(np.sum(Xs * Xs))
    w, Q = np.linalg.eigh(Xs @ Xs.T)
    w, Q = w[::-1][:k] / kept, Q[:, ::-1][:, :k]
    U, d, V = r["vectors"], r["values"], r["loadings"]
    e_d = float(np.max(np.abs(d - w) / w))
    e_u = float(np.max(np.abs(np.abs(np.sum(U * Q, axis=0)) - 1.0)))
    e_o = float(np.max(np.abs(U.T @ U - np.eye(k))))
    e_pve = float(np.max(np.abs(r["pve"] - w / (tr / kept))))
    e_px = relmax(r["projection_all"][~keep], Xh @ V / np.sqrt(kept))
    v_ref = Xs.T @ U / np.sqrt(d) / np.sqrt(kept)
    e_v = relmax(V, v_ref)
    print("flashpca(snps=ranges, keep=random70): %d samples x %d SNPs; eigenvalues %.2e, |u'u_ref| - 1 %.2e, U'U - I %.2e, pve %.2e, held-out Px %.2e, "
          "V %.2e" % (keep.sum(), kept, e_d, e_u, e_o, e_pve, e_px, e_v))
    assert e_d <= 1e-9 and e_u <= 1e-8 and e_o <= 1e-10 and e_pve <= 1e-11 and e_px <= 1e-11 and e_v <= 1e-11
    assert np.array_equal(r["center"], ms[:, 0], equal_nan=True) and np.array_equal(r["scale"], ms[:, 1], equal_nan=True)
    assert np.array_equal(r["projection_all"][keep], r["projection"])
    for kw in (dict(maf=0.05), dict(geno=0.01), dict(maf=0.05, snps=mask)):
        with pytest.raises(ValueError, match="cannot be combined with keep"):
            fp.flashpca(HM3, ndim=k, keep=keep, **kw)


def test_ucca_with_snps(fp):
    """A SNP's F test does not depend on the other SNPs: the filtered scan is the selected rows of the unfiltered one (tolerances of
    tests/test_gpu_ucca.py: R 1e-10, F 4e-10, P 1e-8 relative)."""
    N = fp.count_fam_rows(CHR1 + ".fam")
    Y = np.random.default_rng(3).standard_normal((N, 3))
    full = fp.ucca(CHR1, Y, standy="sd")
    P = full["result"].shape[0]
    mask = masks_for(P)["random70"]
    sub = fp.ucca(CHR1, Y, standy="sd", snps=mask)
    a, b = sub["result"], full["result"][mask]
    assert a.shape == (int(mask.sum()), 3) and np.array_equal(sub["snps_kept"], mask) and "snps_kept" not in full
    assert sub["snp_ids"] == [s for s, m in zip(full["snp_ids"], mask) if m] and sub["npheno"] == 3
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b[:, 0])
    e = [float(np.max(np.abs(a[ok, c] - b[ok, c]) / np.abs(b[ok, c]))) for c in range(3)]
    print("ucca(snps=random70) on data_chr1: %d of %d SNPs, %d without variance; R %.2e, F %.2e, P %.2e against the rows of the unfiltered scan" % (
        mask.sum(), P, (~ok).sum(), e[0], e[1], e[2]))
    assert ok.sum() > 0.9 * mask.sum() and b[ok, 2].min() >= 1e-290
    assert e[0] < 1e-10 and e[1] < 4e-10 and e[2] < 1e-8


# ---- 6. refusals of fpca_create_snp_subset -------------------------------------------------------------------------
def test_create_snp_subset_refusals(fp):
    codes, N, P = read_bed_codes(CHR1)
    B = np.random.default_rng(5).standard_normal((N, 16))
    mask = masks_for(P)["random70"]

    def refused(call, msg):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == -1

    with fp.Context.from_bed(CHR1 + ".bed", N, accum="auto") as src:
        before = src.apply_xt(B)
        refused(lambda: src.snp_subset(np.zeros(P, dtype=bool)), "the mask keeps 0 of %d SNPs" % P)
        src.set_rank(2, 0)
        refused(lambda: src.snp_subset(mask), "the source is one shard of several")
        src.set_rank(1, 0)  # (one rank is no sharding)
        with src.snp_subset(mask) as sub:
            assert sub.P == int(mask.sum())
        # a source under a sample mask or with a preloaded mean/sd: the subset is a fresh context and inherits neither
        src.set_sample_mask(np.arange(N) % 2 == 0)
        with src.snp_subset(mask) as sub, fp.Context.from_packed(pack_codes(codes[mask]), N, int(mask.sum()), accum="auto") as ref:
            assert sub.nkept == N and np.array_equal(sub.stats()[0], ref.stats()[0], equal_nan=True)
        src.set_sample_mask(None)
        after = src.apply_xt(B)
        print("the source after two refused and two served calls: apply_xt equal to before: %s" % np.array_equal(before, after))
        assert np.array_equal(before, after)
    with fp.Context.from_bed(CHR1 + ".bed", N, accum="auto") as src:
        src.set_allreduce(lambda ptr, count, stream: 0)
        refused(lambda: src.snp_subset(mask), "the source is one shard of several")
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.snp_subset(np.ones(30, dtype=bool)), "the source holds a dense matrix")
