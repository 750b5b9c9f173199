"""SNP subsets without a GPU: the three entry points in the header, the binding and both builds of the library; snp_filter() on the
.bim files of the fixtures (id lists, ranges, the order of the four steps); the QC rule through the host-only hook
fpca_debug_snp_qc_rule against a numpy restatement, its ties, the zero-call SNP and the threshold refusals; and the register
discipline of the gather kernel."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
CHR1 = os.path.join(GOLD, "data_chr1")
# the reference's exclusion_regions_hg19.txt (long-range LD), written by the tests that need the file
REGIONS = "5 44000000 51500000 r1\n6 25000000 33500000 r2\n8 8000000 12000000 r3\n11 45000000 57000000 r4\n"


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    for proto in ("int fpca_snp_missing(fpca_ctx *ctx, uint32_t *n_missing);",
                  "int fpca_snp_qc(fpca_ctx *ctx, double min_maf, double max_missing, uint8_t *keep, uint64_t *n_kept);",
                  "int fpca_create_snp_subset(fpca_ctx **out, fpca_ctx *src, const uint8_t *keep, int accum);"):
        assert re.search("^" + re.escape(proto), main, re.M), proto
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "fpca_debug_snp_qc_rule(" in dbg and "fpca_debug_snp_subset_bench(" in dbg
    names = ("fpca_snp_missing", "fpca_snp_qc", "fpca_create_snp_subset", "fpca_debug_snp_qc_rule", "fpca_debug_snp_subset_bench")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    assert L.fpca_abi_version() == 4
    # NULL arguments: -1 with a message, before any device work
    keep = np.ones(4, dtype=np.uint8)
    nm = np.zeros(4, dtype=np.uint32)
    n = C.c_uint64(7)
    assert L.fpca_snp_missing(None, _vp(nm)) == -1 and b"fpca_snp_missing (NULL context)" in L.fpca_last_error()
    assert L.fpca_snp_qc(None, 0.05, 1.0, _vp(keep), C.byref(n)) == -1 and b"fpca_snp_qc (NULL context)" in L.fpca_last_error()
    h = C.c_void_p(1234)
    assert L.fpca_create_snp_subset(C.byref(h), None, _vp(keep), 0) == -1 and b"fpca_create_snp_subset (src is NULL)" in L.fpca_last_error()
    assert h.value is None  # (*out is cleared on failure)
    assert L.fpca_create_snp_subset(None, None, _vp(keep), 0) == -1 and b"(out is NULL)" in L.fpca_last_error()
    # the Python layer
    for m in ("snp_missing", "snp_qc", "snp_subset"):
        assert callable(getattr(fp.Context, m))
    p = inspect.signature(fp.flashpca).parameters
    assert p["snps"].default is None and p["maf"].default == 0.0 and p["geno"].default == 1.0
    assert inspect.signature(fp.ucca).parameters["snps"].default is None
    assert list(inspect.signature(fp.snp_filter).parameters) == ["prefix", "extract", "exclude", "extract_ranges", "exclude_ranges"]
    q = inspect.signature(fp.Context.snp_qc).parameters
    assert q["maf"].default == 0.0 and q["geno"].default == 1.0 and q["keep"].default is None
    # matrix input and the combination with keep= are refused before anything is uploaded
    with pytest.raises(ValueError, match="PLINK fileset"):
        fp.flashpca(np.zeros((8, 5)), ndim=1, snps=np.ones(5, dtype=bool))
    with pytest.raises(ValueError, match="PLINK fileset"):
        fp.flashpca(np.zeros((8, 5)), ndim=1, maf=0.05)
    with pytest.raises(ValueError, match="PLINK fileset"):
        fp.ucca(np.zeros((8, 5)), np.zeros((8, 1)), snps=np.ones(5, dtype=bool))
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, maf=0.05, keep=np.ones(957, dtype=bool))
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, geno=0.01, keep=np.ones(957, dtype=bool))


def bim(prefix):
    rows = [l.split() for l in open(prefix + ".bim").read().splitlines() if l.strip()]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([int(r[3]) for r in rows])


def test_snp_filter_ranges(tmp_path):
    import flashpca_amd as fp

    regions = tmp_path / "exclusion_regions_hg19.txt"
    regions.write_text(REGIONS)
    chrom, ids, bp = bim(HM3)
    assert ids.size == 14389
    m = fp.snp_filter(HM3, exclude_ranges=str(regions))
    assert m.dtype == np.bool_ and m.shape == (14389,) and int((~m).sum()) == 53
    # the same selection, restated
    out = np.zeros(ids.size, dtype=bool)
    for c, lo, hi in (("5", 44000000, 51500000), ("6", 25000000, 33500000), ("8", 8000000, 12000000), ("11", 45000000, 57000000)):
        out |= (chrom == c) & (bp >= lo) & (bp <= hi)
    assert np.array_equal(m, ~out)
    assert np.array_equal(fp.snp_filter(HM3, extract_ranges=str(regions)), out)
    # triples instead of a file; a "chr5" / "CHR5" spelling matches
    trip = [("chr5", 44000000, 51500000), ("CHR6", "25000000", "33500000"), (8, 8000000, 12000000), ("11", 45000000, 57000000)]
    assert np.array_equal(fp.snp_filter(HM3, exclude_ranges=trip), m)
    assert fp.snp_filter(CHR1, exclude_ranges=str(regions)).all()  # chromosome 1 only: nothing goes
    # both ends inclusive: a range that begins and ends exactly on a SNP's position includes that SNP, one base pair short does not
    j = int(np.flatnonzero(chrom == "5")[10])
    same = (chrom == chrom[j]) & (bp == bp[j])
    assert np.array_equal(fp.snp_filter(HM3, extract_ranges=[(chrom[j], int(bp[j]), int(bp[j]))]), same)
    k = int(np.flatnonzero(chrom == "5")[20])
    assert bp[k] > bp[j]
    inside = (chrom == "5") & (bp >= bp[j]) & (bp <= bp[k])
    assert np.array_equal(fp.snp_filter(HM3, extract_ranges=[("5", int(bp[j]), int(bp[k]))]), inside)
    short = fp.snp_filter(HM3, extract_ranges=[("5", int(bp[j]) + 1, int(bp[k]) - 1)])
    assert not short[j] and not short[k] and np.array_equal(short, inside & (bp > bp[j]) & (bp < bp[k])) and short.any()
    with pytest.raises(ValueError, match="a range is"):
        fp.snp_filter(HM3, exclude_ranges=[("5", 1)])


def test_snp_filter_id_lists_and_order(tmp_path):
    import flashpca_amd as fp

    chrom, ids, bp = bim(CHR1)
    P = ids.size
    assert fp.snp_filter(CHR1).all() and fp.snp_filter(CHR1).shape == (P,)
    want = [ids[3], ids[100], ids[7], ids[100], "rsNOT_IN_THE_BIM"]  # duplicates are harmless, unknown ids are ignored
    ref = np.isin(ids, want)
    assert int(ref.sum()) >= 3
    assert np.array_equal(fp.snp_filter(CHR1, extract=want), ref)
    assert np.array_equal(fp.snp_filter(CHR1, exclude=want), ~ref)
    f = tmp_path / "ids.txt"  # PLINK's format: the id is the first field, blank lines are skipped, no newline at the end
    f.write_text("%s extra fields\n\n   \n%s\t1\n%s\nrsNOT_IN_THE_BIM\n%s" % (ids[3], ids[100], ids[7], ids[100]))
    assert np.array_equal(fp.snp_filter(CHR1, extract=str(f)), ref)
    assert np.array_equal(fp.snp_filter(CHR1, exclude=str(f)), ~ref)
    with pytest.raises(ValueError, match="none of the listed SNP ids"):
        fp.snp_filter(CHR1, extract=["rsNOPE1", "rsNOPE2"])
    assert fp.snp_filter(CHR1, exclude=["rsNOPE1"]).all()
    # order: extract, extract_ranges, exclude, exclude_ranges
    lo, hi = int(bp[50]), int(bp[400])
    a = fp.snp_filter(CHR1, extract=list(ids[:300]), extract_ranges=[("1", lo, hi)], exclude=list(ids[100:120]),
                      exclude_ranges=[("chr1", int(bp[200]), int(bp[250]))])
    b = np.isin(ids, ids[:300]) & ((chrom == "1") & (bp >= lo) & (bp <= hi)) & ~np.isin(ids, ids[100:120]) & ~((bp >= bp[200]) & (bp <= bp[250]))
    assert np.array_equal(a, b) and 0 < int(a.sum()) < 300
    # an exclude that names an extracted id wins (exclude comes after extract); an extract never brings back what a range left out
    assert not fp.snp_filter(CHR1, extract=[ids[5], ids[6]], exclude=[ids[5]])[5]
    assert not fp.snp_filter(CHR1, extract=[ids[5]], extract_ranges=[("1", int(bp[500]), int(bp[600]))]).any()


# ---- the QC rule -------------------------------------------------------------------------------------------
def rule_numpy(mean, nm, N, maf, geno, keep):
    """include/fpca.h, restated: p = mean / 2, maf = min(p, 1 - p) (0 without a call), dropped when maf < min_maf; miss = n_missing / N,
    dropped when miss > max_missing; both strict; entries that are 0 stay 0."""
    with np.errstate(invalid="ignore"):
        p = mean / 2.0
        m = np.minimum(p, 1.0 - p)
    m = np.where((nm >= N) | np.isnan(p), 0.0, m)
    out = np.asarray(keep) != 0
    if maf > 0:
        out = out & ~(m < maf)
    if geno < 1:
        out = out & ~(nm.astype(np.float64) / np.float64(N) > geno)
    return out


def rule_c(L, mean, nm, N, maf, geno, keep):
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    nm = np.ascontiguousarray(nm, dtype=np.uint32)
    k8 = np.ascontiguousarray(np.asarray(keep), dtype=np.uint8).copy()
    n = C.c_uint64(0)
    rc = L.fpca_debug_snp_qc_rule(_vp(mean), _vp(nm), N, mean.size, float(maf), float(geno), _vp(k8), C.byref(n))
    return rc, k8, n.value


@pytest.fixture(scope="module", params=["product", "testhooks"])
def L(request, built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    return _lib._load(fp.LIB_PATH if request.param == "product" else fp.HOOKS_LIB_PATH)


def test_qc_rule_against_numpy(L):
    rng = np.random.default_rng(20261018)
    N, P = 957, 5000
    nm = rng.integers(0, 40, P).astype(np.uint32)
    nm[rng.random(P) < 0.01] = N  # SNPs without a single call
    good = N - nm.astype(np.int64)
    freq = rng.beta(0.4, 0.4, P)  # many rare variants, either allele
    n2 = rng.binomial(good, freq ** 2)
    n1 = rng.binomial(good - n2, np.clip(2 * freq * (1 - freq) / np.maximum(1 - freq ** 2, 1e-300), 0, 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (2 * n2 + n1).astype(np.float64) / good.astype(np.float64)  # K1's formula: NaN without a call
    assert np.isnan(mean).sum() == (nm == N).sum() > 0
    keep_in = (rng.random(P) < 0.8).astype(np.uint8) * rng.integers(1, 255, P).astype(np.uint8)  # non-zero, not only 1
    for maf, geno in ((0.05, 1.0), (0.0, 0.02), (0.01, 0.01), (0.5, 0.0), (0.0, 1.0), (-1.0, 2.0), (0.2, 0.5)):
        rc, k8, n = rule_c(L, mean, nm, N, maf, geno, keep_in)
        ref = rule_numpy(mean, nm, N, maf, geno, keep_in)
        assert rc == 0 and set(np.unique(k8)) <= {0, 1}
        assert np.array_equal(k8 != 0, ref), (maf, geno)
        assert n == int(ref.sum())
        assert not k8[keep_in == 0].any()  # entries that are 0 on input stay 0
        if maf <= 0 and geno >= 1:
            assert np.array_equal(k8 != 0, keep_in != 0)  # both filters off: only the normalisation to 0 / 1
        else:
            assert not k8[nm == N].any()  # a zero-call SNP goes under either active filter
    assert 0 < int(rule_numpy(mean, nm, N, 0.05, 1.0, keep_in).sum()) < int((keep_in != 0).sum())


def test_qc_rule_ties_and_zero_call_snp(L):
    N = 200
    ones = np.ones(4, dtype=np.uint8)
    # exactly at the threshold: kept; just beyond: dropped (strict comparisons, as in PLINK)
    mean = np.array([0.1, 0.09, 1.9, 1.0])
    nm = np.array([2, 2, 3, 3], dtype=np.uint32)
    rc, k8, n = rule_c(L, mean, nm, N, 0.05, 1.0, ones)
    assert 1.0 - 1.9 / 2.0 >= 0.05  # (0.05000000000000004 in binary: the major-allele side of the tie is not exact, and stays as well)
    assert rc == 0 and list(k8) == [1, 0, 1, 1] and n == 3  # mean 0.1 -> maf 0.05 stays, mean 0.09 -> 0.045 goes
    rc, k8, n = rule_c(L, mean, nm, N, 0.0, 0.01, ones)
    assert rc == 0 and list(k8) == [1, 1, 0, 0] and n == 2  # 2 of 200 missing = 0.01 stays, 3 of 200 goes
    # a SNP without a single call (mean = 0 / 0): maf 0 and missing rate 1
    mean = np.array([np.nan, 1.0])
    nm = np.array([N, 0], dtype=np.uint32)
    assert list(rule_c(L, mean, nm, N, 1e-300, 1.0, ones[:2])[1]) == [0, 1]
    assert list(rule_c(L, mean, nm, N, 0.0, 0.999, ones[:2])[1]) == [0, 1]
    assert list(rule_c(L, mean, nm, N, 0.0, 1.0, ones[:2])[1]) == [1, 1]  # no filter active
    # entries that are 0 on input stay 0, whatever the SNP
    assert list(rule_c(L, np.array([1.0, 1.0]), np.array([0, 0], dtype=np.uint32), N, 0.05, 0.01, np.array([0, 9], dtype=np.uint8))[1]) == [0, 1]


def test_qc_rule_threshold_refusals(L):
    mean, nm, ones = np.array([1.0]), np.zeros(1, dtype=np.uint32), np.ones(1, dtype=np.uint8)
    for maf, geno, msg in ((np.nan, 1.0, b"NaN"), (0.05, np.nan, b"NaN"), (0.51, 1.0, b"above 0.5"), (0.0, -0.01, b"negative")):
        rc, k8, _ = rule_c(L, mean, nm, 10, maf, geno, ones)
        assert rc == -1 and msg in L.fpca_last_error(), (maf, geno, L.fpca_last_error())
        assert list(k8) == [1]  # (nothing is written by a refused call)
    assert rule_c(L, mean, nm, 10, 0.5, 0.0, ones)[0] == 0  # the limits themselves are valid
    n = C.c_uint64(0)
    assert L.fpca_debug_snp_qc_rule(None, _vp(nm), 10, 1, 0.0, 1.0, _vp(ones), C.byref(n)) == -1


def test_gather_kernel_does_not_spill():
    """The pattern of tests/test_subset_cpu.py: the kernel of snp_subset.hip compiles without spills, scratch or LDS, by the compiler's own
    remarks and by the code object's metadata, and moves its bytes as 16-byte vectors."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "snp_subset.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "snp_subset.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    assert len(names) == 1 and "k_gather_records" in names[0], names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0], key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 2 and all(int(v) == 0 for _, v in remarks), remarks
    assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr).group(1)) == 8
    assert len(re.findall(r"global_load_dwordx4", txt)) >= 4 and len(re.findall(r"global_store_dwordx4", txt)) >= 4
