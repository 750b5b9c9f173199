"""The genotype census and the two QC rules without a GPU: the five entry points in the header, the three hooks in the debug header only,
the binding and both builds of the library; the refusals that need no device; the --mind rule and the --geno / --maf / --hwe rule through
the host-only hooks fpca_debug_sample_qc_rule / fpca_debug_snp_qc_counts_rule against numpy (tests/qc_yardstick.py) -- thresholds exactly
at a value, entries that start at 0, no SNP counted, NaN thresholds --; the counts rule against fpca_debug_snp_qc_rule on the counts of the
four golden filesets; the Python argument refusals; and the compiler's resource remarks for the three kernels."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qc_yardstick as Y  # noqa: E402

ROOT = Y.ROOT
HM3 = os.path.join(Y.GOLD, "hapmap3_data")
NAN = float("nan")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


@pytest.fixture(scope="module", params=["product", "testhooks"])
def L(request, built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    return _lib._load(fp.LIB_PATH if request.param == "product" else fp.HOOKS_LIB_PATH)


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    for proto in ("int fpca_snp_counts(fpca_ctx *ctx, const uint8_t *samples /* [N] or NULL */, uint32_t *counts /* [P_g][4] */);",
                  "int fpca_sample_counts(fpca_ctx *ctx, const uint8_t *snps /* [P_g] or NULL */, uint32_t *counts /* [N][4] */);",
                  "int fpca_hwe_exact(fpca_ctx *ctx, const uint32_t *counts /* [n][4] */, uint64_t n, double *p /* [n] */);",
                  "int fpca_sample_qc(fpca_ctx *ctx, const uint8_t *snps /* [P_g] or NULL */, double max_missing, uint8_t *samples /* [N] in/out */, uint64_t *n_kept);",
                  "int fpca_snp_qc_samples(fpca_ctx *ctx, const uint8_t *samples /* [N] or NULL */, double min_maf, double max_missing, double min_hwe_p,"):
        assert re.search("^" + re.escape(proto), main, re.M), proto
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    for word in ("mid-p", "founders-only", "byte parity with the plink binary"):
        assert word in main, word  # what is not claimed is said in the header
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    hooks = ("fpca_debug_sample_qc_rule", "fpca_debug_snp_qc_counts_rule", "fpca_bench_qc")
    for h in hooks:
        assert h + "(" in dbg and h not in main, h
    names = ("fpca_snp_counts", "fpca_sample_counts", "fpca_hwe_exact", "fpca_sample_qc", "fpca_snp_qc_samples") + hooks
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        lib = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(lib, name) is not None, (path, name)
    # the switch of the test build is not in the product (its name is nowhere in the shipped binary)
    assert b"FPCA_QC_SLAB_SNPS" not in open(fp.LIB_PATH, "rb").read() and b"FPCA_QC_SLAB_SNPS" in open(fp.HOOKS_LIB_PATH, "rb").read()
    # NULL context: -1 with a message, before any device work
    lib = fp.lib()
    u32, u8, f64 = np.zeros(16, dtype=np.uint32), np.ones(4, dtype=np.uint8), np.zeros(4)
    assert lib.fpca_snp_counts(None, None, _vp(u32)) == -1 and b"fpca_snp_counts (NULL context)" in lib.fpca_last_error()
    assert lib.fpca_sample_counts(None, None, _vp(u32)) == -1 and b"fpca_sample_counts (NULL context)" in lib.fpca_last_error()
    assert lib.fpca_hwe_exact(None, _vp(u32), 4, _vp(f64)) == -1 and b"fpca_hwe_exact (NULL context)" in lib.fpca_last_error()
    assert lib.fpca_sample_qc(None, None, 0.1, _vp(u8), None) == -1 and b"fpca_sample_qc (NULL context)" in lib.fpca_last_error()
    assert lib.fpca_snp_qc_samples(None, None, 0.0, 1.0, 0.0, _vp(u8), None) == -1 and b"fpca_snp_qc_samples (NULL context)" in lib.fpca_last_error()
    assert lib.fpca_bench_qc(None, 1, _vp(f64), None) == -1 and b"fpca_bench_qc (NULL context)" in lib.fpca_last_error()
    # the Python layer
    sig = lambda f: inspect.signature(f).parameters  # noqa: E731
    assert list(sig(fp.Context.snp_counts)) == ["self", "samples"] and sig(fp.Context.snp_counts)["samples"].default is None
    assert list(sig(fp.Context.sample_counts)) == ["self", "snps"] and sig(fp.Context.sample_counts)["snps"].default is None
    assert list(sig(fp.Context.hwe_exact)) == ["self", "counts"]
    q = sig(fp.Context.sample_qc)
    assert list(q) == ["self", "mind", "snps", "keep"] and (q["snps"].default, q["keep"].default) == (None, None)
    q = sig(fp.Context.snp_qc_samples)
    assert list(q) == ["self", "samples", "maf", "geno", "hwe", "keep"]
    assert (q["maf"].default, q["geno"].default, q["hwe"].default, q["keep"].default) == (0.0, 1.0, 0.0, None)
    q = sig(fp.qc_filter)
    assert list(q) == ["prefix", "mind", "geno", "hwe", "maf", "snps", "keep", "device"]
    assert [q[k].default for k in list(q)[1:]] == [1.0, 1.0, 0.0, 0.0, None, None, 0]
    q = sig(fp.flashpca)
    assert (q["mind"].default, q["hwe"].default) == (1.0, 0.0)


def test_python_refusals_before_anything_is_uploaded(built_lib):
    import flashpca_amd as fp

    X = np.zeros((8, 5))
    for kw in (dict(mind=0.05), dict(hwe=1e-6), dict(mind=NAN), dict(hwe=NAN)):
        with pytest.raises(ValueError, match="numeric matrix"):
            fp.flashpca(X, ndim=1, **kw)
    keep = np.ones(957, dtype=bool)
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, hwe=1e-6, keep=keep)
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, hwe=1e-6, mind=0.05, keep=keep)
    # the earlier refusals stay, with mind= beside them
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, maf=0.05, mind=0.05, keep=keep)
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, geno=0.01, mind=0.05, keep=keep)
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, ld=(10, 5, 0.2), mind=0.05, keep=keep)


# ---- the --mind rule -----------------------------------------------------------------------------------------------
def mind_c(L, counts, n_snps, mind, samples):
    s8 = np.ascontiguousarray(samples, dtype=np.uint8).copy()
    c32 = np.ascontiguousarray(counts, dtype=np.uint32)
    n = C.c_uint64(12345)
    rc = L.fpca_debug_sample_qc_rule(_vp(c32), n_snps, len(s8), float(mind), _vp(s8), C.byref(n))
    return rc, s8, n.value


def test_sample_rule_against_numpy(L):
    rng = np.random.default_rng(20261019)
    N, n_snps = 500, 1000
    counts = np.zeros((N, 4), dtype=np.uint32)
    counts[:, 1] = rng.integers(0, 60, N)
    counts[:8, 1] = [0, 9, 10, 11, 49, 50, 51, 1000]  # 10 / 1000 and 50 / 1000 are exactly at the thresholds 0.01 and 0.05 below
    counts[:, 0] = n_snps - counts[:, 1]
    start = (rng.random(N) >= 0.2).astype(np.uint8) * 7  # entries that start at 0; non-zero, not only 1
    start[:8] = 7
    for mind in (0.0, 0.01, 0.05, 0.0595, 0.999, 1.0, 2.0, float("inf")):
        for samples in (np.ones(N, dtype=np.uint8), start):
            ref = Y.sample_rule(counts, n_snps, mind, samples != 0)
            rc, s8, n = mind_c(L, counts, n_snps, mind, samples)
            assert rc == 0 and set(np.unique(s8)) <= {0, 1}
            assert np.array_equal(s8 != 0, ref), mind
            assert n == int(ref.sum()) and not s8[samples == 0].any()
    # exactly at the threshold stays, one more goes
    rc, s8, _ = mind_c(L, counts, n_snps, 0.01, np.ones(N, dtype=np.uint8))
    assert list(s8[:4]) == [1, 1, 1, 0]
    rc, s8, _ = mind_c(L, counts, n_snps, 0.05, np.ones(N, dtype=np.uint8))
    assert list(s8[4:8]) == [1, 1, 0, 0]
    # max_missing >= 1 disables the filter even for a sample without a call; 0 keeps only the samples without a missing call
    rc, s8, n = mind_c(L, counts, n_snps, 1.0, np.ones(N, dtype=np.uint8))
    assert rc == 0 and n == N
    rc, s8, n = mind_c(L, counts, n_snps, 0.0, np.ones(N, dtype=np.uint8))
    assert rc == 0 and n == int((counts[:, 1] == 0).sum())


def test_sample_rule_refusals(L):
    counts = np.zeros((4, 4), dtype=np.uint32)
    ones = np.ones(4, dtype=np.uint8)
    for n_snps, mind, word in ((0, 0.05, b"no SNP is counted"), (0, 1.0, b"no SNP is counted"), (10, NAN, b"NaN"), (10, -0.01, b"negative")):
        rc, s8, _ = mind_c(L, counts, n_snps, mind, ones)
        assert rc == -1 and word in L.fpca_last_error() and list(s8) == [1, 1, 1, 1], (n_snps, mind)
    assert L.fpca_debug_sample_qc_rule(_vp(counts), 10, 4, 0.05, None, None) == -1
    assert L.fpca_debug_sample_qc_rule(None, 10, 4, 0.05, _vp(ones), None) == -1


# ---- the --geno / --maf / --hwe rule -------------------------------------------------------------------------------
def snp_c(L, counts, n, maf, geno, hwe, p, keep):
    k8 = np.ascontiguousarray(keep, dtype=np.uint8).copy()
    c32 = np.ascontiguousarray(counts, dtype=np.uint32)
    p64 = None if p is None else np.ascontiguousarray(p, dtype=np.float64)
    nk = C.c_uint64(12345)
    rc = L.fpca_debug_snp_qc_counts_rule(_vp(c32), _vp(p64), n, len(k8), float(maf), float(geno), float(hwe), _vp(k8), C.byref(nk))
    return rc, k8, nk.value


def test_snp_rule_against_numpy(L):
    rng = np.random.default_rng(7)
    P, n = 2000, 400
    miss = rng.integers(0, 30, P)
    miss[:6] = [0, 3, 4, 5, 400, 399]  # 4 / 400 is exactly geno = 0.01; 400: no call at all; 399: one call
    good = n - miss
    c0 = (rng.random(P) * 0.3 * good).astype(np.int64)
    c2 = (rng.random(P) * (good - c0)).astype(np.int64)
    c0[6:10], c2[6:10], miss[6:10] = [0, 0, 19, 19], [40, 39, 2, 1], 0  # maf 40 / 800 = 0.05 exactly, one below, and again via hom A1
    good = n - miss
    counts = np.stack([c0, miss, c2, good - c0 - c2], axis=1).astype(np.uint32)
    assert (counts.sum(axis=1) == n).all()
    p = rng.random(P)
    p[10:14] = [1e-6, np.nextafter(1e-6, 0), 0.0, 1.0]  # exactly at hwe = 1e-6, just below
    start = (rng.random(P) >= 0.2).astype(np.uint8) * 200
    start[:14] = 1
    for maf, geno, hwe in ((0, 1, 0), (0.05, 1, 0), (0, 0.01, 0), (0, 1, 1e-6), (0.05, 0.01, 1e-6), (0.5, 0.0, 1.0), (0.01, 0.05, 0.3), (-1, 2, -1)):
        for keep in (np.ones(P, dtype=np.uint8), start):
            ref = Y.snp_rule(counts, n, maf, geno, hwe, p, keep != 0)
            rc, k8, nk = snp_c(L, counts, n, maf, geno, hwe, p, keep)
            assert rc == 0 and set(np.unique(k8)) <= {0, 1}
            assert np.array_equal(k8 != 0, ref), (maf, geno, hwe)
            assert nk == int(ref.sum()) and not k8[keep == 0].any()
    ones = np.ones(P, dtype=np.uint8)
    _, k8, _ = snp_c(L, counts, n, 0, 0.01, 0, None, ones)  # geno: exactly at the threshold stays
    assert list(k8[:6]) == [1, 1, 1, 0, 0, 0]
    _, k8, _ = snp_c(L, counts, n, 0.05, 1, 0, None, ones)  # maf: exactly at the threshold stays; a SNP without a call counts as maf 0
    assert list(k8[6:10]) == [1, 0, 1, 0] and k8[4] == 0
    _, k8, _ = snp_c(L, counts, n, 0, 1, 1e-6, p, ones)     # hwe: exactly at the threshold stays
    assert list(k8[10:14]) == [1, 0, 0, 1]
    rc, k8, nk = snp_c(L, counts, n, 0, 1, 0, None, ones)   # everything off: p is not read
    assert rc == 0 and nk == P


def test_snp_rule_refusals(L):
    counts = np.tile(np.array([5, 0, 5, 5], dtype=np.uint32), (4, 1))
    p, ones = np.ones(4), np.ones(4, dtype=np.uint8)
    for maf, geno, hwe, word in ((NAN, 1, 0, b"NaN"), (0, NAN, 0, b"NaN"), (0, 1, NAN, b"NaN"), (0.6, 1, 0, b"above 0.5"), (0, -0.1, 0, b"negative"),
                                 (0, 1, 1.5, b"above 1")):
        rc, k8, _ = snp_c(L, counts, 15, maf, geno, hwe, p, ones)
        assert rc == -1 and word in L.fpca_last_error() and list(k8) == [1, 1, 1, 1], (maf, geno, hwe)
    assert snp_c(L, counts, 0, 0.05, 1, 0, p, ones)[0] == -1       # no sample
    assert snp_c(L, counts, 15, 0, 1, 1e-6, None, ones)[0] == -1  # hwe on, no p-values
    assert L.fpca_debug_snp_qc_counts_rule(_vp(counts), _vp(p), 15, 4, 0.0, 1.0, 0.0, None, None) == -1


@pytest.mark.parametrize("name", Y.FILESETS)
def test_counts_rule_agrees_with_the_k1_rule_on_the_golden_filesets(L, name):
    """All samples, hwe off: the decision from the counts is the decision of fpca_snp_qc's rule from K1's mean and missing count."""
    codes, N, P = Y.golden_codes(name)
    counts = Y.snp_counts(codes)
    c = counts.astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (2 * c[:, 0] + c[:, 2]).astype(np.float64) / (c[:, 0] + c[:, 2] + c[:, 3]).astype(np.float64)  # K1: one divide of two integers
    nmiss = np.ascontiguousarray(counts[:, 1])
    dropped = []
    for maf in (0.01, 0.05, 0.5):
        for geno in (0, 0.005, 0.01):
            k1 = np.ones(P, dtype=np.uint8)
            n1 = C.c_uint64(0)
            assert L.fpca_debug_snp_qc_rule(_vp(mean), _vp(nmiss), N, P, maf, float(geno), _vp(k1), C.byref(n1)) == 0
            rc, k8, nk = snp_c(L, counts, N, maf, geno, 0.0, None, np.ones(P, dtype=np.uint8))
            assert rc == 0 and np.array_equal(k8, k1) and nk == n1.value, (maf, geno)
            assert np.array_equal(k8 != 0, Y.snp_rule(counts, N, maf, geno, 0.0, None, np.ones(P, dtype=bool)))
            dropped.append(P - nk)
    print("%s: dropped of %d at maf x geno: %s" % (name, P, dropped))
    assert 0 < max(dropped) <= P


# ---- the kernels' resources ----------------------------------------------------------------------------------------
def test_census_kernels_need_no_scratch():
    """The pattern of tests/test_king_cpu.py: qc_census.hip holds k_snp_counts, the two instances of k_sample_counts and k_hwe_exact, which
    compile without spills and without scratch, by the compiler's own remarks and by the code object's metadata; only k_snp_counts has LDS
    (the 64 bytes of its block reduction, as K1); the per-sample pass combines its slabs with a vector-memory integer atomic add and has
    no float atomic; the HWE kernel has no atomic.  Recorded: k_snp_counts 62 VGPRs, 8 waves/SIMD; k_sample_counts 92 VGPRs, 5 waves/SIMD
    (69 of them the vertical counters), 48 atomic adds each; k_hwe_exact 32 VGPRs, 8 waves/SIMD."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "qc_census.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "qc_census.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    assert len(names) == 4 and sum("k_sample_counts" in n for n in names) == 2, names
    assert sum("k_snp_counts" in n for n in names) == 1 and sum("k_hwe_exact" in n for n in names) == 1, names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0] * 4, key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 8 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * 4
    fn = re.findall(r"Function Name: (\S+)", r.stderr)
    lds = dict(zip(fn, (int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr))))
    occ = dict(zip(fn, (int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr))))
    vgpr = dict(zip(fn, (int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr))))
    print("qc_census.hip: VGPRs %s, occupancy %s, LDS %s" % (vgpr, occ, lds))
    assert len(fn) == 4 and all((v == 64) if "k_snp_counts" in k else (v == 0) for k, v in lds.items()), lds
    assert all(o >= 4 for o in occ.values()), occ
    assert "scratch_" not in txt and "buffer_store" not in txt
    # per kernel: the text between its label and its end marker
    body = {n: txt.split(n + ":", 1)[1].split(".Lfunc_end", 1)[0] for n in names}
    for n, b in body.items():
        adds = len(re.findall(r"global_atomic_add_u32|global_atomic_add ", b))
        if "k_sample_counts" in n:
            assert adds == 48 and "global_atomic_add_f" not in b and "cmpswap" not in b, (n, adds)
            assert len(re.findall(r"global_load_dword ", b)) >= 15, n
        else:
            assert "global_atomic" not in b and "flat_atomic" not in b, n
        if "k_snp_counts" in n:
            assert "global_load_dwordx4" in b and "v_bcnt_u32_b32" in b, n
        if "k_hwe_exact" in n:
            assert "ds_" not in b and "v_div_scale_f64" in b, n
