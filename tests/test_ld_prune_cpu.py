"""LD pruning without a GPU: the two entry points in the header, the binding and both builds of the library; the pruning rule through the
host-only hook fpca_debug_ld_prune_rule against a plain-Python restatement of include/fpca.h (three nested loops, every window visits all
its pairs) on random bitmaps; and the register discipline of the band kernel."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    for proto in ("int fpca_ld_band(fpca_ctx *ctx, uint64_t snp0, uint64_t nsnp, uint32_t span, double *r2 /* [nsnp][span] */);",
                  "int fpca_ld_prune(fpca_ctx *ctx, const uint32_t *chrom /* [P_g] or NULL */, uint32_t window, uint32_t step, double r2,"):
        assert re.search("^" + re.escape(proto), main, re.M), proto
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "fpca_debug_ld_prune_rule(" in dbg and "fpca_bench_ld(" in dbg
    assert "fpca_debug_ld_prune_rule" not in main and "fpca_bench_ld" not in main  # the hooks are not part of the drop-in boundary
    names = ("fpca_ld_band", "fpca_ld_prune", "fpca_debug_ld_prune_rule", "fpca_bench_ld")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    assert L.fpca_abi_version() == 4
    # NULL context: -1 with a message, before any device work
    buf = np.zeros(8)
    keep = np.ones(4, dtype=np.uint8)
    assert L.fpca_ld_band(None, 0, 4, 2, _vp(buf)) == -1 and b"fpca_ld_band (NULL context)" in L.fpca_last_error()
    assert L.fpca_ld_prune(None, None, 10, 5, 0.2, _vp(keep), None) == -1 and b"fpca_ld_prune (NULL context)" in L.fpca_last_error()
    # the Python layer
    for m in ("ld_band", "ld_prune", "bench_ld"):
        assert callable(getattr(fp.Context, m))
    q = inspect.signature(fp.Context.ld_prune).parameters
    assert (q["window"].default, q["step"].default, q["r2"].default, q["chrom"].default, q["keep"].default) == (1000, 50, 0.05, None, None)
    assert list(inspect.signature(fp.ld_prune).parameters)[:7] == ["prefix", "window", "step", "r2", "snps", "maf", "geno"]
    assert inspect.signature(fp.flashpca).parameters["ld"].default is None and inspect.signature(fp.ucca).parameters["ld"].default is None
    # refused before anything is uploaded
    with pytest.raises(ValueError, match="PLINK fileset"):
        fp.flashpca(np.zeros((8, 5)), ndim=1, ld=(10, 5, 0.2))
    with pytest.raises(ValueError, match="PLINK fileset"):
        fp.ucca(np.zeros((8, 5)), np.zeros((8, 1)), ld=(10, 5, 0.2))
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(os.path.join(ROOT, "tests", "golden", "hapmap3_data"), ndim=2, ld=(10, 5, 0.2), keep=np.ones(957, dtype=bool))
    with pytest.raises(ValueError, match="ld is \\(window, step, r2\\)"):
        fp.flashpca(os.path.join(ROOT, "tests", "golden", "hapmap3_data"), ndim=2, ld=(10, 5))


# ---- the rule --------------------------------------------------------------------------------------------------
def rule_python(bits, P, w, s, totals, maf, chrom, keep):
    """include/fpca.h, restated with nothing but loops."""
    words = (w - 1 + 31) // 32
    keep = [bool(k) for k in keep]
    for j in range(P):
        n, sx, sq = (int(v) for v in totals[j])
        if n * sq - sx * sx == 0:
            keep[j] = False
    runs, c0 = [], 0
    for j in range(1, P + 1):
        if j == P or (chrom is not None and chrom[j] != chrom[c0]):
            runs.append((c0, j))
            c0 = j
    for c0, c1 in runs:
        L, o = c1 - c0, 0
        while True:
            end = min(o + w, L)
            for i in range(c0 + o, c0 + end):
                if not keep[i]:
                    continue
                for j in range(i + 1, c0 + end):
                    d = j - i - 1
                    if not keep[j] or not (int(bits[i * words + (d >> 5)]) >> (d & 31)) & 1:
                        continue
                    if maf[i] < maf[j]:
                        keep[i] = False
                        break
                    keep[j] = False
            if end >= L:
                break
            o += s
    return np.array(keep, dtype=bool)


def rule_c(L, bits, P, w, s, totals, maf, chrom, keep):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    maf = np.ascontiguousarray(maf, dtype=np.float64)
    c32 = None if chrom is None else np.ascontiguousarray(chrom, dtype=np.uint32)
    k8 = np.ascontiguousarray(keep, dtype=np.uint8).copy()
    n = C.c_uint64(0)
    rc = L.fpca_debug_ld_prune_rule(_vp(bits), P, w, s, _vp(totals), _vp(maf), _vp(c32), _vp(k8), C.byref(n))
    return rc, k8, n.value


@pytest.fixture(scope="module", params=["product", "testhooks"])
def L(request, built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    return _lib._load(fp.LIB_PATH if request.param == "product" else fp.HOOKS_LIB_PATH)


def random_case(rng, P, w, density, ties):
    words = (w - 1 + 31) // 32
    # every bit of every word is random: pairs past the window, past the last SNP and across chromosomes must be ignored
    bits = (rng.random((P, words * 32)) < density)
    bits = np.packbits(bits.reshape(P, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(P * words)
    maf = rng.integers(1, 4 if ties else 1000, P) / 2000.0  # few distinct values: equal-MAF ties everywhere
    n = rng.integers(50, 100, P).astype(np.uint64)
    sx = rng.integers(1, 50, P).astype(np.uint64)
    totals = np.stack([n, sx, sx + 2 * rng.integers(0, 20, P).astype(np.uint64)], axis=1)  # sum x^2 >= sum x; n sq - sx^2 > 0 since n > sx
    mono = rng.random(P) < 0.04
    totals[mono, 2] = totals[mono, 1] = totals[mono, 0]  # n n - n n == 0: every call is a 1
    none = rng.random(P) < 0.02
    totals[none] = 0  # no call at all
    return bits, maf, totals, int((mono | none).sum())


CHROMS = {
    "one": lambda P: None,
    "explicit_one": lambda P: np.full(P, 3),
    "runs_of_1": lambda P: np.r_[np.arange(5), np.full(P - 10, 9), np.arange(5)],  # five chromosomes of one SNP at either end
    "short_runs": lambda P: np.repeat(np.arange(P // 6 + 1), 6)[:P],  # every chromosome shorter than most windows
    "mixed": lambda P: np.r_[np.full(100, 1), np.full(1, 2), np.full(120, 1), np.full(3, 4), np.full(P - 224, 5)],  # code 1 twice: two runs
}


@pytest.mark.parametrize("chrom_kind", list(CHROMS))
def test_rule_against_plain_python(L, chrom_kind):
    rng = np.random.default_rng(20261019)
    P = 300
    chrom = CHROMS[chrom_kind](P)
    assert chrom is None or chrom.shape == (P,)
    checked = 0
    for w, s in ((2, 1), (2, 2), (3, 1), (7, 7), (7, 1), (20, 3), (32, 5), (33, 33), (34, 1), (64, 64), (65, 64), (70, 1), (70, 9), (70, 70)):
        for density, ties, precleared in ((0.05, False, False), (0.3, True, True), (0.9, False, True)):
            bits, maf, totals, nmono = random_case(rng, P, w, density, ties)
            keep_in = ((rng.random(P) >= 0.25) if precleared else np.ones(P, dtype=bool)).astype(np.uint8) * 200  # non-zero, not only 1
            ref = rule_python(bits, P, w, s, totals, maf, chrom, keep_in)
            rc, k8, n = rule_c(L, bits, P, w, s, totals, maf, chrom, keep_in)
            assert rc == 0 and set(np.unique(k8)) <= {0, 1}
            assert np.array_equal(k8 != 0, ref), (chrom_kind, w, s, density)
            assert n == int(ref.sum()) and not k8[keep_in == 0].any()
            assert nmono > 0 and 0 < ref.sum() < (keep_in != 0).sum()  # (something goes, something stays)
            checked += 1
    assert checked == 42


def test_rule_ties_order_and_revisits(L):
    """Hand-made cases: an equal-MAF tie drops the later SNP; a strictly rarer i goes instead and its scan ends there; a pair that only a later
    window holds fires there; a pair that shares no window never fires."""
    def run(P, w, s, pairs, maf, keep=None, totals=None):
        words = (w - 1 + 31) // 32
        bits = np.zeros(P * words, dtype=np.uint32)
        for i, j in pairs:
            bits[i * words + ((j - i - 1) >> 5)] |= np.uint32(1 << ((j - i - 1) & 31))
        totals = np.tile(np.array([10, 5, 7], dtype=np.uint64), (P, 1)) if totals is None else totals
        keep = np.ones(P, dtype=np.uint8) if keep is None else keep
        ref = rule_python(bits, P, w, s, totals, maf, None, keep)
        rc, k8, _ = rule_c(L, bits, P, w, s, totals, np.asarray(maf, dtype=np.float64), None, keep)
        assert rc == 0 and np.array_equal(k8 != 0, ref)
        return list(k8)

    assert run(4, 4, 4, [(0, 1)], [0.2, 0.2, 0.2, 0.2]) == [1, 0, 1, 1]  # tie: the later one goes
    assert run(4, 4, 4, [(0, 1)], [0.1, 0.2, 0.2, 0.2]) == [0, 1, 1, 1]  # i strictly rarer: i goes
    assert run(4, 4, 4, [(0, 1), (0, 2)], [0.1, 0.2, 0.2, 0.2]) == [0, 1, 1, 1]  # ... and its scan ends: 2 is not touched
    assert run(4, 4, 4, [(0, 1), (0, 2)], [0.3, 0.2, 0.2, 0.2]) == [1, 0, 0, 1]
    assert run(4, 4, 4, [(0, 1), (1, 2)], [0.3, 0.2, 0.2, 0.2]) == [1, 0, 1, 1]  # 1 is gone before it is an i: 2 survives
    # windows [0, 3) and [2, 5) with step 2: the pair (1, 3) shares no window (1 < (1 // 2) 2 + 3 = 3 is false for j = 3), (2, 4) shares the second
    assert run(5, 3, 2, [(1, 3)], [0.2] * 5) == [1, 1, 1, 1, 1]
    assert run(5, 3, 2, [(2, 4)], [0.2] * 5) == [1, 1, 1, 1, 0]
    assert run(5, 3, 1, [(1, 3)], [0.2] * 5) == [1, 1, 1, 0, 1]  # step 1: window [1, 4) holds it
    # the last window is the one that reaches the end: with window 4, step 3 on 5 SNPs that is [3, 5) -- (0, 4) is never co-windowed
    assert run(5, 4, 3, [(0, 3), (0, 4)], [0.2] * 5) == [1, 1, 1, 0, 1]
    # pre-cleared and monomorphic SNPs hold their positions and are never compared
    tot = np.tile(np.array([10, 5, 7], dtype=np.uint64), (4, 1))
    tot[1] = (10, 10, 10)
    assert run(4, 4, 4, [(0, 1), (1, 2)], [0.2] * 4, totals=tot) == [1, 0, 1, 1]
    assert run(4, 4, 4, [(0, 1), (1, 2), (0, 3)], [0.2] * 4, keep=np.array([1, 0, 1, 1], dtype=np.uint8)) == [1, 0, 1, 0]


def test_rule_refusals(L):
    bits, totals, maf, keep = np.zeros(4, dtype=np.uint32), np.ones((4, 3), dtype=np.uint64), np.zeros(4), np.ones(4, dtype=np.uint8)
    for w, s, msg in ((1, 1, b"window = 1"), (0, 1, b"window = 0"), (5, 0, b"step = 0"), (5, 6, b"step = 6 is larger than window = 5")):
        rc, k8, _ = rule_c(L, bits, 4, w, s, totals, maf, None, keep)
        assert rc == -1 and msg in L.fpca_last_error(), (w, s, L.fpca_last_error())
        assert list(k8) == [1, 1, 1, 1]  # (nothing is written by a refused call)
    assert rule_c(L, bits, 4, 5, 5, totals, maf, None, keep)[0] == 0
    assert L.fpca_debug_ld_prune_rule(None, 4, 5, 5, _vp(totals), _vp(maf), None, _vp(keep), None) == -1


def test_band_kernels_do_not_spill():
    """The pattern of tests/test_snp_subset_cpu.py: the kernels of ld_band.hip compile without spills, scratch or LDS, by the compiler's own
    remarks and by the code object's metadata; the band kernel keeps its six accumulator planes in 256 registers (two waves per SIMD) and
    reads its records as 16-byte vectors."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ld_band.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "ld_band.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    assert len(names) == 3 and sum("k_ld_band" in n for n in names) == 2 and sum("k_ld_totals" in n for n in names) == 1, names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0, 0, 0], key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 6 and all(int(v) == 0 for _, v in remarks), remarks
    occ = sorted(int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr))
    assert occ[:2] == [2, 2], occ
    assert len(re.findall(r"v_mfma_i32_32x32x32_i8", txt)) >= 2 * (6 + 1) * 16 and len(re.findall(r"global_load_dwordx4", txt)) >= 16
    assert "global_atomic_or" in txt
