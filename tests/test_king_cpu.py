"""KING-robust kinship without a GPU: the three entry points in the header, the two hooks in the debug header only, the binding and both
builds of the library; the NULL-context refusals; the cutoff rule through the host-only hook fpca_debug_king_rule against a plain-Python
restatement of include/fpca.h (a loop: the largest current degree goes, the largest index among equals) on random graphs, stars, cliques,
chains and an empty list; and the register discipline of the pair kernel."""
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
    for proto in ("int fpca_king_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *phi /* [ni][nj] */);",
                  "int fpca_king_pairs(fpca_ctx *ctx, const uint8_t *keep /* [N] or NULL */, double thr, uint64_t max_pairs, uint32_t *i, uint32_t *j, double *phi,",
                  "int fpca_king_cutoff(fpca_ctx *ctx, double thr, uint8_t *keep /* [N] in/out, like fpca_snp_qc */, uint64_t *n_kept);"):
        assert re.search("^" + re.escape(proto), main, re.M), proto
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "fpca_debug_king_rule(" in dbg and "fpca_bench_king(" in dbg
    assert "fpca_debug_king_rule" not in main and "fpca_bench_king" not in main  # the hooks are not part of the drop-in boundary
    names = ("fpca_king_block", "fpca_king_pairs", "fpca_king_cutoff", "fpca_debug_king_rule", "fpca_bench_king")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    # NULL context: -1 with a message, before any device work
    buf = np.zeros(4)
    keep = np.ones(4, dtype=np.uint8)
    i32 = np.zeros(4, dtype=np.uint32)
    n = C.c_uint64(0)
    assert L.fpca_king_block(None, 0, 2, 0, 2, _vp(buf)) == -1 and b"fpca_king_block (NULL context)" in L.fpca_last_error()
    assert L.fpca_king_pairs(None, None, 0.1, 4, _vp(i32), _vp(i32), _vp(buf), C.byref(n)) == -1
    assert b"fpca_king_pairs (NULL context)" in L.fpca_last_error()
    assert L.fpca_king_cutoff(None, 0.1, _vp(keep), None) == -1 and b"fpca_king_cutoff (NULL context)" in L.fpca_last_error()
    assert L.fpca_bench_king(None, 1, _vp(buf), None) == -1 and b"fpca_bench_king (NULL context)" in L.fpca_last_error()
    # the Python layer
    for m in ("king_block", "king_pairs", "king_cutoff", "bench_king"):
        assert callable(getattr(fp.Context, m))
    assert list(inspect.signature(fp.Context.king_block).parameters) == ["self", "i0", "ni", "j0", "nj"]
    q = inspect.signature(fp.Context.king_pairs).parameters
    assert list(q) == ["self", "thr", "keep", "max_pairs"] and (q["keep"].default, q["max_pairs"].default) == (None, 1 << 24)
    q = inspect.signature(fp.Context.king_cutoff).parameters
    assert list(q) == ["self", "thr", "keep"] and (q["thr"].default, q["keep"].default) == (0.0884, None)
    q = inspect.signature(fp.king_cutoff).parameters
    assert list(q) == ["prefix", "thr", "snps", "maf", "geno", "ld", "keep", "device"]
    assert (q["thr"].default, q["snps"].default, q["maf"].default, q["geno"].default, q["ld"].default, q["keep"].default) == (0.0884, None, 0.0, 1.0, None, None)
    assert inspect.signature(fp.flashpca).parameters["unrelated"].default is None
    # refused before anything is uploaded
    with pytest.raises(ValueError, match="numeric matrix"):
        fp.flashpca(np.zeros((8, 5)), ndim=1, unrelated=0.0884)
    # the earlier refusals stay
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(os.path.join(ROOT, "tests", "golden", "hapmap3_data"), ndim=2, maf=0.05, keep=np.ones(957, dtype=bool), unrelated=0.0884)
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(os.path.join(ROOT, "tests", "golden", "hapmap3_data"), ndim=2, ld=(10, 5, 0.2), keep=np.ones(957, dtype=bool), unrelated=0.0884)


# ---- the rule --------------------------------------------------------------------------------------------------
def rule_python(pairs, N, keep):
    """include/fpca.h, restated with nothing but loops."""
    keep = [bool(k) for k in keep]
    edges = {(min(a, b), max(a, b)) for a, b in pairs if a != b and keep[a] and keep[b]}
    while edges:
        deg = [0] * N
        for a, b in edges:
            deg[a] += 1
            deg[b] += 1
        best = 0
        for v in range(N):  # the largest degree; among equals the largest index
            if deg[v] >= deg[best]:
                best = v
        keep[best] = False
        edges = {e for e in edges if best not in e}
    return np.array(keep, dtype=bool)


def rule_c(L, pairs, N, keep):
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    i, j = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
    k8 = np.ascontiguousarray(keep, dtype=np.uint8).copy()
    n = C.c_uint64(0)
    rc = L.fpca_debug_king_rule(_vp(i) if len(p) else None, _vp(j) if len(p) else None, len(p), N, _vp(k8), C.byref(n))
    return rc, k8, n.value


@pytest.fixture(scope="module", params=["product", "testhooks"])
def L(request, built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    return _lib._load(fp.LIB_PATH if request.param == "product" else fp.HOOKS_LIB_PATH)


def check_case(L, pairs, N, keep):
    ref = rule_python(pairs, N, keep)
    rc, k8, n = rule_c(L, pairs, N, keep)
    assert rc == 0 and set(np.unique(k8)) <= {0, 1}
    assert np.array_equal(k8 != 0, ref), (N, len(pairs))
    assert n == int(ref.sum()) and not k8[np.asarray(keep) == 0].any()
    # what is left holds no edge
    left = k8 != 0
    assert not any(left[a] and left[b] and a != b for a, b in pairs)
    return ref


def test_rule_against_plain_python_on_random_graphs(L):
    rng = np.random.default_rng(20261019)
    checked = 0
    for N in (50, 51, 120, 257, 400):
        for avg_deg, precleared in ((0.5, False), (2.0, True), (6.0, False), (20.0, True)):
            m = int(N * avg_deg / 2)
            pairs = rng.integers(0, N, (m, 2))  # either order, repeats and a few i == j among them
            pairs = [(int(a), int(b)) for a, b in pairs]
            keep = ((rng.random(N) >= 0.2) if precleared else np.ones(N, dtype=bool)).astype(np.uint8) * 200  # non-zero, not only 1
            ref = check_case(L, pairs, N, keep)
            assert 0 < ref.sum() < (keep != 0).sum()  # (something goes, something stays)
            checked += 1
    assert checked == 20


def test_rule_stars_cliques_chains_and_the_empty_list(L):
    one = lambda N: np.ones(N, dtype=np.uint8)  # noqa: E731
    # empty list: nothing goes; a 0 stays 0
    rc, k8, n = rule_c(L, [], 60, one(60))
    assert rc == 0 and k8.all() and n == 60
    k = one(60)
    k[[3, 59]] = 0
    rc, k8, n = rule_c(L, [], 60, k)
    assert rc == 0 and n == 58 and not k8[3] and not k8[59]
    # a star: the centre goes, every leaf stays -- wherever the centre's index lies
    for centre in (0, 25, 69):
        star = [(centre, v) for v in range(70) if v != centre]
        ref = check_case(L, star, 70, one(70))
        assert not ref[centre] and ref.sum() == 69
    # two stars sharing nothing, plus a star whose centre was cleared on entry: its leaves have no edge left
    k = one(100)
    k[50] = 0
    ref = check_case(L, [(0, v) for v in range(1, 20)] + [(30, v) for v in range(31, 45)] + [(50, v) for v in range(51, 70)], 100, k)
    assert not ref[0] and not ref[30] and ref.sum() == 97
    # a clique of 12 inside 50 samples: all degrees equal, the largest index goes each time, sample 5 is left
    clique = [(a, b) for a in range(5, 17) for b in range(a + 1, 17)]
    ref = check_case(L, clique, 50, one(50))
    assert ref.sum() == 50 - 11 and ref[5] and not ref[6:17].any()
    # a chain 0 - 1 - ... - 9: the inner nodes tie at degree 2, the largest index (8) goes first, then 6, 4, 2 -- and 0 - 1 is left: 1 goes
    chain = [(v, v + 1) for v in range(9)]
    ref = check_case(L, chain, 50, one(50))
    assert list(np.flatnonzero(~ref)) == [1, 2, 4, 6, 8]
    # a long chain and a chain listed backwards with repeats
    check_case(L, [(v, v + 1) for v in range(399)], 400, one(400))
    check_case(L, [(v + 1, v) for v in range(99)] * 2, 100, one(100))
    # a tie between a degree reached by decrements and an untouched one: 0-1, 0-2, 3-4, 3-5, 2-3 -> 3 (degree 3) goes, then 0 (2) -> kept 1, 2, 4, 5
    ref = check_case(L, [(0, 1), (0, 2), (3, 4), (3, 5), (2, 3)], 50, one(50))
    assert list(np.flatnonzero(~ref)) == [0, 3]


def test_rule_refusals(L):
    keep = np.ones(4, dtype=np.uint8)
    rc, k8, _ = rule_c(L, [(0, 4)], 4, keep)
    assert rc == -1 and b"outside the 4 samples" in L.fpca_last_error() and list(k8) == [1, 1, 1, 1]
    i32 = np.zeros(1, dtype=np.uint32)
    assert L.fpca_debug_king_rule(_vp(i32), _vp(i32), 1, 4, None, None) == -1
    assert L.fpca_debug_king_rule(None, _vp(i32), 1, 4, _vp(keep), None) == -1


def test_king_kernels_do_not_spill():
    """The pattern of tests/test_ld_prune_cpu.py: king.hip holds the two instances of k_king, which compile without spills, scratch or LDS, by
    the compiler's own remarks and by the code object's metadata; five accumulator planes leave room for two waves per SIMD (the occupancy
    the remarks state is printed and held to that); the records are read as 16-byte vectors and the list is appended with a vector-memory
    atomic add.  Recorded: occupancy 3 waves/SIMD, 136 VGPRs, 0 AGPRs for both instances."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "king.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "king.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    assert len(names) == 2 and all("k_king" in n for n in names), names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0, 0], key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 4 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0, 0]
    assert [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)] == [0, 0]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    print("k_king: occupancy %s waves/SIMD, VGPRs %s, AGPRs %s" % (occ, vgprs, agprs))
    assert len(occ) == 2 and all(o >= 2 for o in occ), occ
    assert len(re.findall(r"v_mfma_i32_32x32x32_i8", txt)) >= 2 * (5 + 1) * 16 and len(re.findall(r"global_load_dwordx4", txt)) >= 16
    assert "global_atomic_add_x2" in txt
