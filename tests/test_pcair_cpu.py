"""PC-AiR's partition without a GPU: the four entry points in the header, the hook in the debug header only, the binding and both builds of
the library; the NULL-context refusals; the Python signatures; the partition rule through the host-only fpca_pcair_partition against a
plain-Python restatement of include/fpca.h (tests/pcair_yardstick.py: a loop that also records which tie-break decided each removal) on
random graphs of 5 - 300 samples, stars, cliques, chains and an empty list, with repeated and reversed pairs and a pre-cleared keep; the
agreement with fpca_debug_king_rule where n_div and kin cannot decide; and the register discipline of the census kernel.
kin values are multiples of 2^-10 below 1: a sum of at most 300 of them is exact in fp64 in any order."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from pcair_yardstick import DEGREE, INDEX, KINSUM, NDIV, partition_python

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 2 ** -5.5


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    for proto in ("int fpca_king_census(fpca_ctx *ctx, const uint8_t *keep /* [N] or NULL */, double kin_thr, double div_thr,",
                  "int fpca_pcair_partition(uint64_t N, uint64_t n_pairs, const uint32_t *i, const uint32_t *j, const double *kin,",
                  "int fpca_pcair_king(fpca_ctx *ctx, double kin_thr, double div_thr, uint8_t *keep /* [N] in/out */, uint64_t *n_kept,",
                  "int fpca_pcair_pairs(fpca_ctx *ctx, double div_thr, uint64_t n_pairs, const uint32_t *i, const uint32_t *j, const double *kin,"):
        assert re.search("^" + re.escape(proto), main, re.M), proto
    assert "PARITY WITH GENESIS IS NOT CLAIMED" in main
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "int fpca_bench_king_census(fpca_ctx *ctx, int reps, double *ms);" in dbg
    assert "fpca_bench_king_census" not in main  # the hook is not part of the drop-in boundary
    names = ("fpca_king_census", "fpca_pcair_partition", "fpca_pcair_king", "fpca_pcair_pairs", "fpca_bench_king_census")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    # NULL context: -1 with a message that names the function, before any device work
    buf = np.zeros(4)
    keep = np.ones(4, dtype=np.uint8)
    u32 = np.zeros(4, dtype=np.uint32)
    n = C.c_uint64(0)
    assert L.fpca_king_census(None, None, THR, -THR, None, None, 0, _vp(u32), _vp(u32)) == -1
    assert b"fpca_king_census (NULL context)" in L.fpca_last_error()
    assert L.fpca_pcair_king(None, THR, -THR, _vp(keep), C.byref(n), None, None) == -1
    assert b"fpca_pcair_king (NULL context)" in L.fpca_last_error()
    assert L.fpca_pcair_pairs(None, -THR, 0, None, None, None, _vp(keep), C.byref(n), None) == -1
    assert b"fpca_pcair_pairs (NULL context)" in L.fpca_last_error()
    assert L.fpca_bench_king_census(None, 1, _vp(buf)) == -1 and b"fpca_bench_king_census (NULL context)" in L.fpca_last_error()
    assert list(keep) == [1, 1, 1, 1]


def test_python_signatures_and_early_refusals(built_lib):
    import flashpca_amd as fp

    def params(f):
        return [(k, v.default) for k, v in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert params(fp.Context.king_census) == [("self", E), ("kin_thr", THR), ("div_thr", -THR), ("keep", None), ("exclude", None)]
    assert params(fp.Context.pcair_partition) == [("self", E), ("kin_thr", THR), ("div_thr", -THR), ("keep", None), ("kin_pairs", None), ("counts", False)]
    assert params(fp.Context.bench_king_census) == [("self", E), ("reps", 5)]
    assert params(fp.pcair_partition_rule) == [("N", E), ("i", E), ("j", E), ("kin", E), ("n_div", E), ("keep", None)]
    assert params(fp.pcair_partition) == [("prefix", E), ("kin_thr", THR), ("div_thr", -THR), ("snps", None), ("maf", 0.0), ("geno", 1.0), ("ld", None),
                                          ("keep", None), ("kin_pairs", None), ("device", 0)]
    assert params(fp.pcair) == [("prefix", E), ("ndim", 10), ("kin_thr", THR), ("div_thr", -THR), ("iterations", 1), ("relate_pcs", None), ("eps", 0.01),
                                ("snps", None), ("maf", 0.0), ("geno", 1.0), ("ld", None), ("keep", None), ("device", 0), ("flashpca_kw", E)]
    assert inspect.signature(fp.pcair).parameters["flashpca_kw"].kind is inspect.Parameter.VAR_KEYWORD
    # flashpca()'s signature is not touched (tests/test_king_rel_cpu.py holds its tail)
    assert "pcair" not in " ".join(inspect.signature(fp.flashpca).parameters)
    # refused before anything is uploaded: no device is asked for
    hm3 = os.path.join(ROOT, "tests", "golden", "hapmap3_data")
    for it in (3, 0, "2"):
        with pytest.raises(ValueError, match="iterations"):
            fp.pcair(hm3, ndim=2, iterations=it)
    with pytest.raises(ValueError, match="numeric matrix"):
        fp.pcair(np.zeros((8, 5)), ndim=1)
    with pytest.raises(ValueError, match="not passed on"):
        fp.pcair(hm3, ndim=2, unrelated=0.0884)


# ---- the rule --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["product", "testhooks"])
def L(request, built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    return _lib._load(fp.LIB_PATH if request.param == "product" else fp.HOOKS_LIB_PATH)


def rule_c(L, N, i, j, kin, n_div, keep):
    i, j = np.ascontiguousarray(i, dtype=np.uint32), np.ascontiguousarray(j, dtype=np.uint32)
    kin = np.ascontiguousarray(kin, dtype=np.float64)
    n_div = np.ascontiguousarray(n_div, dtype=np.uint32)
    k8 = np.ascontiguousarray(keep, dtype=np.uint8).copy()
    n = C.c_uint64(0)
    m = i.size
    rc = L.fpca_pcair_partition(N, m, _vp(i) if m else None, _vp(j) if m else None, _vp(kin) if m else None, _vp(n_div), _vp(k8), C.byref(n))
    return rc, k8, n.value


def check_case(L, N, pairs, kin, n_div, keep, decided=None, tied=None):
    i = [a for a, _ in pairs]
    j = [b for _, b in pairs]
    ref = partition_python(N, i, j, kin, n_div, keep, decided, tied)
    rc, k8, n = rule_c(L, N, i, j, kin, n_div, keep)
    assert rc == 0, L.fpca_last_error()
    assert set(np.unique(k8)) <= {0, 1}
    assert np.array_equal(k8 != 0, ref), (N, len(pairs), np.flatnonzero((k8 != 0) != ref)[:8])
    assert n == int(ref.sum()) and not k8[np.asarray(keep) == 0].any()
    left = k8 != 0
    assert not any(left[a] and left[b] for a, b in pairs)  # what is left holds no edge
    return ref


def random_graph(rng, N, avg_deg, kin_levels, div_levels):
    """Pairs in either order with repeats (no i == j: that is refused), kin from `kin_levels` multiples of 2^-10, n_div below div_levels."""
    m = max(int(N * avg_deg / 2), 1)
    a = rng.integers(0, N, m)
    b = (a + 1 + rng.integers(0, N - 1, m)) % N
    pairs = [(int(x), int(y)) for x, y in zip(a, b)]
    pairs += [(y, x) for x, y in pairs[: m // 5]]  # a fifth of them again, reversed (with another kin: the first one listed counts)
    kin = rng.integers(1, kin_levels + 1, len(pairs)) / 1024.0
    return pairs, kin, rng.integers(0, div_levels, N).astype(np.uint32)


def test_rule_against_plain_python_on_random_graphs(L):
    rng = np.random.default_rng(20261021)
    decided, tied = {}, {}
    checked = 0
    for N in (5, 17, 50, 120, 257, 300):
        for avg_deg, precleared in ((0.7, False), (2.0, True), (6.0, False), (20.0, True)):
            for kin_levels, div_levels in ((1, 1), (2, 2), (400, 3), (3, 1000)):
                pairs, kin, n_div = random_graph(rng, N, min(avg_deg, N / 2), kin_levels, div_levels)
                keep = ((rng.random(N) >= 0.2) if precleared else np.ones(N, dtype=bool)).astype(np.uint8) * 200  # non-zero, not only 1
                ref = check_case(L, N, pairs, kin, n_div, keep, decided, tied)
                assert ref.sum() <= (keep != 0).sum()
                checked += 1
    print("%d graphs; removals decided by %s; ties left after %s" % (checked, decided, tied))
    assert checked == 96
    # every level decided removals, and every level's tie occurred (so the next level was consulted)
    assert all(decided.get(k, 0) > 0 for k in (DEGREE, NDIV, KINSUM, INDEX)), decided
    assert all(tied.get(k, 0) > 0 for k in (DEGREE, NDIV, KINSUM)), tied


def test_rule_stars_cliques_chains_and_the_empty_list(L):
    one = lambda N: np.ones(N, dtype=np.uint8)  # noqa: E731
    zero = lambda N: np.zeros(N, dtype=np.uint32)  # noqa: E731
    q = 0.25
    # empty list: nothing goes; a 0 stays 0
    rc, k8, n = rule_c(L, 60, [], [], [], zero(60), one(60))
    assert rc == 0 and k8.all() and n == 60
    k = one(60)
    k[[3, 59]] = 0
    rc, k8, n = rule_c(L, 60, [], [], [], zero(60), k)
    assert rc == 0 and n == 58 and not k8[3] and not k8[59]
    # a star: the centre goes whatever its n_div, every leaf stays
    for centre in (0, 25, 69):
        star = [(centre, v) for v in range(70) if v != centre]
        nd = zero(70)
        nd[centre] = 50
        ref = check_case(L, 70, star, [q] * 69, nd, one(70))
        assert not ref[centre] and ref.sum() == 69
    # a star whose centre was cleared on entry: its leaves have no edge left
    k = one(100)
    k[50] = 0
    ref = check_case(L, 100, [(0, v) for v in range(1, 20)] + [(50, v) for v in range(51, 70)], [q] * 38, zero(100), k)
    assert not ref[0] and ref.sum() == 98
    # a clique of 12 inside 50 samples, all else equal: the largest index goes each time, sample 5 is left
    clique = [(a, b) for a in range(5, 17) for b in range(a + 1, 17)]
    ref = check_case(L, 50, clique, [q] * len(clique), zero(50), one(50))
    assert ref.sum() == 50 - 11 and ref[5] and not ref[6:17].any()
    # the same clique, sample 16 with the most divergent partners: it is the one that stays
    nd = zero(50)
    nd[5:17] = 3
    nd[16] = 9
    ref = check_case(L, 50, clique, [q] * len(clique), nd, one(50))
    assert ref.sum() == 50 - 11 and ref[16] and not ref[5:16].any()
    # the same clique, equal n_div, the edges of sample 10 carrying more kin: the sums decide until two samples are left
    kin = [0.375 if 10 in e else q for e in clique]
    ref = check_case(L, 50, clique, kin, zero(50), one(50))
    assert ref.sum() == 50 - 11
    # the chain 0 - 1 - 2 - 3 with the weakest link at 0 - 1: 1 and 2 tie at degree 2, the sum of 1 is smaller, it goes (the index would
    # have said 2); then 3 goes by its index
    ref = check_case(L, 4, [(0, 1), (1, 2), (2, 3)], [0.125, 0.25, 0.5], zero(4), one(4))
    assert list(ref) == [True, False, True, False]
    # a chain 0 - 1 - ... - 9, all else equal: 8 goes first, then 6, 4, 2 -- and 0 - 1 is left: 1 goes
    chain = [(v, v + 1) for v in range(9)]
    ref = check_case(L, 50, chain, [q] * 9, zero(50), one(50))
    assert list(np.flatnonzero(~ref)) == [1, 2, 4, 6, 8]
    # a long chain, and a chain listed backwards with repeats that carry another kin (the first listed counts)
    check_case(L, 400, [(v, v + 1) for v in range(399)], [q] * 399, zero(400), one(400))
    back = [(v + 1, v) for v in range(99)]
    check_case(L, 100, back * 2, [(1 + v % 3) / 1024.0 for v in range(99)] + [0.5] * 99, zero(100), one(100))
    # two samples, one pair listed twice with kin in the other order of size: nothing but the index can decide either way
    ref = check_case(L, 2, [(0, 1), (1, 0)], [0.125, 0.5], zero(2), one(2))
    assert list(ref) == [True, False]


def test_rule_falls_through_to_king_cutoffs_rule(L):
    """n_div all zero and one common kin: equal degrees give equal sums (an exact multiple of the kin), so nothing but the index is left
    and the mask is fpca_debug_king_rule's on the same pairs."""
    rng = np.random.default_rng(5)
    for N, avg_deg in ((40, 1.0), (150, 3.0), (300, 8.0), (300, 30.0)):
        pairs, _, _ = random_graph(rng, N, avg_deg, 1, 1)
        i = np.array([a for a, _ in pairs], dtype=np.uint32)
        j = np.array([b for _, b in pairs], dtype=np.uint32)
        keep = (rng.random(N) >= 0.1).astype(np.uint8)
        rc, k8, n = rule_c(L, N, i, j, np.full(i.size, 0.0625), np.zeros(N, dtype=np.uint32), keep)
        old = keep.copy()
        m = C.c_uint64(0)
        assert L.fpca_debug_king_rule(_vp(i), _vp(j), i.size, N, _vp(old), C.byref(m)) == 0
        assert rc == 0 and np.array_equal(k8, old) and n == m.value and 0 < n < keep.sum()


def test_rule_refusals(L):
    nd = np.zeros(4, dtype=np.uint32)
    keep = np.array([1, 7, 1, 1], dtype=np.uint8)
    rc, k8, _ = rule_c(L, 4, [0], [4], [0.25], nd, keep)
    assert rc == -1 and b"fpca_pcair_partition: pair 0 names sample 4 of 4" in L.fpca_last_error() and list(k8) == [1, 7, 1, 1]
    rc, k8, _ = rule_c(L, 4, [0, 2], [1, 2], [0.25, 0.25], nd, keep)
    assert rc == -1 and b"fpca_pcair_partition: pair 1 pairs sample 2 with itself" in L.fpca_last_error() and list(k8) == [1, 7, 1, 1]
    rc, k8, _ = rule_c(L, 4, [0], [1], [float("nan")], nd, keep)
    assert rc == -1 and b"not finite" in L.fpca_last_error()
    u32 = np.zeros(1, dtype=np.uint32)
    one = np.ones(1)
    assert L.fpca_pcair_partition(4, 1, _vp(u32), _vp(u32), _vp(one), _vp(nd), None, None) == -1
    assert L.fpca_pcair_partition(4, 1, None, _vp(u32), _vp(one), _vp(nd), _vp(keep), None) == -1
    assert L.fpca_pcair_partition(4, 1, _vp(u32), _vp(u32), None, _vp(nd), _vp(keep), None) == -1
    assert L.fpca_pcair_partition(4, 0, None, None, None, None, _vp(keep), None) == -1
    assert L.fpca_pcair_partition(1 << 32, 0, None, None, None, _vp(nd), _vp(keep), None) == -1


def test_python_rule_wrapper(built_lib):
    import flashpca_amd as fp

    got = fp.pcair_partition_rule(6, [0, 1, 2], [1, 2, 3], [0.25, 0.25, 0.25], np.zeros(6, dtype=np.uint32))
    assert got.dtype == np.bool_ and list(got) == [True, False, False, True, True, True]
    got = fp.pcair_partition_rule(6, [0, 1, 2], [1, 2, 3], [0.25, 0.25, 0.25], [0, 0, 5, 0, 0, 0], keep=[1, 1, 1, 1, 0, 1])
    # the chain 0 - 1 - 2 - 3: 1 and 2 tie at degree 2 and 1 has fewer divergent partners, it goes; of 2 - 3, 3 has fewer; 4 was cleared
    assert list(got) == [True, False, True, False, False, True]
    with pytest.raises(ValueError, match="n_div"):
        fp.pcair_partition_rule(6, [0], [1], [0.25], np.zeros(5, dtype=np.uint32))
    with pytest.raises(ValueError, match="kin has one entry per pair"):
        fp.pcair_partition_rule(6, [0], [1], [0.25, 0.5], np.zeros(6, dtype=np.uint32))
    with pytest.raises(fp.FpcaError, match="names sample 6 of 6"):
        fp.pcair_partition_rule(6, [0], [6], [0.25], np.zeros(6, dtype=np.uint32))


def test_census_kernel_does_not_spill():
    """The pattern of test_king_kernels_do_not_spill (tests/test_king_cpu.py): pcair.hip holds one kernel, k_king_census, which compiles
    without spills, scratch or LDS, by the compiler's own remarks and by the code object's metadata, at two waves per SIMD or more; it
    issues k_king's products (five planes and the x.x-only loop), reads the records as 16-byte vectors, appends to the list with a 64-bit
    vector-memory atomic add and counts with 32-bit ones that return nothing.  Recorded: occupancy 3 waves/SIMD, 136 VGPRs, 0 AGPRs."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pcair.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "pcair.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    assert len(names) == 1 and "k_king_census" in names[0], names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0], key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 2 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0]
    assert [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)] == [0]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    print("k_king_census: occupancy %s waves/SIMD, VGPRs %s, AGPRs %s" % (occ, vgprs, agprs))
    assert len(occ) == 1 and occ[0] >= 2, occ
    assert len(re.findall(r"v_mfma_i32_32x32x32_i8", txt)) >= (5 + 1) * 16 and len(re.findall(r"global_load_dwordx4", txt)) >= 16
    assert "global_atomic_add_x2" in txt and len(re.findall(r"global_atomic_add v\[", txt)) >= 4
    assert "__launch_bounds__(256, 2) void k_king_census" in open(os.path.join(csrc, "pcair.hip")).read()
