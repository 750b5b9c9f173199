"""The KING relationship table without a GPU: the four entry points in the header, the bench hook in the debug header only, the binding and
both builds of the library; the NULL-context refusals; the Python signatures; fpca_king_classify (host only) against a plain-Python
restatement of include/fpca.h on random arrays and on hand-made boundaries; the register discipline of the pair kernel; write_kin0 byte for
byte."""
import ctypes as C
import inspect
import math
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
    for proto in (r"int fpca_king_counts_block\(fpca_ctx \*ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, uint32_t \*counts",
                  r"int fpca_king_related\(fpca_ctx \*ctx, const uint8_t \*keep[^,]*, double thr, uint32_t min_shared, uint64_t max_pairs, uint32_t \*i,",
                  r"int fpca_king_cutoff_shared\(fpca_ctx \*ctx, double thr, uint32_t min_shared, uint8_t \*keep[^,]*, uint64_t \*n_kept\);",
                  r"int fpca_king_classify\(uint64_t n_pairs, const double \*phi, const uint32_t \*counts[^,]*, double po_ibs0, uint8_t \*type"):
        assert re.search("^" + proto, main, re.M), proto
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "fpca_bench_king_rel(" in dbg and "fpca_bench_king_rel" not in main  # the hook is not part of the drop-in boundary
    names = ("fpca_king_counts_block", "fpca_king_related", "fpca_king_cutoff_shared", "fpca_king_classify", "fpca_bench_king_rel")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    # NULL context: -1 with a message that names the entry point, before any device work
    buf = np.zeros(4)
    keep = np.ones(4, dtype=np.uint8)
    i32 = np.zeros(4, dtype=np.uint32)
    c32 = np.zeros((4, 6), dtype=np.uint32)
    n = C.c_uint64(0)
    assert L.fpca_king_counts_block(None, 0, 2, 0, 2, _vp(c32), _vp(buf)) == -1 and b"fpca_king_counts_block (NULL context)" in L.fpca_last_error()
    assert L.fpca_king_related(None, None, 0.1, 0, 4, _vp(i32), _vp(i32), _vp(buf), _vp(c32), C.byref(n)) == -1
    assert b"fpca_king_related (NULL context)" in L.fpca_last_error()
    assert L.fpca_king_cutoff_shared(None, 0.1, 0, _vp(keep), None) == -1 and b"fpca_king_cutoff_shared (NULL context)" in L.fpca_last_error()
    assert L.fpca_bench_king_rel(None, 1, _vp(buf), None) == -1 and b"fpca_bench_king_rel (NULL context)" in L.fpca_last_error()


def test_python_signatures():
    import flashpca_amd as fp

    assert list(inspect.signature(fp.Context.king_counts_block).parameters) == ["self", "i0", "ni", "j0", "nj"]
    q = inspect.signature(fp.Context.king_related).parameters
    assert list(q) == ["self", "thr", "keep", "min_shared", "max_pairs", "po_ibs0"]
    assert [q[k].default for k in list(q)[1:]] == [0.0442, None, 0, 1 << 24, 0.005]
    q = inspect.signature(fp.Context.king_cutoff_shared).parameters
    assert list(q) == ["self", "thr", "min_shared", "keep"] and [q[k].default for k in list(q)[1:]] == [0.0884, 0, None]
    q = inspect.signature(fp.Context.bench_king_rel).parameters
    assert list(q) == ["self", "reps"] and q["reps"].default == 5
    q = inspect.signature(fp.king_related).parameters
    assert list(q) == ["prefix", "thr", "min_shared", "po_ibs0", "snps", "maf", "geno", "ld", "keep", "device"]
    assert [q[k].default for k in list(q)[1:]] == [0.0442, 0, 0.005, None, 0.0, 1.0, None, None, 0]
    assert list(inspect.signature(fp.write_kin0).parameters) == ["path", "prefix", "table"]
    q = inspect.signature(fp.flashpca).parameters
    assert q["unrelated_min_shared"].default == 0 and list(q)[-2:] == ["unrelated_min_shared", "solver_kw"]
    # the existing signatures stay (tests/test_king_cpu.py holds them in full)
    assert list(inspect.signature(fp.Context.king_pairs).parameters) == ["self", "thr", "keep", "max_pairs"]
    assert list(inspect.signature(fp.Context.king_cutoff).parameters) == ["self", "thr", "keep"]


# ---- fpca_king_classify --------------------------------------------------------------------------------------
def classify_python(phi, counts, po_ibs0):
    """include/fpca.h, restated with nothing but comparisons."""
    out = []
    for v, c in zip(phi, counts):
        shared, ibs0 = int(c[0]), int(c[1])
        if math.isnan(v) or shared == 0:
            out.append(255)
        elif v > 0.354:
            out.append(5)
        elif v > 0.177:
            out.append(1 if ibs0 / shared < po_ibs0 else 2)
        elif v > 0.0884:
            out.append(3)
        elif v > 0.0442:
            out.append(4)
        else:
            out.append(0)
    return np.array(out, dtype=np.uint8)


@pytest.fixture(scope="module", params=["product", "testhooks"])
def L(request, built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    return _lib._load(fp.LIB_PATH if request.param == "product" else fp.HOOKS_LIB_PATH)


def classify_c(L, phi, counts, po_ibs0):
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 6)
    out = np.full(phi.size, 77, dtype=np.uint8)
    rc = L.fpca_king_classify(phi.size, _vp(phi), _vp(counts), po_ibs0, _vp(out))
    return rc, out


def test_classify_against_plain_python_on_random_arrays(L):
    rng = np.random.default_rng(20261020)
    n = 4000
    phi = rng.uniform(-0.3, 0.55, n)
    phi[rng.random(n) < 0.05] = np.nan
    phi[:8] = [0.354, 0.177, 0.0884, 0.0442, 0.5, 0.25, 0.0, -1.0]
    counts = rng.integers(0, 2 ** 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    counts[:, 0] = rng.integers(0, 3000, n)
    counts[:, 1] = rng.integers(0, 40, n)
    counts[rng.random(n) < 0.03, 0] = 0
    for po in (0.005, 0.0, 0.01, 1.5):
        rc, got = classify_c(L, phi, counts, po)
        want = classify_python(phi, counts, po)
        assert rc == 0 and np.array_equal(got, want), po
        hist = {t: int((got == t).sum()) for t in (0, 1, 2, 3, 4, 5, 255)}
        print("po_ibs0 %g: types %s" % (po, hist))
        assert all(hist[t] > 0 for t in (0, 2, 3, 4, 5, 255)) and (hist[1] > 0) == (po > 0)  # (no fraction is below 0)


def test_classify_boundaries(L):
    c = lambda shared, ibs0: [shared, ibs0, 9, 9, 9, 9]  # noqa: E731
    up = lambda v: np.nextafter(v, 1.0)  # noqa: E731
    cases = [
        # every cut point belongs to the lower side: the comparisons on phi are strict
        (0.354, c(1000, 0), 1), (up(0.354), c(1000, 0), 5), (0.354, c(1000, 50), 2),
        (0.177, c(1000, 0), 3), (up(0.177), c(1000, 0), 1), (up(0.177), c(1000, 50), 2),
        (0.0884, c(1000, 0), 4), (up(0.0884), c(1000, 0), 3),
        (0.0442, c(1000, 0), 0), (up(0.0442), c(1000, 0), 4),
        (0.5, c(1000, 0), 5), (0.0, c(1000, 0), 0), (-0.7, c(1000, 500), 0),
        # no value
        (float("nan"), c(1000, 0), 255), (0.25, c(0, 0), 255), (0.5, c(0, 0), 255), (float("nan"), c(0, 0), 255),
        # ibs0 / shared exactly equal to po_ibs0 = 0.005 is NOT parent-offspring; one SNP fewer is
        (0.25, c(1000, 5), 2), (0.25, c(1000, 4), 1), (0.25, c(200, 1), 2), (0.25, c(201, 1), 1), (0.25, c(2 ** 32 - 1, 0), 1),
    ]
    phi = [v for v, _, _ in cases]
    counts = [k for _, k, _ in cases]
    want = np.array([t for _, _, t in cases], dtype=np.uint8)
    assert 5.0 / 1000.0 == 0.005 and 1.0 / 200.0 == 0.005
    rc, got = classify_c(L, phi, counts, 0.005)
    assert rc == 0 and np.array_equal(got, want), (got, want)
    assert np.array_equal(classify_python(phi, counts, 0.005), want)
    # po_ibs0 = 0: nobody is parent-offspring
    rc, got = classify_c(L, [0.25, 0.25], [c(1000, 0), c(1000, 3)], 0.0)
    assert rc == 0 and list(got) == [2, 2]
    # an empty list is served, NULL arrays and all
    assert L.fpca_king_classify(0, None, None, 0.005, None) == 0


def test_classify_refusals(L):
    for bad in (float("nan"), -1e-9, -1.0, float("inf"), float("-inf")):
        rc, got = classify_c(L, [0.25], [[1000, 0, 0, 0, 0, 0]], bad)
        assert rc == -1 and b"fpca_king_classify: po_ibs0" in L.fpca_last_error() and got[0] == 77, bad
    one = np.zeros(1)
    c6 = np.zeros(6, dtype=np.uint32)
    t = np.zeros(1, dtype=np.uint8)
    assert L.fpca_king_classify(1, None, _vp(c6), 0.005, _vp(t)) == -1
    assert L.fpca_king_classify(1, _vp(one), None, 0.005, _vp(t)) == -1
    assert L.fpca_king_classify(1, _vp(one), _vp(c6), 0.005, None) == -1
    import flashpca_amd as fp

    with pytest.raises(ValueError):
        fp.king_classify([0.1, 0.2], np.zeros((3, 6), dtype=np.uint32))
    with pytest.raises(fp.FpcaError):
        fp.king_classify([0.1], np.zeros((1, 6), dtype=np.uint32), po_ibs0=float("nan"))


# ---- the kernel ------------------------------------------------------------------------------------------------
def test_king_rel_kernels_do_not_spill():
    """The pattern of test_king_kernels_do_not_spill: king_rel.hip holds the two instances of k_king_rel, which compile without spills,
    scratch or LDS, by the compiler's own remarks and by the code object's metadata; seven accumulator planes (112 registers) and the
    operand buffers leave room for two waves per SIMD (the occupancy the remarks state is printed and held to that); both paths of both
    instances are there -- 2 x (7 + 2) x 16 matrix instructions --, the records are read as 16-byte vectors and the list is appended with a
    vector-memory atomic add.  Recorded: occupancy 2 waves/SIMD, 171 (BLOCK) and 182 (PAIRS) VGPRs, 0 AGPRs."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "king_rel.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "king_rel.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    assert len(names) == 2 and all("k_king_rel" in n for n in names), names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0, 0], key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 4 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0, 0]
    assert [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)] == [0, 0]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    print("k_king_rel: occupancy %s waves/SIMD, VGPRs %s, AGPRs %s" % (occ, vgprs, agprs))
    assert len(occ) == 2 and all(o >= 2 for o in occ), occ
    assert len(re.findall(r"v_mfma_i32_32x32x32_i8", txt)) >= 2 * (7 + 2) * 16
    assert "global_load_dwordx4" in txt and "global_atomic_add_x2" in txt
    # the inner loop is this file's own: the shared header and its two users are not what carries the seventh plane
    src = open(os.path.join(csrc, "king_rel.hip")).read()
    assert "0x00010000u" in src and "rel_products" in src
    for other in ("ld_planes.hpp", "ld_band.hip", "king.hip"):
        assert "0x00010000u" not in open(os.path.join(csrc, other)).read(), other


# ---- .kin0 -----------------------------------------------------------------------------------------------------
def test_write_kin0_byte_for_byte(tmp_path):
    import flashpca_amd as fp

    prefix = str(tmp_path / "three")
    with open(prefix + ".fam", "w") as f:
        f.write("F1 A 0 0 1 -9\nF1 B 0 0 2 -9\nF2\tC\tA\tB\t1\t-9\n")
    table = dict(i=np.array([0, 0, 1], dtype=np.uint32), j=np.array([1, 2, 2], dtype=np.uint32), phi=np.array([0.25, -0.125, 0.1]),
                 shared=np.array([1000, 800, 3], dtype=np.uint32), ibs0=np.array([0, 100, 1], dtype=np.uint32),
                 hethet=np.array([250, 200, 1], dtype=np.uint32))
    out = str(tmp_path / "out.kin0")
    fp.write_kin0(out, prefix, table)
    want = ("FID1\tID1\tFID2\tID2\tN_SNP\tHetHet\tIBS0\tKinship\n"
            "F1\tA\tF1\tB\t1000\t0.25\t0\t0.25\n"
            "F1\tA\tF2\tC\t800\t0.25\t0.125\t-0.125\n"
            "F1\tB\tF2\tC\t3\t0.33333333333333331\t0.33333333333333331\t0.10000000000000001\n")
    assert open(out, "rb").read() == want.encode()
    # every real reads back to the double it was
    rows = [l.split("\t") for l in open(out).read().splitlines()[1:]]
    assert [float(r[7]) for r in rows] == [0.25, -0.125, 0.1] and float(rows[2][5]) == 1.0 / 3.0
    # an empty table is a header alone; a pair outside the .fam is refused
    fp.write_kin0(out, prefix, {k: v[:0] for k, v in table.items()})
    assert open(out).read() == "FID1\tID1\tFID2\tID2\tN_SNP\tHetHet\tIBS0\tKinship\n"
    with pytest.raises(ValueError, match="has 3 rows"):
        fp.write_kin0(out, prefix, dict(table, j=np.array([1, 3, 2], dtype=np.uint32)))
