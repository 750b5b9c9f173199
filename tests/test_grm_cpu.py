"""The relationship matrix without a GPU: the four entry points in the header with their definitions, the bench hook in the debug header
only, the binding and both builds of the library; the NULL-context refusals; the Python signatures; write_grm / read_grm byte for byte on a
hand-made 5-sample triangle; the packed-triangle index; the register discipline of grm.hip."""
import ctypes as C
import inspect
import os
import re
import struct
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
    for proto in (r"int fpca_grm_block\(fpca_ctx \*ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, int divisor, double \*grm /\*[^*]*\*/,\s*uint32_t \*shared /\*[^*]*\*/\);",
                  r"int fpca_grm_tri\(fpca_ctx \*ctx, int divisor, double \*grm /\*[^*]*\*/, uint32_t \*shared /\*[^*]*\*/\);",
                  r"int fpca_grm_pairs\(fpca_ctx \*ctx, const uint8_t \*keep[^,]*, double thr, int divisor, uint64_t max_pairs, uint32_t \*i, uint32_t \*j,\s*"
                  r"double \*g, uint32_t \*shared[^,]*, uint64_t \*n_pairs\);",
                  r"int fpca_grm_cutoff\(fpca_ctx \*ctx, double thr, int divisor, uint8_t \*keep[^,]*, uint64_t \*n_kept\);"):
        assert re.search("^" + proto, main, re.M), proto
    for name, val in (("FPCA_GRM_DIV_SHARED", 0), ("FPCA_GRM_DIV_P", 1), ("FPCA_GRM_DIV_NONE", 2)):
        assert re.search(r"^#define %s %d$" % (name, val), main, re.M), name
    # the definitions are written down where the prototypes are
    for text in ("Relationship matrix", "S_ij = sum_s z_is z_js", "n_ij == 0 is tested and gives NaN", "i (i + 1) / 2 + j", "G > thr",
                 "sd_s <= 1e-9"):
        assert text in main, text
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "int fpca_bench_grm(fpca_ctx *ctx, int reps, double *ms, double *flops);" in dbg and "fpca_bench_grm" not in main
    names = ("fpca_grm_block", "fpca_grm_tri", "fpca_grm_pairs", "fpca_grm_cutoff", "fpca_bench_grm")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    L = fp.lib()
    # NULL context: -1 with a message that names the entry point, before any device work
    buf = np.zeros(4)
    keep = np.ones(4, dtype=np.uint8)
    i32 = np.zeros(4, dtype=np.uint32)
    n = C.c_uint64(0)
    assert L.fpca_grm_block(None, 0, 2, 0, 2, 0, _vp(buf), _vp(i32)) == -1 and b"fpca_grm_block (NULL context)" in L.fpca_last_error()
    assert L.fpca_grm_tri(None, 0, _vp(buf), None) == -1 and b"fpca_grm_tri (NULL context)" in L.fpca_last_error()
    assert L.fpca_grm_pairs(None, None, 0.1, 0, 4, _vp(i32), _vp(i32), _vp(buf), None, C.byref(n)) == -1
    assert b"fpca_grm_pairs (NULL context)" in L.fpca_last_error()
    assert L.fpca_grm_cutoff(None, 0.025, 0, _vp(keep), None) == -1 and b"fpca_grm_cutoff (NULL context)" in L.fpca_last_error()
    assert L.fpca_bench_grm(None, 1, _vp(buf), None) == -1 and b"fpca_bench_grm (NULL context)" in L.fpca_last_error()


def test_python_signatures():
    import flashpca_amd as fp

    q = inspect.signature(fp.Context.grm_block).parameters
    assert list(q) == ["self", "i0", "ni", "j0", "nj", "divisor", "counts"] and [q[k].default for k in list(q)[5:]] == ["shared", False]
    q = inspect.signature(fp.Context.grm_tri).parameters
    assert list(q) == ["self", "divisor", "counts"] and [q[k].default for k in list(q)[1:]] == ["shared", False]
    q = inspect.signature(fp.Context.grm_pairs).parameters
    assert list(q) == ["self", "thr", "keep", "divisor", "max_pairs"] and [q[k].default for k in list(q)[2:]] == [None, "shared", 1 << 24]
    assert q["thr"].default is inspect.Parameter.empty
    q = inspect.signature(fp.Context.grm_cutoff).parameters
    assert list(q) == ["self", "thr", "keep", "divisor"] and [q[k].default for k in list(q)[1:]] == [0.025, None, "shared"]
    q = inspect.signature(fp.Context.bench_grm).parameters
    assert list(q) == ["self", "reps"] and q["reps"].default == 5
    q = inspect.signature(fp.grm).parameters
    assert list(q) == ["prefix", "divisor", "snps", "maf", "geno", "ld", "device"]
    assert [q[k].default for k in list(q)[1:]] == ["shared", None, 0.0, 1.0, None, 0]
    q = inspect.signature(fp.rel_cutoff).parameters
    assert list(q) == ["prefix", "thr", "divisor", "snps", "maf", "geno", "ld", "keep", "device"]
    assert [q[k].default for k in list(q)[1:]] == [0.025, "shared", None, 0.0, 1.0, None, None, 0]
    assert list(inspect.signature(fp.write_grm).parameters) == ["path", "ids", "tri", "shared"]
    assert list(inspect.signature(fp.read_grm).parameters) == ["path"]
    # flashpca()'s signature is not touched (tests/test_king_rel_cpu.py holds its tail)
    assert list(inspect.signature(fp.flashpca).parameters)[-2:] == ["unrelated_min_shared", "solver_kw"]
    with pytest.raises(ValueError, match="divisor must be one of"):
        fp.api._grm_divisor("n1")
    assert [fp.api._grm_divisor(d) for d in ("shared", "p", "none", 7)] == [0, 1, 2, 7]


def test_triangle_index():
    """Entry i (i + 1) / 2 + j, j <= i, row by row: the order np.tril_indices walks, GCTA's."""
    N = 7
    i, j = np.tril_indices(N)
    assert np.array_equal(i * (i + 1) // 2 + j, np.arange(N * (N + 1) // 2))
    assert 4 * 5 // 2 + 4 == 14 and 4 * 5 // 2 + 0 == 10 and 0 * 1 // 2 + 0 == 0  # the last row of a 5-sample triangle is 10 .. 14


def test_write_read_grm_byte_for_byte(tmp_path):
    import flashpca_amd as fp

    ids = [("F1", "A"), ("F1", "B"), ("F2", "C"), ("F3", "D 4"), ("F3", "E")]  # (an IID with a blank survives: the separator is the tab)
    tri = np.array([1.0, 0.5, 1.25, -0.125, 1e-3, 0.98, 0.0, 1.0 / 3.0, float("nan"), 1.5, 0.25, -1.0, 2.0 ** -30, 7.0, 0.1])
    shared = np.array([1000, 999, 1000, 998, 997, 1000, 3, 2, 0, 5, 16777216, 1, 2, 3, 4], dtype=np.uint32)
    path = str(tmp_path / "five")
    fp.write_grm(path, ids, tri, shared)
    assert open(path + ".grm.bin", "rb").read() == struct.pack("<15f", *tri)
    assert open(path + ".grm.N.bin", "rb").read() == struct.pack("<15f", *[float(v) for v in shared])
    assert open(path + ".grm.id", "rb").read() == b"F1\tA\nF1\tB\nF2\tC\nF3\tD 4\nF3\tE\n"
    back = fp.read_grm(path)
    assert back["ids"] == ids and back["tri"].dtype == np.float32 and back["shared"].dtype == np.float32
    assert np.array_equal(back["tri"], tri.astype(np.float32), equal_nan=True) and np.array_equal(back["shared"], shared.astype(np.float32))
    # entry i (i + 1) / 2 + j of the file is G_ij
    assert back["tri"][3 * 4 // 2 + 1] == np.float32(1.0 / 3.0) and back["tri"][4 * 5 // 2 + 4] == np.float32(0.1)
    # sizes that do not make a triangle are refused, writing and reading
    with pytest.raises(ValueError, match="5 samples have a triangle of 15 entries"):
        fp.write_grm(path, ids, tri[:14], shared[:14])
    with pytest.raises(ValueError, match="5 samples have a triangle of 15 entries"):
        fp.write_grm(path, ids, tri, shared[:10])
    with open(path + ".grm.id", "a") as f:
        f.write("F4\tG\n")
    with pytest.raises(ValueError, match="names 6 samples: a triangle of 21 entries"):
        fp.read_grm(path)


def test_grm_kernels_do_not_spill():
    """The pattern of test_king_rel_kernels_do_not_spill: grm.hip holds nine kernels -- k_grm_live, k_grm_kill, two instances each of
    k_grm_dot and k_grm_shared, three of k_grm_finish -- which compile without spills or scratch, by the compiler's own remarks and by the
    code object's metadata.  k_grm_dot alone uses LDS: 32 KB, the double-buffered table of one 128-byte chunk; four accumulators (32
    registers), the two operand buffers and the staged table leave room for at least two waves per SIMD (printed and held to that).  Its
    loop is 64 FP64 matrix instructions per 16 bytes of a record, each with one 8-byte LDS read in front; the count kernel holds 16 int8
    matrix instructions per chunk; the list is appended with a vector-memory atomic add.
    Recorded: k_grm_dot 113 VGPRs, 0 AGPRs, occupancy 4 waves/SIMD; k_grm_shared 66 VGPRs, occupancy 7."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "grm.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "grm.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    want = {"k_grm_live": 1, "k_grm_kill": 1, "k_grm_dot": 2, "k_grm_shared": 2, "k_grm_finish": 3}
    assert len(names) == 9 and all(sum(k in n for n in names) == v for k, v in want.items()), names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0] * 9, key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 18 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * 9
    fn = re.findall(r"Function Name: (\S+)", r.stderr)
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(fn) == len(occ) == len(vgprs) == len(agprs) == len(lds) == 9
    for f, o, v, a, l in zip(fn, occ, vgprs, agprs, lds):
        print("%s: occupancy %d waves/SIMD, VGPRs %d, AGPRs %d, LDS %d bytes" % (f, o, v, a, l))
        assert o >= 2, (f, o)
        assert l == (32768 if "k_grm_dot" in f else 0), (f, l)
    assert len(re.findall(r"v_mfma_f64_16x16x4_f64", txt)) >= 2 * 64  # (the compiler may unroll the chunk's eight steps)
    assert len(re.findall(r"v_mfma_i32_32x32x32_i8", txt)) >= 2 * 16
    assert "ds_read_b64" in txt and "global_load_dwordx4" in txt and "global_atomic_add_x2" in txt
    # the operand is the table entry itself: the Gram kernel holds no fp64 arithmetic but the matrix instruction
    dot = re.findall(r"^_ZN\w*k_grm_dot\w*:[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M)
    assert len(dot) == 2
    for body in dot:
        assert not re.search(r"v_(fma|mul|add|div\w*)_f64", body)
