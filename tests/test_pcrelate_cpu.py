"""PC-Relate without a GPU: the three entry points in the header with their definitions, the bench hook in the debug header only, the
binding and both builds of the library; the NULL-context refusals; the Python signatures; the register discipline of pcrelate.hip."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_entry_points_declared_bound_and_exported(built_lib):
    import flashpca_amd as fp
    from flashpca_amd import _lib

    main = open(os.path.join(ROOT, "include", "fpca.h")).read()
    for proto in (r"int fpca_pcrelate_beta\(fpca_ctx \*ctx, const double \*pcs /\*[^*]*\*/, int npc, const uint8_t \*train /\*[^*]*\*/,\s*"
                  r"double \*beta /\*[^*]*\*/\);",
                  r"int fpca_pcrelate_block\(fpca_ctx \*ctx, const double \*pcs /\*[^*]*\*/, int npc, const double \*beta /\*[^*]*\*/,\s*"
                  r"const uint8_t \*train /\*[^*]*\*/, double eps, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj,\s*"
                  r"double \*kin /\*[^*]*\*/, double \*den /\*[^*]*\*/\);",
                  r"int fpca_pcrelate_tri\(fpca_ctx \*ctx, const double \*pcs /\*[^*]*\*/, int npc, const double \*beta /\*[^*]*\*/,\s*"
                  r"const uint8_t \*train /\*[^*]*\*/, double eps, double \*kin /\*[^*]*\*/, double \*den /\*[^*]*\*/\);"):
        assert re.search("^" + proto, main, re.M), proto
    # the definitions are written down where the prototypes are
    for text in ("PC-Relate", "x_is in {2, -, 1, 0} for the raw codes {0, 1, 2, 3}", "sd_s > 1e-9", "V = [1 | pcs]", "0 <= npc <= 31",
                 "nothing is re-estimated over train", "rhs_sk = mean_s c_k +", "<= 1e-12 x the largest pivot", "eps < mu_is < 1 - eps (strict)",
                 "r_is = x_is - 2 mu_is", "w_is = sqrt(mu_is (1 - mu_is))", "kin_ij = S_ij / (4 D_ij)", "D_ij == 0 is tested and gives NaN",
                 "2 kin_ii - 1", "i (i + 1) / 2 + j", "bit for bit that of fpca_pcrelate_beta"):
        assert text in main, text
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "int fpca_bench_pcrelate(fpca_ctx *ctx, int npc, int reps, double *ms, double *flops);" in dbg and "fpca_bench_pcrelate" not in main
    names = ("fpca_pcrelate_beta", "fpca_pcrelate_block", "fpca_pcrelate_tri", "fpca_bench_pcrelate")
    for path in (fp.LIB_PATH, fp.HOOKS_LIB_PATH):
        L = C.CDLL(path)
        for name in names:
            assert name in _lib.SIGNATURES and getattr(L, name) is not None, (path, name)
    # the switches that force small slabs and panels exist in the test build only
    assert b"FPCA_PCR_" not in open(fp.LIB_PATH, "rb").read()
    hooks = open(fp.HOOKS_LIB_PATH, "rb").read()
    assert all(n in hooks for n in (b"FPCA_PCR_SLAB_ROWS", b"FPCA_PCR_PANEL_SNPS", b"FPCA_PCR_BENCH_OPERANDS"))
    L = fp.lib()
    # NULL context: -1 with a message that names the entry point, before any device work
    buf = np.zeros(8)
    assert L.fpca_pcrelate_beta(None, _vp(buf), 1, None, _vp(buf)) == -1 and b"fpca_pcrelate_beta (NULL context)" in L.fpca_last_error()
    assert L.fpca_pcrelate_block(None, _vp(buf), 1, None, None, 0.01, 0, 2, 0, 2, _vp(buf), None) == -1
    assert b"fpca_pcrelate_block (NULL context)" in L.fpca_last_error()
    assert L.fpca_pcrelate_tri(None, _vp(buf), 1, None, None, 0.01, _vp(buf), None) == -1 and b"fpca_pcrelate_tri (NULL context)" in L.fpca_last_error()
    assert L.fpca_bench_pcrelate(None, 4, 1, _vp(buf), None) == -1 and b"fpca_bench_pcrelate (NULL context)" in L.fpca_last_error()


def test_python_signatures():
    import flashpca_amd as fp

    empty = inspect.Parameter.empty
    q = inspect.signature(fp.Context.pcrelate_beta).parameters
    assert list(q) == ["self", "pcs", "train"] and q["pcs"].default is empty and q["train"].default is None
    q = inspect.signature(fp.Context.pcrelate_block).parameters
    assert list(q) == ["self", "pcs", "i0", "ni", "j0", "nj", "train", "eps", "beta", "den"]
    assert [q[k].default for k in list(q)[6:]] == [None, 0.01, None, False] and all(q[k].default is empty for k in list(q)[1:6])
    q = inspect.signature(fp.Context.pcrelate_tri).parameters
    assert list(q) == ["self", "pcs", "train", "eps", "beta", "den"] and [q[k].default for k in list(q)[2:]] == [None, 0.01, None, False]
    q = inspect.signature(fp.Context.bench_pcrelate).parameters
    assert list(q) == ["self", "npc", "reps"] and [q[k].default for k in list(q)[1:]] == [4, 5]
    q = inspect.signature(fp.pcrelate).parameters
    assert list(q) == ["prefix", "pcs", "train", "eps", "snps", "maf", "geno", "ld", "device"]
    assert [q[k].default for k in list(q)[2:]] == [None, 0.01, None, 0.0, 1.0, None, 0] and q["pcs"].default is empty
    # flashpca()'s signature is not touched (tests/test_king_rel_cpu.py holds its tail)
    assert list(inspect.signature(fp.flashpca).parameters)[-2:] == ["unrelated_min_shared", "solver_kw"]


def test_pcrelate_kernels_do_not_spill():
    """The pattern of test_grm_kernels_do_not_spill: pcrelate.hip holds six kernels -- k_pcr_beta, k_pcr_operands, two instances each of
    k_pcr_gram and k_pcr_finish -- which compile without spills or scratch, by the compiler's own remarks and by the code object's metadata,
    each with at least one wave per SIMD and k_pcr_gram (a 64 x 64 workgroup tile) with at least two.  k_pcr_gram holds the FP64 matrix
    instruction, 32 per 16-SNP step, fed from LDS by 16-byte reads (64 KB: the two tiles' (r, w) pairs of a step, double-buffered) that the
    16-byte global loads of the next step fill.
    Recorded (also DESIGN 7k): k_pcr_beta 46 VGPRs, 0 AGPRs, LDS 24832, occupancy 2; k_pcr_operands 30 VGPRs, 0 AGPRs, LDS 33856, occupancy 4;
    k_pcr_gram 134 VGPRs, 0 AGPRs, LDS 65536, occupancy 2; k_pcr_finish 16 VGPRs, 0 AGPRs, LDS 0, occupancy 8."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pcrelate.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "pcrelate.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    want = {"k_pcr_beta": 1, "k_pcr_operands": 1, "k_pcr_gram": 2, "k_pcr_finish": 2}
    assert len(names) == 6 and all(sum(k in n for n in names) == v for k, v in want.items()), names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0] * 6, key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 12 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * 6
    fn = re.findall(r"Function Name: (\S+)", r.stderr)
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(fn) == len(occ) == len(vgprs) == len(agprs) == len(lds) == 6
    for f, o, v, a, l in zip(fn, occ, vgprs, agprs, lds):
        print("%s: occupancy %d waves/SIMD, VGPRs %d, AGPRs %d, LDS %d bytes" % (f, o, v, a, l))
        assert o >= (2 if "k_pcr_gram" in f else 1), (f, o)
        if "k_pcr_gram" in f:
            assert l == 65536, (f, l)
        if "k_pcr_finish" in f:
            assert l == 0, (f, l)
    gram = re.findall(r"^_ZN\w*k_pcr_gram\w*:[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M)
    assert len(gram) == 2
    for body in gram:
        assert len(re.findall(r"v_mfma_f64_16x16x4_f64", body)) >= 32
        assert "ds_read_b128" in body and "ds_write_b128" in body and "global_load_dwordx4" in body
        assert "atomic" not in body
