"""PC-Relate IBD sharing without a GPU: the three entry points in the header with their definitions, the bench hook in the debug header
only, the bindings and both builds of the library; the NULL-context refusals; fpca_pcrelate_classify (host only) against a table of
hand-made pairs; the Python signatures; the register discipline of pcrelate_ibd.hip."""
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
    for proto in (r"int fpca_pcrelate_ibd_block\(fpca_ctx \*ctx, const double \*pcs /\*[^*]*\*/, int npc, const double \*beta /\*[^*]*\*/,\s*"
                  r"const uint8_t \*train /\*[^*]*\*/, double eps, const double \*f /\*[^*]*\*/, uint64_t i0, uint64_t ni,\s*"
                  r"uint64_t j0, uint64_t nj, double \*k2 /\*[^*]*\*/, double \*k0 /\*[^*]*\*/,\s*uint32_t \*nsnp /\*[^*]*\*/\);",
                  r"int fpca_pcrelate_ibd_tri\(fpca_ctx \*ctx, const double \*pcs /\*[^*]*\*/, int npc, const double \*beta /\*[^*]*\*/,\s*"
                  r"const uint8_t \*train /\*[^*]*\*/, double eps, const double \*f /\*[^*]*\*/,\s*"
                  r"double \*k2 /\*[^*]*\*/, double \*k0 /\*[^*]*\*/, uint32_t \*nsnp /\*[^*]*\*/\);",
                  r"int fpca_pcrelate_classify\(uint64_t n_pairs, const double \*kin, const double \*k0, const double \*k2, const uint32_t \*nsnp, "
                  r"double k0_switch,\s*double po_k0, double \*k0_out /\*[^*]*\*/, double \*k1_out /\*[^*]*\*/, uint8_t \*type /\*[^*]*\*/\);"):
        assert re.search("^" + proto, main, re.M), proto
    # the definitions are written down where the prototypes are
    for text in ("PC-Relate IBD sharing", "m_is in {0, 1} is the usable indicator", "v = mu (1 - mu)", "gD = mu if x = 0, 0 if x = 1, 1 - mu if x = 2",
                 "q = gD - v", "u = mu^2", "t = (1 - mu)^2", "a = [x = 0]", "c = [x = 2]", "every operand is 0 where m_is = 0",
                 "Q_ij = sum_s q_is q_js", "E_ij = sum_s v_is v_js", "H_ij = sum_s (u_is t_js + t_is u_js)", "I0_ij = sum_s (a_is c_js + c_is a_js)",
                 "n_ij = sum_s m_is m_js", "Q_ij / E_ij - f_i f_j", "never a\n *             fused multiply-add", "E_ij == 0 is tested and gives NaN",
                 "I0_ij / H_ij", "H_ij == 0 is tested and gives NaN", "n_ij as uint32", "carry no meaning", "are the same bits",
                 "k0_out = k0 when kin > k0_switch, else 1 - 4 kin + k2", "k1_out = 1 - k0_out - k2", "conventions of the caller",
                 "Parity with GENESIS::pcrelate is not claimed", "a non-finite\n *   entry of f"):
        assert text in main, text
    assert "#define FPCA_ABI_VERSION 4" in main and _lib.ABI_VERSION == 4  # (no struct changed)
    dbg = open(os.path.join(ROOT, "include", "fpca_debug.h")).read()
    assert "int fpca_bench_pcrelate_ibd(fpca_ctx *ctx, int npc, int reps, double *ms, double *flops);" in dbg and "fpca_bench_pcrelate_ibd" not in main
    assert dbg.index("int fpca_bench_pcrelate(") < dbg.index("int fpca_bench_pcrelate_ibd(")
    names = ("fpca_pcrelate_ibd_block", "fpca_pcrelate_ibd_tri", "fpca_pcrelate_classify", "fpca_bench_pcrelate_ibd")
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
    assert L.fpca_pcrelate_ibd_block(None, _vp(buf), 1, None, None, 0.01, None, 0, 2, 0, 2, _vp(buf), None, None) == -1
    assert b"fpca_pcrelate_ibd_block (NULL context)" in L.fpca_last_error()
    assert L.fpca_pcrelate_ibd_tri(None, _vp(buf), 1, None, None, 0.01, None, _vp(buf), None, None) == -1
    assert b"fpca_pcrelate_ibd_tri (NULL context)" in L.fpca_last_error()
    assert L.fpca_bench_pcrelate_ibd(None, 4, 1, _vp(buf), None) == -1 and b"fpca_bench_pcrelate_ibd (NULL context)" in L.fpca_last_error()


# kin, k0 (the IBS0 form), k2, nsnp -> type, at k0_switch = 0.03125 and po_k0 = 0.1.  np.nextafter gives both sides of every cut point.
def _up(x):
    return float(np.nextafter(x, 1.0))


SWITCH, PO = 0.03125, 0.1
PAIRS = [
    # (kin, k0, k2, nsnp, type)
    (float("nan"), 0.5, 0.1, 100, 255),   # no kinship
    (0.25, float("nan"), 0.1, 100, 255),  # above the switch the IBS0 form is taken: NaN
    (0.01, float("nan"), 0.0, 100, 0),    # below the switch it is not read
    (0.01, 0.9, float("nan"), 100, 255),  # below the switch k0_out rests on k2
    (0.25, 0.0, 0.0, 0, 255),             # no shared SNP
    (0.5, 0.0, 1.0, 100, 5),
    (_up(0.354), 0.0, 1.0, 100, 5),
    (0.354, 0.0, 0.3, 100, 1),
    (0.354, 0.25, 0.3, 100, 2),
    (0.25, 0.0, 0.0, 100, 1),
    (0.25, float(np.nextafter(PO, 0.0)), 0.0, 100, 1),
    (0.25, PO, 0.25, 100, 2),             # (strict: k0_out < po_k0)
    (0.25, 0.25, 0.25, 100, 2),
    (_up(0.177), 0.0, 0.0, 100, 1),
    (_up(0.177), 0.3, 0.2, 100, 2),
    (0.177, 0.0, 0.0, 100, 3),
    (0.125, 0.5, 0.0, 100, 3),
    (_up(0.0884), 0.6, 0.0, 100, 3),
    (0.0884, 0.6, 0.0, 100, 4),
    (0.0625, 0.75, 0.0, 100, 4),
    (_up(0.0442), 0.8, 0.0, 100, 4),
    (0.0442, 0.8, 0.0, 100, 0),
    (_up(SWITCH), 0.7, 0.01, 100, 0),     # just above the switch: the IBS0 form
    (SWITCH, 0.7, 0.01, 100, 0),          # at the switch (strict): 1 - 4 kin + k2
    (0.0, 0.9, 0.0, 1, 0),
    (-0.01, 0.9, -0.002, 100, 0),
]


def test_classify_against_hand_made_pairs(built_lib):
    import flashpca_amd as fp

    kin, k0, k2 = (np.array([p[c] for p in PAIRS]) for c in range(3))
    nsnp = np.array([p[3] for p in PAIRS], dtype=np.uint32)
    want = np.array([p[4] for p in PAIRS], dtype=np.uint8)
    assert set(want) == {0, 1, 2, 3, 4, 5, 255}  # every code
    g0, g1, typ = fp.pcrelate_classify(kin, k0, k2, nsnp, k0_switch=SWITCH, po_k0=PO)
    with np.errstate(invalid="ignore"):
        e0 = np.where(kin > SWITCH, k0, 1.0 - 4.0 * kin + k2)
        e1 = 1.0 - e0 - k2
    for p, row in enumerate(PAIRS):
        print("kin %-22r k0 %-22r k2 %-8r nsnp %-4d -> k0_out %-22r k1_out %-22r type %d (expected %d)" % (row[:4] + (g0[p], g1[p], typ[p], row[4])))
    assert np.array_equal(g0, e0, equal_nan=True) and np.array_equal(g1, e1, equal_nan=True)
    assert g0[22] == 0.7 and g0[23] == 1.0 - 4.0 * SWITCH + 0.01  # both sides of k0_switch
    assert typ.dtype == np.uint8 and np.array_equal(typ, want), np.flatnonzero(typ != want)
    # the defaults: 2^-5.5 and 0.1
    d0, d1, dt = fp.pcrelate_classify(kin, k0, k2, nsnp)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(d0, np.where(kin > 2 ** -5.5, k0, 1.0 - 4.0 * kin + k2), equal_nan=True)
    # no pairs at all
    z = np.zeros(0)
    assert all(a.size == 0 for a in fp.pcrelate_classify(z, z, z, np.zeros(0, dtype=np.uint32)))
    L = fp.lib()
    out0, out1, t8 = np.zeros(2), np.zeros(2), np.zeros(2, dtype=np.uint8)
    two, n2 = np.zeros(2), np.ones(2, dtype=np.uint32)
    for sw, po in ((float("nan"), 0.1), (float("inf"), 0.1), (0.03, float("nan")), (0.03, float("-inf"))):
        assert L.fpca_pcrelate_classify(2, _vp(two), _vp(two), _vp(two), _vp(n2), sw, po, _vp(out0), _vp(out1), _vp(t8)) == -1, (sw, po)
        assert b"fpca_pcrelate_classify" in L.fpca_last_error()
    assert L.fpca_pcrelate_classify(2, None, _vp(two), _vp(two), _vp(n2), 0.03, 0.1, _vp(out0), _vp(out1), _vp(t8)) == -1
    assert L.fpca_pcrelate_classify(2, _vp(two), _vp(two), _vp(two), _vp(n2), 0.03, 0.1, _vp(out0), _vp(out1), None) == -1
    assert L.fpca_pcrelate_classify(0, None, None, None, None, 0.03, 0.1, None, None, None) == 0
    with pytest.raises(ValueError):
        fp.pcrelate_classify(two, two, two[:1], n2)


def test_python_signatures():
    import flashpca_amd as fp

    empty = inspect.Parameter.empty
    q = inspect.signature(fp.Context.pcrelate_ibd_block).parameters
    assert list(q) == ["self", "pcs", "i0", "ni", "j0", "nj", "f", "train", "eps", "beta"]
    assert [q[k].default for k in list(q)[6:]] == [None, None, 0.01, None] and all(q[k].default is empty for k in list(q)[1:6])
    q = inspect.signature(fp.Context.pcrelate_ibd_tri).parameters
    assert list(q) == ["self", "pcs", "f", "train", "eps", "beta"] and [q[k].default for k in list(q)[2:]] == [None, None, 0.01, None]
    q = inspect.signature(fp.Context.bench_pcrelate_ibd).parameters
    assert list(q) == ["self", "npc", "reps"] and [q[k].default for k in list(q)[1:]] == [4, 5]
    q = inspect.signature(fp.pcrelate_classify).parameters
    assert list(q) == ["kin", "k0", "k2", "nsnp", "k0_switch", "po_k0"] and [q[k].default for k in list(q)[4:]] == [2 ** -5.5, 0.1]
    q = inspect.signature(fp.pcrelate_ibd).parameters
    assert list(q) == ["prefix", "pcs", "train", "eps", "k0_switch", "snps", "maf", "geno", "ld", "device"]
    assert [q[k].default for k in list(q)[2:]] == [None, 0.01, 2 ** -5.5, None, 0.0, 1.0, None, 0] and q["pcs"].default is empty
    q = inspect.signature(fp.pcrelate_related).parameters
    assert list(q)[:6] == ["prefix", "pcs", "train", "thr", "min_snps", "po_k0"] and list(q)[-5:] == ["snps", "maf", "geno", "ld", "device"]
    assert [q[k].default for k in list(q)[2:6]] == [None, 2 ** -5.5, 0, 0.1] and [q[k].default for k in list(q)[-5:]] == [None, 0.0, 1.0, None, 0]
    # what the existing tests pin is not touched
    assert list(inspect.signature(fp.pcrelate).parameters) == ["prefix", "pcs", "train", "eps", "snps", "maf", "geno", "ld", "device"]
    assert list(inspect.signature(fp.flashpca).parameters)[-2:] == ["unrelated_min_shared", "solver_kw"]


def test_pcrelate_ibd_kernels_do_not_spill():
    """The pattern of test_pcrelate_kernels_do_not_spill: pcrelate_ibd.hip holds five kernels -- k_pcr_ibd_operands, k_pcr_ibd for the
    rectangle and for the triangle (each the three instances of one template, one per product set, chosen by grid.y) and two of
    k_pcr_ibd_finish -- which compile without spills or scratch, by the compiler's own remarks and by the code object's metadata.
    k_pcr_ibd was designed for two waves per SIMD (two accumulator sets per instance, 64 registers, and 64 KB of LDS: two workgroups fit a
    CU's 160 KB); that is asserted.  It holds the FP64 matrix instruction -- 32 per 16-SNP step in the two fp64 instances, 48 in the
    integer one, 112 in all -- fed from LDS by 16-byte reads that the 16-byte global loads of the next step fill, and no atomics.
    Recorded (also DESIGN 7l): k_pcr_ibd_operands 30 VGPRs, 0 AGPRs, LDS 33856, occupancy 4; k_pcr_ibd 153 (triangle) / 158 (rectangle)
    VGPRs, 0 AGPRs, LDS 65536, occupancy 2 -- compiled alone the instances take 134 (q, v), 134 (u, t) and 150 (s, m); k_pcr_ibd_finish 19
    VGPRs, 0 AGPRs, LDS 0, occupancy 8."""
    csrc = os.path.join(ROOT, "flashpca_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "pcrelate_ibd.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "pcrelate_ibd.hip"), "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        txt = open(out).read()
    names = re.findall(r"\.name:\s+(\S+)", txt)
    want = {"k_pcr_ibd_operands": 1, "k_pcr_ibdILb": 2, "k_pcr_ibd_finish": 2}
    assert len(names) == 5 and all(sum(k in n for n in names) == v for k, v in want.items()), names
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        assert [int(v) for v in re.findall(r"\.%s:\s+(\d+)" % key, txt)] == [0] * 5, key
    remarks = re.findall(r"remark:\s+(VGPRs|SGPRs) Spill: (\d+)", r.stderr)
    assert len(remarks) == 10 and all(int(v) == 0 for _, v in remarks), remarks
    assert [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)] == [0] * 5
    fn = re.findall(r"Function Name: (\S+)", r.stderr)
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    vgprs = [int(v) for v in re.findall(r"remark:\s+VGPRs: (\d+)", r.stderr)]
    agprs = [int(v) for v in re.findall(r"remark:\s+AGPRs: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(fn) == len(occ) == len(vgprs) == len(agprs) == len(lds) == 5
    for f, o, v, a, l in zip(fn, occ, vgprs, agprs, lds):
        print("%s: occupancy %d waves/SIMD, VGPRs %d, AGPRs %d, LDS %d bytes" % (f, o, v, a, l))
        if "k_pcr_ibdILb" in f:
            assert o == 2 and l == 65536 and v + a <= 256, (f, o, l, v, a)
        else:
            assert o >= 1, (f, o)
        if "k_pcr_ibd_finish" in f:
            assert l == 0, (f, l)
    gram = re.findall(r"^(_ZN\w*k_pcr_ibdILb\w*):[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M)
    assert len(gram) == 2
    for name, body in gram:
        mfma = len(re.findall(r"v_mfma_f64_16x16x4_f64", body))
        assert mfma >= 32 + 32 + 48, (name, mfma)
        assert "ds_read_b128" in body and "ds_write_b128" in body and "global_load_dwordx4" in body
        assert "atomic" not in body
    # the finish kernel rounds f_i f_j before it subtracts: a multiply and an add of their own
    for name, body in re.findall(r"^(_ZN\w*k_pcr_ibd_finish\w*):[^\n]*\n(.*?)s_endpgm", txt, re.S | re.M):
        assert "v_mul_f64" in body and "v_add_f64" in body, name
