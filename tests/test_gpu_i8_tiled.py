"""The band-tiled packed copies of the int8 GEMMs (csrc/kernels.hpp packed_piece_offset).

The layout changes which bytes a lane loads from where, nothing else: the integer sums are exact and every floating-point operation
downstream runs in the same order, so the operator on the tiled copies must equal the operator on the row-major ones BIT FOR BIT.
Each setting runs in a fresh child process on the -DFPCA_TEST_HOOKS build (FPCA_I8_TILED=0: every copy row-major, as before the
tiling; FPCA_DEBUG_I8_NOK2COPY: no third copy, K2 stays on the row-major kernel).  Y comes from Context.apply_xxt, which stages the
host block and calls the library's apply_xxt_dev on it."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
case = json.loads(sys.argv[2])
with fp.test_hooks():
    with fp.Context.synthetic(case["N"], case["P"], n_pop=case.get("n_pop", 6), missing_rate=case["miss"], accum="i8x%d" % case["S"],
                              realistic=case.get("realistic", False)) as ctx:
        if case.get("comm"):
            ctx.comm_init_rank(1, 0, fp.Context.comm_unique_id())
        B = np.random.default_rng(case["N"] + case["b"]).standard_normal((case["N"], case["b"]))
        Y = ctx.apply_xxt(B)
        Y2 = ctx.apply_xxt(B)  # (the second apply finds every buffer and list in place)
        info = {"mode": ctx.missing_mode(case["b"]), "chunks": ctx.allreduce_chunks() if case.get("comm") else 1,
                "repeat_equal": bool(np.array_equal(Y, Y2))}
        if case.get("oracle"):
            np.save(sys.argv[3] + ".packed.npy", ctx.download_packed())
np.save(sys.argv[3], Y)
print("CHILD " + json.dumps(info))
"""

# b in {16, 32, 64} x S in {4, 7}; ragged N and P (no multiple of 256); P = 700 pads to 768 SNPs = 192 bytes per sample row: an odd
# number (3) of 64-byte chunks; 1999 pads to 2048 (8 chunks)
CASES = [
    dict(id="b16-S7-nothing-missing-oracle", N=3001, P=1999, b=16, S=7, miss=0.0, mode=2, oracle=True),
    dict(id="b32-S7-sparse-odd-chunks", N=2050, P=700, b=32, S=7, miss=0.001, mode=3, env={"FPCA_I8_MODE": "3"}),
    dict(id="b64-S7-sparse", N=1300, P=1999, b=64, S=7, miss=0.001, mode=3, env={"FPCA_I8_MODE": "3"}),
    dict(id="b16-S4-nothing-missing-odd-chunks", N=2050, P=700, b=16, S=4, miss=0.0, mode=2),
    dict(id="b32-S4-sparse", N=3001, P=1999, b=32, S=4, miss=0.001, mode=3, env={"FPCA_I8_MODE": "3"}),
    dict(id="b64-S4-nothing-missing-odd-chunks", N=1300, P=700, b=64, S=4, miss=0.0, mode=2),
    dict(id="b16-S7-hybrid", N=3000, P=2000, b=16, S=7, miss=0.001, mode=4, n_pop=3, realistic=True),
    # K3 in three row chunks of the sample-major copy (built-in communicator on one rank): launches at r0 > 0
    dict(id="b32-S7-row-chunks", N=40000, P=1500, b=32, S=7, miss=0.001, mode=3, comm=True, chunks=3,
         env={"FPCA_AR_CHUNKS": "3", "FPCA_I8_MODE": "3"}),
    # no third copy: K3 on the tiled sample-major copy, K2 on the row-major matrix
    dict(id="b16-S7-no-third-copy", N=3001, P=1999, b=16, S=7, miss=0.001, mode=3, env={"FPCA_I8_MODE": "3"},
         env_tiled={"FPCA_DEBUG_I8_NOK2COPY": "1"}),
    # the two-matrix kernels read the tiled sample-major copy too (K2 of these routes stays on the row-major matrix)
    dict(id="b16-S7-both-matrices", N=3001, P=700, b=16, S=7, miss=0.001, mode=0, env={"FPCA_I8_MODE": "0"}),
    dict(id="b32-S4-skip-empty-blocks", N=2050, P=1999, b=32, S=4, miss=0.0002, mode=1, env={"FPCA_I8_MODE": "1"}),
]


def _run(case, tiled, out):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    env.update(case.get("env", {}))
    env["FPCA_I8_TILED"] = "1" if tiled else "0"
    if tiled:
        env.update(case.get("env_tiled", {}))
    spec = {k: v for k, v in case.items() if k not in ("env", "env_tiled", "id")}
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(spec), out], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
    return np.load(out), info, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_tiled_and_row_major_copies_give_the_same_bits(case, built_lib):
    with tempfile.TemporaryDirectory() as tmp:
        Y0, i0, _ = _run(case, False, os.path.join(tmp, "y0.npy"))
        Y1, i1, err1 = _run(case, True, os.path.join(tmp, "y1.npy"))
        assert i0["mode"] == case["mode"] and i1["mode"] == case["mode"], (i0, i1)  # the route the case is about
        assert i0["chunks"] == case.get("chunks", 1) and i1["chunks"] == case.get("chunks", 1)
        assert i0["repeat_equal"] and i1["repeat_equal"]
        assert ("no band-tiled copy" in err1) == ("env_tiled" in case), err1[-1000:]  # the third copy was made unless the case forbids it
        assert np.isfinite(Y1).all() and np.max(np.abs(Y1)) > 0
        assert np.array_equal(Y0, Y1), "max |difference| %g of %g" % (np.max(np.abs(Y0 - Y1)), np.max(np.abs(Y0)))
        if case.get("oracle"):  # ... and against the oracle's dense product, at the tolerance of test_operator_parity
            from oracle import oracle as O

            packed = np.load(os.path.join(tmp, "y1.npy.packed.npy"))
            X = O.OracleData(packed=packed, N=case["N"], P=case["P"], stand="binom2").dense()
            B = np.random.default_rng(case["N"] + case["b"]).standard_normal((case["N"], case["b"]))
            Z = X @ (X.T @ B)
            assert np.max(np.abs(Y1 - Z) / np.max(np.abs(Z), axis=0)) <= 1e-11


def _gemm_registers():
    """(VGPRs + AGPRs as the code object states them, spilled VGPRs) of every k_gemm_i8 instance, keyed by its I8Cfg arguments."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                               os.path.join(ROOT, "flashpca_amd", "csrc", "kernels_i8.hip"), "-o", out], stderr=subprocess.DEVNULL)
        txt = open(out).read()
    regs = {}
    for name, vgpr, spill in re.findall(r"\.name:\s+(\S+)\s.*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)", txt, re.S):
        m = re.search(r"k_gemm_i8INS\d_5I8CfgI((?:L[bi]\d+E)+)E", name)
        if m:
            regs[tuple(int(x) for x in re.findall(r"L[bi](\d+)E", m.group(1)))] = (int(vgpr), int(spill))
    return regs


def test_tiled_gemm_instances_need_no_more_registers_than_their_twins():
    """Same -S output as test_gemm_kernels_do_not_spill: every TILED instance of k_gemm_i8 (last I8Cfg argument) has a row-major twin
    and needs no more VGPRs + AGPRs than it (the unified register count of the code object), so the occupancy is the twin's: two
    workgroups per CU for the 3.5-tile one-matrix kernel of the headline.  Every one-matrix shape the default routes launch -- G.M
    alone, 2 to 8 tiles and the two half-tile shapes -- has a TILED instance."""
    regs = _gemm_registers()
    tiled = {k: v for k, v in regs.items() if len(k) == 10 and k[9] == 1}
    assert len(tiled) >= 9
    for nt, half in [(n, 0) for n in range(2, 9)] + [(2, 1), (4, 1)]:
        assert (0, 2, nt, 4, 1, 256, 1, 2, half, 1) in tiled, (nt, half)
    for k, (v, spill) in sorted(tiled.items()):
        twin = regs[k[:9] + (0,)]
        print(k, "registers", v, "twin", twin[0])
        assert spill == 0
        if k[0] == 0:  # the one-matrix kernels: the count itself
            assert v <= twin[0], (k, v, twin)
        else:  # the two-matrix kernels (one workgroup per CU either way): what the hardware allocates, in blocks of 8 registers
            assert (v + 7) // 8 <= (twin[0] + 7) // 8, (k, v, twin)
    v = tiled[(0, 2, 4, 4, 1, 256, 1, 2, 1, 1)][0]
    assert 2 * ((v + 7) // 8 * 8) <= 512  # two workgroups (one wave per SIMD each) share a SIMD's 512 registers
