"""The generated code of the L1-bypassing twins of the int8 GEMM (csrc/kernels_i8.hip: I8Nt), read from hipcc -S for gfx950 the way
test_gpu_i8_tiled.py reads register counts.  No GPU.

A twin differs from its plain instance in the `nt` bit of the packed-word loads and in nothing else: the same registers, no spill, the same
number of 16- and 8-byte global loads, instruction for instruction the same length, and `nt` on no store.  How many loads carry the bit
follows from the kernel's issue sites: issue_p is called in the prologue and once per chunk (2 sites of MT x PW packed pieces); issue_q
in the prologue and once per chunk by a 4-wave kernel (2 sites), and by an 8-wave kernel twice in the prologue, once per chunk, and three
times more on the path of the idle waves of a half tile (6 sites) -- NP pieces per site, of which the 8-wave half-tile kernel loads one
as 8 bytes; these stay plain.  The gather kernels (csrc/missing_kernels.hip) keep default-policy loads throughout: `nt` on their rows and
index lists was measured and lost (profiles/load_policy_ab.txt)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asm(src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                               os.path.join(ROOT, "flashpca_amd", "csrc", src), "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def _bodies(txt, pat):
    """{symbol: its instructions} of the kernels whose symbol matches."""
    lines = txt.split("\n")
    res = {}
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN4fpca4kern\w+):", l)
        if m and re.search(pat, m.group(1)):
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            res[m.group(1)] = [x.split(";")[0].strip() for x in lines[i + 1:end]]
    return res


def _count(body, op, nt=None):
    hits = [x for x in body if x.split() and x.split()[0] == op]
    return len(hits) if nt is None else sum(1 for x in hits if (x.split()[-1] == "nt") == nt)


@pytest.fixture(scope="module")
def gemm():
    txt = _asm("kernels_i8.hip")
    regs = {}  # symbol -> (VGPRs + AGPRs as the code object states them, AGPRs, spilled VGPRs)
    for block in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        regs[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)), int(block.split()[0]), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)))
    return _bodies(txt, "k_gemm_i8"), regs


_CFG = r"5I8CfgI((?:L[bi]\d+E)+)E"


def _cfg(m):
    return tuple(int(x) for x in re.findall(r"L[bi](\d+)E", m))


def test_gemm_twins_differ_in_the_policy_bit_alone(gemm):
    bodies, regs = gemm
    plain, twins = {}, {}
    for name in bodies:
        m = re.search(r"k_gemm_i8INS\d_4I8NtINS\d_" + _CFG + r"EEE", name)
        if m:
            twins[_cfg(m.group(1))] = name
            continue
        m = re.search(r"k_gemm_i8INS\d_" + _CFG, name)
        assert m, name
        plain[_cfg(m.group(1))] = name
    # (TWO, MT, NT, WR, WC, KC, G, MODE, HALF, TILED): the headline's 3.5 tiles at 512 and 256 rows, the cheap pass's 2 tiles at 256 rows
    shapes = [(0, 2, 4, 8, 1, 256, 1, 2, 1, 1), (0, 2, 4, 4, 1, 256, 1, 2, 1, 1), (0, 2, 2, 4, 1, 256, 1, 2, 0, 1)]
    assert sorted(twins) == sorted(shapes), sorted(twins)
    for name in plain.values():  # no other instance carries the bit anywhere
        assert not any(x.endswith(" nt") for x in bodies[name]), name
    for cfg, name in sorted(twins.items()):
        body, base = bodies[name], bodies[plain[cfg]]
        _, mt, nt, wr, _, kc, _, _, half, _ = cfg
        pw, threads, cols = kc // 128, 64 * wr, 32 * nt - 16 * half
        rstep = threads // (kc // 16)
        half8 = bool(half) and rstep == 32
        np16 = (cols - 16) // rstep if half8 else cols // rstep  # 16-byte operand pieces per site (and one 8-byte piece if half8)
        sites_p, sites_q = 2, (6 if wr == 8 else 2)
        assert regs[name] == regs[plain[cfg]] and regs[name][2] == 0, (name, regs[name], regs[plain[cfg]])
        assert regs[name][0] > 0
        n16, n8 = _count(body, "global_load_dwordx4"), _count(body, "global_load_dwordx2")
        assert (n16, n8) == (_count(base, "global_load_dwordx4"), _count(base, "global_load_dwordx2")), name
        assert n16 == sites_p * mt * pw + sites_q * np16, (name, n16)  # every 16-byte load of the kernel is one of the two streams
        assert _count(body, "global_load_dwordx4", nt=True) == sites_p * mt * pw, name
        assert _count(body, "global_load_dwordx2", nt=True) == 0, name
        assert n8 >= (sites_q if half8 else 0)
        marked = [x for x in body if x.endswith(" nt")]
        assert all(x.split()[0] == "global_load_dwordx4" for x in marked), [x for x in marked if "load" not in x][:3]
        assert len(body) == len(base), (name, len(body), len(base))  # instruction for instruction the plain kernel
        print(cfg, "registers", regs[name], "16-byte loads", n16, "8-byte loads", n8, "nt", len(marked))


def test_gather_kernels_keep_plain_loads():
    bodies = _bodies(_asm("missing_kernels.hip"), "k_sparse_rows_sum")
    assert len(bodies) == 2 * (3 + 3 + 2), sorted(bodies)  # fp64 / fp32 rows: plain and batched at 16, 32, 64 columns, several-rows at 16, 32
    for name, body in bodies.items():
        assert any(x.startswith("global_load_") for x in body) and not any(x.endswith(" nt") for x in body), name
