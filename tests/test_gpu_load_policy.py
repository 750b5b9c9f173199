"""The L1-bypassing loads of the int8 GEMM's packed words (csrc/kernels_i8.hip: I8Nt, i8_nt_p) give the bits of the plain loads.

An `nt` load fetches the same bytes by another way through the caches, so every output must equal the plain arm's byte for byte.  The
switch (test build) is read once per process: FPCA_I8_LOADS = plain | p.  Every group below runs both arms as two child processes side by
side and compares every array.  (Of the arms measured in profiles/load_policy_ab.txt -- packed words, operand pieces, gathered rows, index
lists -- only the packed words are kept; the others, their switches and their instances are gone, and with them their cases here.)

 * Data: synthetic 1,000 samples x 768 SNPs: N_pad = 1,024 = 4 chunks of 256 codes (prologue, three-buffer steady state, the clamped
   re-stage of the last two chunks), P_pad = 768 = one and a half 512-row tiles (waves 4..7 of the last one idle).  X'B, X T and X X'B at
   (b, S) = (16, 7), (16, 4), (32, 7), route 2 (nothing missing) and route 3 (0.5 % missing), with FPCA_I8_ROWS = 512 and 256, unsplit and
   under FPCA_I8_SPLITS = 4 (units of one chunk).
 * Gather edges (every group, route 3, a matrix of its own: the gathers run beside the GEMMs whose loads change): sample 5 is missing in
   70 SNPs (its list crosses the 64-entry batch), SNP 100 has no missing call, every other SNP one to three; and one group more with
   FPCA_SPARSE_SIDE_BYTES = 1 (both gathers on the side stream).
 * The instances: the FPCA_I8_VERBOSE line of every launch names its policy.  A launch whose instance has an L1-bypassing twin (one
   operand, G.M alone, band-tiled: 3.5 tiles at 512 and 256 rows, 2 tiles at 256 rows) must name the arm's policy, every other launch
   `plain`; over the groups all three twins are launched.  They are not in fpca_debug_i8_instances (they share their plain twin's six
   numbers), so the census of test_gpu_i8_planes.py neither sees nor misses them: this is where they run."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = 1000, 768
ARMS = ["plain", "p"]

_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
N, P = 1000, 768
out = {}

def mark(s):
    sys.stderr.write("MARK " + s + "\n")
    sys.stderr.flush()

def applies(ctx, cid, b):
    rng = np.random.default_rng(77 + b)
    Bi = rng.integers(-4, 5, size=(N, b)).astype(np.float64)
    Bn, Tn = rng.standard_normal((N, b)), rng.standard_normal((P, b))
    mark(cid)
    out[cid + ".xt"], out[cid + ".x"], out[cid + ".xxt"] = ctx.apply_xt(Bi), ctx.apply_x(Tn), ctx.apply_xxt(Bn)

def edge_matrix():
    rng = np.random.default_rng(5)
    codes = rng.choice(np.array([0, 2, 3], dtype=np.uint8), size=(P, N))  # code 1 = missing
    for j in range(P):
        if j != 100:
            codes[j, rng.choice(np.setdiff1d(np.arange(N), [5]), size=1 + j % 3, replace=False)] = 1
    codes[[j for j in range(80) if j != 100][:70], 5] = 1
    pad = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    pad[:, :N] = codes
    q = pad.reshape(P, -1, 4)
    return (q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)).astype(np.uint8)

with fp.test_hooks():
    for b, S in ((16, 7), (16, 4), (32, 7)):
        for route, miss in ((2, 0.0), (3, 0.005)):
            os.environ["FPCA_I8_MODE"] = str(route)
            with fp.Context.synthetic(N, P, n_pop=6, missing_rate=miss, accum="i8x%d" % S) as ctx:
                assert ctx.missing_mode(b) == route
                applies(ctx, "b%dS%dr%d" % (b, S, route), b)
    os.environ["FPCA_I8_MODE"] = "3"
    with fp.Context.from_packed(edge_matrix(), N, P, accum="i8x7") as ctx:
        assert ctx.missing_mode(16) == 3
        out["edge.snp_missing"] = ctx.snp_missing()
        applies(ctx, "edge", 16)
np.savez(sys.argv[2], **out)
"""

_LAUNCH = re.compile(r"int8 GEMM launch: (one|two) operands?, mode (\d), nt (\d)( \(half tile\))?, (band-tiled|row-major)(, E alone)?; phase B from row \d+; "
                     r"rows (\d+), loads (\w+)")


def _launched(stderr):
    """[(has an L1-bypassing twin, key, policy named)] of every launch line."""
    res = []
    for m in _LAUNCH.finditer(stderr):
        one, mode, nt, half, tiled, e_only, rows, loads = m.groups()
        key = (int(nt), bool(half), int(rows))
        twin = (one == "one" and mode == "2" and tiled == "band-tiled" and not e_only and key in ((4, True, 512), (4, True, 256), (2, False, 256)))
        res.append((twin, key, loads))
    return res


def _arms(env_extra):
    """Both arms of one group, side by side: [(arrays, stderr)] in the order of ARMS."""
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for i8 in ARMS:
            env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
            env.update(env_extra)
            env.update({"FPCA_I8_VERBOSE": "1", "FPCA_I8_LOADS": i8})
            out = os.path.join(tmp, i8 + ".npz")
            procs.append((out, subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, out], stdout=subprocess.PIPE,
                                                stderr=subprocess.PIPE, text=True, env=env)))
        res = []
        for out, p in procs:
            so, se = p.communicate(timeout=300)
            assert p.returncode == 0, so[-2000:] + se[-3000:]
            res.append((dict(np.load(out)), se))
    return res


def _same_bytes(plain, arm, name):
    assert sorted(plain) == sorted(arm)
    for k in sorted(plain):
        a, w = plain[k], arm[k]
        assert a.dtype == w.dtype and a.shape == w.shape and np.isfinite(a).all(), (name, k)
        assert a.tobytes() == w.tobytes(), (name, k, float(np.max(np.abs(a - w))))


GROUPS = [
    ("rows512", {"FPCA_I8_ROWS": "512"}),
    ("rows512-splits4", {"FPCA_I8_ROWS": "512", "FPCA_I8_SPLITS": "4"}),
    ("rows256", {"FPCA_I8_ROWS": "256"}),
    ("rows256-splits4", {"FPCA_I8_ROWS": "256", "FPCA_I8_SPLITS": "4"}),
    ("rows512-side", {"FPCA_I8_ROWS": "512", "FPCA_SPARSE_SIDE_BYTES": "1"}),
]
_SEEN = {}  # group -> the twins it launched, per arm


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", GROUPS, ids=[g[0] for g in GROUPS])
def test_every_arm_gives_the_plain_bits(name, env, built_lib):
    res = _arms(env)
    plain = res[0][0]
    assert len(plain) == 3 * 7 + 1 and all(np.max(np.abs(v)) > 0 for v in plain.values())
    miss = plain["edge.snp_missing"]
    assert miss[100] == 0 and np.all(np.delete(miss, 100) >= 1) and miss.sum() == sum(1 + j % 3 for j in range(P) if j != 100) + 70
    rows = int(env["FPCA_I8_ROWS"])
    for i8, (arrays, stderr) in zip(ARMS, res):
        _same_bytes(plain, arrays, "%s: %s" % (name, i8))
        launched = _launched(stderr)
        assert len(launched) >= 7 * 4, stderr[-2000:]  # (X'B, X T and both of X X'B, of seven contexts)
        for twin, key, loads in launched:
            assert loads == (i8 if twin else "plain"), (name, i8, key, loads)
        twins = {key for twin, key, _ in launched if twin}
        assert twins == ({(4, True, 512)} if rows == 512 else {(4, True, 256), (2, False, 256)}), (name, twins)
        _SEEN.setdefault(i8, set()).update(twins)
        if "FPCA_I8_SPLITS" in env:  # units of one chunk
            assert "x 4 splits (1 chunks each)" in stderr
    print(name, "arms equal;", len(launched), "launches")


@pytest.mark.gpu
def test_every_twin_instance_was_launched(built_lib):
    """After the groups above (run alone, this starts the two groups that reach them all)."""
    if not all(len(_SEEN.get(i8, ())) == 3 for i8 in ARMS):
        for name, env in (GROUPS[0], GROUPS[2]):
            test_every_arm_gives_the_plain_bits(name, env, built_lib)
    for i8 in ARMS:
        assert _SEEN[i8] == {(4, True, 512), (4, True, 256), (2, False, 256)}, (i8, _SEEN)
