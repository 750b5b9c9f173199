"""The missing-call gathers under a capped grid (csrc/missing_kernels.hip: k_sparse_rows_sum, k_sparse_rows_sum_batched).

Both kernels walk their rows in a grid-stride loop, one wave a row, so the number of blocks decides which wave adds a row's entries and
nothing about the additions: a gather launched with the few blocks that stay resident beside a GEMM must leave the bits the full grid
leaves.

Kernel level (fpca_debug_gather; the test build's FPCA_GATHER_BLOCKS = n caps the grid of every launch; one child process per value):
unset against 1, 2, 5 and 64 blocks, outputs compared as uint64 bit patterns.  Data: random reals over forty octaves, fp64 rows and fp32
rows with colw; 16 / 32 / 64 columns; the plain kernel, the batched kernel, the batched kernel with a per-row factor (fp64 rows); with
and without init; rows_out 1, 7 and 1031 with nrec = rows_out - 3 lists (none for a single row) and zero rows behind them -- one block
walks 1031 rows, 64 blocks are more than 7 rows can use; lists of 0, 1, 15, 16, 17, 63, 64, 65 and 257 entries: every residue of the
16-entry iteration and of the 64-entry batch.  The output is NaN before the launch.

Operator level (route 3 forced, 2500 x 2100, 16 columns, 7 and 4 slices, 0.1 % and 0.4 % missing calls): with FPCA_SPARSE_SIDE_BYTES=1
the gathers go to the side stream with the resident grid -- X'B, X T and X X'B must have the bits they have with the gathers inline, and
so with one block on the side stream."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 257]
ROWS_OUT = [1, 7, 1031]
BLOCKS = [None, 1, 2, 5, 64]

_KERNEL_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
LENGTHS, ROWS_OUT = %r, %r
out = {}
with fp.test_hooks():
    for b in (16, 32, 64):
        rng = np.random.default_rng(7 * b)
        v_rows = 601
        V64 = rng.standard_normal((v_rows, b)) * np.exp2(rng.uniform(-20, 20, size=(v_rows, 1)))
        rs = rng.uniform(0.5, 2.0, size=v_rows)
        colw = 2.0 ** (np.arange(b) %% 23 - 11.0)
        for rows_out in ROWS_OUT:
            nrec = max(rows_out - 3, 0)
            lens = [LENGTHS[(r * 4 + 8) %% len(LENGTHS)] for r in range(nrec)]  # (7 rows: 257, 16, 65, 15; 1031 rows: all nine)
            ptr = np.zeros(nrec + 1, dtype=np.int64)
            np.cumsum(lens, out=ptr[1:])
            idx = np.concatenate([np.sort(rng.choice(v_rows, size=n, replace=False)) for n in lens] + [np.zeros(0, dtype=np.int64)])
            init = rng.standard_normal((rows_out, b))
            # (kernel, short_lists, rowscale): the plain kernel, the batched one, the batched one with a per-row factor
            for f32 in (False, True):
                for kname, short, scale in (("plain", False, None), ("batched", True, None), ("scaled", True, rs)):
                    if f32 and scale is not None:
                        continue
                    for with_init in (False, True):
                        res, variant = fp.api.debug_gather(ptr, idx, V64.astype(np.float32) if f32 else V64, b, rows_out=rows_out, rowscale=scale,
                                                           colw=colw if f32 else None, init=init if with_init else None, short_lists=short)
                        assert variant == (1 if kname == "plain" else 2), (kname, variant)
                        out["%%d.%%d.%%s.%%s.%%d" %% (b, rows_out, "f32" if f32 else "f64", kname, with_init)] = res.view(np.uint64)
np.savez(sys.argv[2], **out)
""" % (LENGTHS, ROWS_OUT)

_OP_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
N, P, b = 2500, 2100, 16
out, info = {}, {}
with fp.test_hooks():
    for S in (7, 4):
        for miss in (0.001, 0.004):
            with fp.Context.synthetic(N, P, n_pop=6, missing_rate=miss, accum="i8x%d" % S) as ctx:
                key = "S%d.%g" % (S, miss)
                info[key] = ctx.missing_mode(b)
                rng = np.random.default_rng(100 * S + int(1e4 * miss))
                B, T = rng.standard_normal((N, b)), rng.standard_normal((P, b))
                out[key + ".xt"] = ctx.apply_xt(B).view(np.uint64)
                out[key + ".x"] = ctx.apply_x(T).view(np.uint64)
                out[key + ".xxt"] = ctx.apply_xxt(B).view(np.uint64)
np.savez(sys.argv[2], **out)
print("CHILD " + json.dumps(info))
"""


_LAUNCH = re.compile(r"gather launch: kernel (\d), (\d+) rows, (\d+) blocks, limit (\d+)")


def _child(code, env_extra, path):
    """-> (the child's arrays, its stdout, its gather launches as (kernel, rows, blocks, limit) in launch order)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    env.update(env_extra)
    env["FPCA_GATHER_VERBOSE"] = "1"
    r = subprocess.run([sys.executable, "-c", code, ROOT, path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return dict(np.load(path)), r.stdout, [tuple(int(x) for x in m.groups()) for m in _LAUNCH.finditer(r.stderr)]


@pytest.fixture(scope="module")
def kernel_runs(built_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gather_resident")
    res = {}
    for n in BLOCKS:
        arrays, _, launches = _child(_KERNEL_CHILD, {} if n is None else {"FPCA_GATHER_BLOCKS": str(n)}, str(tmp / ("k%s.npz" % n)))
        # the switch did what it says: every launch one of the two kernels, on (rows + 3) / 4 blocks or the cap
        assert len(launches) == len(arrays) and {k for k, _, _, _ in launches} == {1, 2}
        for kernel, rows, blocks, limit in launches:
            assert limit == (n or 0) and blocks == min((rows + 3) // 4, n or 1 << 30), (n, kernel, rows, blocks, limit)
        res[n] = arrays
    return res


def test_cases_are_complete(kernel_runs):
    full = kernel_runs[None]
    assert len(full) == 3 * len(ROWS_OUT) * 5 * 2  # widths x rows_out x (fp64: plain, batched, scaled; fp32: plain, batched) x init
    for key, bits in full.items():
        b, rows_out = (int(x) for x in key.split(".")[:2])
        v = bits.view(np.float64)
        assert v.shape == (rows_out, b) and np.isfinite(v).all(), key
        if key.endswith(".0"):  # without init: the rows behind the lists are zero, the listed ones (but for the empty list) are not
            nrec = max(rows_out - 3, 0)
            assert not v[nrec:].any(), key
            if rows_out == 1031:
                assert (v[:nrec] != 0).all(axis=1).sum() == nrec - len(range(7, nrec, 9)), key  # (list r is empty for r = 7, 16, 25, ...)


@pytest.mark.parametrize("blocks", BLOCKS[1:])
def test_capped_grid_leaves_the_same_bits(kernel_runs, blocks):
    full, capped = kernel_runs[None], kernel_runs[blocks]
    assert sorted(full) == sorted(capped)
    differing = [k for k in sorted(full) if not np.array_equal(full[k], capped[k])]
    print("FPCA_GATHER_BLOCKS=%d: %d cases, differing: %s" % (blocks, len(full), differing))
    assert not differing


@pytest.fixture(scope="module")
def operator_runs(built_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gather_resident_op")
    envs = {"inline": {}, "side": {"FPCA_SPARSE_SIDE_BYTES": "1"}, "side-1-block": {"FPCA_SPARSE_SIDE_BYTES": "1", "FPCA_GATHER_BLOCKS": "1"}}
    res = {}
    for name, env in envs.items():
        arrays, stdout, launches = _child(_OP_CHILD, dict(env, FPCA_I8_MODE="3"), str(tmp / (name + ".npz")))
        info = json.loads([l for l in stdout.splitlines() if l.startswith("CHILD ")][-1][6:])
        assert all(m == 3 for m in info.values()), (name, info)
        # per context X'B, X T, X X'B: four gathers, of which the per-SNP ones (the plain kernel over the padded SNPs) are the first and
        # the third; the per-sample lists are a few entries long here and take the several-rows-per-wave kernel, which is never capped.
        # Inline the plain kernel takes the full grid; on the side stream the resident one at 0.1 % and the full grid at 0.4 %, where a
        # gather outlasts its GEMM (missing_routes.hip, RESIDENT_GATHER_MAX_RATE)
        assert len(launches) == 4 * 4, launches
        k2 = [l for l in launches if l[0] == 1]
        assert len(k2) == 2 * 4 and all(2100 <= rows <= 2560 for _, rows, _, _ in k2), launches
        assert all(limit == 0 for kernel, _, _, limit in launches if kernel == 3) or name == "side-1-block"
        for i, (_, rows, blocks, limit) in enumerate(k2):
            full = (rows + 3) // 4
            resident = (i // 2) % 2 == 0  # contexts in the child's order: (7, 0.1 %), (7, 0.4 %), (4, 0.1 %), (4, 0.4 %)
            if name == "inline" or (name == "side" and not resident):
                assert (blocks, limit) == (full, 0), (name, i, blocks, limit)
            elif name == "side":
                assert limit > 0 and blocks == min(full, limit), (name, i, blocks, limit)
                print("side stream, context %d: %d rows, resident limit %d, %d blocks (inline %d)" % (i // 2, rows, limit, blocks, full))
            else:
                assert (blocks, limit) == (1, 1), (name, i, blocks, limit)
        res[name] = arrays
    return res


@pytest.mark.parametrize("arm", ["side", "side-1-block"])
def test_operator_side_stream_gathers_leave_the_same_bits(operator_runs, arm):
    inline, side = operator_runs["inline"], operator_runs[arm]
    assert len(inline) == 2 * 2 * 3 and sorted(inline) == sorted(side)
    for key, bits in inline.items():
        v = bits.view(np.float64)
        assert np.isfinite(v).all() and np.abs(v).max() > 0, key
    differing = [k for k in sorted(inline) if not np.array_equal(inline[k], side[k])]
    print("%s against inline: %d outputs, differing: %s" % (arm, len(inline), differing))
    assert not differing
