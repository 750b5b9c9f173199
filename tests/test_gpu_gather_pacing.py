"""The order of additions of the fp64 / fp32 gather-sums (csrc/missing_kernels.hip: k_sparse_rows_sum, k_sparse_rows_sum_batched), pinned on
non-integer data.

The two kernels hold two adjacent columns per lane (one 16-byte load of an fp64 row), b / 2 lanes per row.  Their header promises the sums
of the one-column-per-lane kernels they replaced, bit for bit: entry n of a list is added, in list order, to partial sum n mod A of its
column (A = 4 EPW for the plain kernel, 8 EPW for the batched one, EPW = 64 / b), the A / EPW partial sums v = g, g + EPW, g + 2 EPW, ...
of old lane group g are added pairwise ((a0 + a1) + (a2 + a3), and once more for eight), and the EPW group sums by the halving tree
(group g takes group g + EPW / 2, then g + EPW / 4, ...).  tests/test_gpu_missing_gathers.py compares the kernels with int64 sums of
integer-valued rows, which any order of additions satisfies; here the rows are random reals over forty octaves (fp32 rows too: their
widened sums do not fit 53 bits either), so one addition out of order changes the last bits, and the reference is the order above
restated in numpy fp64, one rounding per addition like the kernel (the plain kernel only adds; the batched one multiplies by a per-row
factor of exactly 1.0 first).

Cases: 16 / 32 / 64 columns, fp64 and fp32 rows (fp32 widened before they are added; colw a power of two per column, x 32: exact), with
and without init (one more addition), lists of 0, 1, 7, 8, 9, 63, 64, 65 and 129 entries and the lengths around every A; the output is NaN
before the launch (fpca_debug_gather).  Measured on the MI355X: profiles/gather_shadow_ab.txt (the same data through the kernels of the
previous commit: the same bits)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_missing_gathers_cpu as M  # noqa: E402

pytestmark = pytest.mark.gpu

REACH = {1: (False, 0.0), 2: (True, 0.0)}  # (short_lists, avg_len) as K2 / K3 pass them: the plain and the batched kernel
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 129, 3, 15, 16, 17, 31, 32, 33, 127, 128, 257, 2]


def _ordered_sum(rows, b, kernel):
    """rows [n][b] fp64, in list order -> the kernel's sum of each column: partial sums, pairs, tree; every + is one fp64 rounding."""
    epw = 64 // b
    depth = 4 if kernel == 1 else 8
    part = np.zeros((depth * epw, b))
    for n in range(rows.shape[0]):
        part[n % (depth * epw)] += rows[n]
    acc = part.reshape(depth, epw, b)  # acc[a][g]: partial sum g + a EPW
    if depth == 4:
        grp = (acc[0] + acc[1]) + (acc[2] + acc[3])
    else:
        grp = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    g = epw
    while g > 1:
        g //= 2
        grp = grp[:g] + grp[g:2 * g]
    return grp[0]


def _reference(ptr, idx, V, b, kernel, rows_out, colw, init):
    ref = np.zeros((rows_out, b))
    for r in range(len(ptr) - 1):
        ref[r] = _ordered_sum(V[idx[ptr[r]:ptr[r + 1]]].astype(np.float64), b, kernel)
    if colw is not None:
        ref *= (colw * 32.0)[None, :]
    if init is not None:
        ref = init + ref
    return ref


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("b", [16, 32, 64])
def test_gather_order_of_additions(built_lib, b, kernel, f32, with_init):
    import flashpca_amd as fp

    rng = np.random.default_rng(100 * b + kernel)
    v_rows, rows_out = 777, len(LENGTHS) + 3
    ptr = np.zeros(len(LENGTHS) + 1, dtype=np.int64)
    np.cumsum(LENGTHS, out=ptr[1:])
    idx = np.concatenate([np.sort(rng.choice(v_rows, size=n, replace=False)) for n in LENGTHS]).astype(np.int64)
    V = rng.standard_normal((v_rows, b)) * np.exp2(rng.uniform(-20, 20, size=(v_rows, 1)))
    V = V.astype(np.float32) if f32 else V
    colw = 2.0 ** (np.arange(b) % 23 - 11.0) if f32 else None
    init = rng.standard_normal((rows_out, b)) if with_init else None
    short_lists, avg_len = REACH[kernel]
    assert M.gather_variant(b, False, short_lists, avg_len) == kernel
    out, variant = fp.api.debug_gather(ptr, idx, V, b, rows_out=rows_out, colw=colw, init=init, short_lists=short_lists, avg_len=avg_len)
    ref = _reference(ptr, idx, V, b, kernel, rows_out, colw, init)
    # the data does tell orders apart: the plain left-to-right sum differs from the kernel's in the last bits of most long lists
    naive = np.array([V[idx[ptr[r]:ptr[r + 1]]].astype(np.float64).sum(axis=0) if LENGTHS[r] else np.zeros(b) for r in range(len(LENGTHS))])
    unscaled = _reference(ptr, idx, V, b, kernel, len(LENGTHS), None, None)
    assert (naive != unscaled).any(axis=1).sum() >= 5
    same = bool(np.array_equal(out, ref))
    bad = np.nonzero((out != ref).any(axis=1))[0]
    print("gather order b %2d kernel %d %s init %d: %d lists, %d calls, bit-identical to the restated order %s" % (
        b, kernel, "fp32" if f32 else "fp64", with_init, len(LENGTHS), idx.size, same))
    assert variant == kernel
    assert np.isfinite(out).all(), "rows the kernel did not write: %s" % np.nonzero(~np.isfinite(out).all(axis=1))[0][:8]
    assert same, (b, kernel, "rows", bad[:8], "lengths", [LENGTHS[r] if r < len(LENGTHS) else -1 for r in bad[:8]])
