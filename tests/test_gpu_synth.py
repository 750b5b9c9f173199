"""The device generator of the synthetic matrix (k_synth_generate, csrc/kernels.hip, behind Context.synthetic) against the replica of
tests/synth_yardstick.py, byte for byte.  Every speed figure of the project is taken on a matrix this kernel writes; the replica is
written from the description in csrc/synth.hpp, not from the kernel (its header says how), and tests/test_synth_cpu.py holds the
library's host generator to the same replica on the same cases, so a difference here is the kernel loop's: the population search, the
word and pad handling, the choice of the threshold, the SNP index.

The kernel writes one 32-bit word (16 samples) per thread and sweeps 256 threads, 4,096 samples a sweep; the cases of
synth_yardstick.GRID sit around the byte, the word, the wave and the sweep, put population boundaries inside words, leave populations
empty, and take SNP indices beyond 2^32.  P <= 64 everywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


def device(fp, N, P, snp_begin=0, seed=Y.DEFAULT_SEED, **kw):
    with fp.Context.synthetic(N, P, snp_begin=snp_begin, seed=seed, **kw) as ctx:
        assert (ctx.N, ctx.P) == (N, P)
        return ctx.download_packed().reshape(P, (N + 3) // 4)


def replica(N, P, snp_begin=0, seed=Y.DEFAULT_SEED, **kw):
    """The replica's records as fpca_download_packed hands records out: the pad samples of the last byte, 01 in the resident matrix
    (and in the replica), are written as 00, as PLINK writes them.  What the device holds there, and up to the pitch, shows in
    test_pitch_padding_is_all_missing_codes."""
    want = Y.generate(N, P, snp_begin, seed, **kw)
    if N % 4:
        want[:, -1] &= (1 << (2 * (N % 4))) - 1
    return want


def differences(got, want, N):
    """For the assertion message: how many cells differ, and the first few as (record, sample, device code, replica code)."""
    a, b = Y.unpack(got, 4 * got.shape[1]), Y.unpack(want, 4 * want.shape[1])  # (pad samples of the last byte included)
    r, s = np.nonzero(a != b)
    return "%d cells differ (N = %d), first (record, sample, device, replica): %s" % (len(r), N, [(int(i), int(j), int(a[i, j]), int(b[i, j])) for i, j in zip(r[:6], s[:6])])


@pytest.mark.parametrize("case", [c for _, c in Y.GRID], ids=[t for t, _ in Y.GRID])
def test_device_generator_equals_the_replica(case, fp):
    got, want = device(fp, **case), replica(**case)
    assert np.array_equal(got, want), differences(got, want, case["N"])


@pytest.mark.parametrize("model", range(len(Y.BRANCH_MODELS)))
def test_lognormal_branches_on_the_device(model, fp):
    """sigma = 4 at the SNP indices where the exponent of the log-normal rate is >= 20 (saturation) and where it is negative
    (tests/test_synth_cpu.py::test_lognormal_branches_are_reached_and_agree finds them), one record each."""
    sat, neg = Y.lognormal_branch_snps()
    m = Y.BRANCH_MODELS[model]
    assert Y.thresholds(1, sat, **m).e[0] >= 20 and Y.thresholds(1, neg, **m).e[0] < 0
    for j in (sat, neg):
        got, want = device(fp, 513, 1, snp_begin=j, **m), replica(513, 1, j, **m)
        assert np.array_equal(got, want), (j, differences(got, want, 513))


@pytest.mark.parametrize("begin", [0, (1 << 32) - 20])
def test_three_shards_concatenate_to_the_whole(begin, fp):
    """Any SNP range of the matrix can be generated on its own (include/fpca.h): three uneven shards, one of them across SNP index
    2^32, against the whole and against the replica; 40 populations, two sweeps."""
    N, P, kw = 4097, 50, dict(n_pop=40, missing_model=2, missing_rate=0.02, lognormal_sigma=1.5)
    whole = device(fp, N, P, snp_begin=begin, **kw)
    parts = [device(fp, N, n, snp_begin=begin + b, **kw) for b, n in ((0, 7), (7, 30), (37, 13))]
    assert np.array_equal(np.concatenate(parts), whole)
    want = replica(N, P, begin, **kw)
    assert np.array_equal(whole, want), differences(whole, want, N)


def test_old_entry_is_the_model_entry_with_zeroed_knobs(fp):
    """fpca_create_synthetic(n_pop, fst, missing_rate) = fpca_create_synthetic_model with maf_model = missing_model = 0."""
    N, P, begin, seed = 513, 24, 300, 5
    h = C.c_void_p()
    fp.api.check(fp.lib().fpca_create_synthetic(C.byref(h), N, begin, P, seed, 12, 0.05, 0.001, 3, 0, 64))
    with fp.Context(h, "fp64") as ctx:
        old = ctx.download_packed().reshape(P, -1)
    new = device(fp, N, P, snp_begin=begin, seed=seed, n_pop=12, fst=0.05, missing_rate=0.001, maf_model=0, missing_model=0, conc_frac=0.0)
    assert np.array_equal(old, new)
    want = replica(N, P, begin, seed, n_pop=12, fst=0.05, missing_rate=0.001)
    assert np.array_equal(old, want), differences(old, want, N)


def test_matrix_does_not_depend_on_standardisation_or_arithmetic(fp):
    N, P, kw = 4097, 16, dict(n_pop=12, realistic=True)
    want = replica(N, P, 300, **kw)
    for stand in ("binom", "binom2"):
        for accum in ("fp64", "auto", "i8x4"):
            got = device(fp, N, P, snp_begin=300, stand=stand, accum=accum, **kw)
            assert np.array_equal(got, want), (stand, accum, differences(got, want, N))


@pytest.mark.parametrize("N", [1, 3, 6, 17, 513, 4094, 4097])
def test_pitch_padding_is_all_missing_codes(N, fp):
    """The pad samples of a record's last byte and the bytes from there to the pitch never leave the device (fpca_download_packed
    clears the former and skips the latter), but K1 counts the 01 codes of the whole padded record and takes the pad samples off
    again, and the LD totals do the same: fpca_snp_missing equals the replica's count of code 01 among the N samples only if every pad
    sample up to the pitch is 01."""
    P = 32
    for kw in (dict(n_pop=1, missing_rate=0.0), dict(n_pop=min(N, 3), missing_rate=0.5), dict(n_pop=1, missing_model=1, conc_frac=0.5)):
        with fp.Context.synthetic(N, P, **kw) as ctx:
            got = ctx.snp_missing()
            packed = ctx.download_packed().reshape(P, -1)
        want = replica(N, P, **kw)
        assert np.array_equal(packed, want), differences(packed, want, N)
        assert np.array_equal(got, (Y.unpack(want, N) == 1).sum(axis=1)), (N, kw, got, (Y.unpack(want, N) == 1).sum(axis=1))
