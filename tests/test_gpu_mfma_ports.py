"""The operand-port patterns of the bare int8 MFMA stream (fpca_debug_mfma_peak, patterns 12..17): every one runs and answers
a plausible rate.  No rate is compared with another here: which port costs more is a measurement (scripts/mfma_i8_peak.py,
profiles/mfma_ports_ab.txt), not a test.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 20000


@pytest.fixture(scope="module")
def lib(built_lib):
    import flashpca_amd

    return flashpca_amd.lib()


def _rate(lib, waves, pattern):
    t = C.c_double(float("nan"))
    return lib.fpca_debug_mfma_peak(waves, ITERS, pattern, C.byref(t)), t.value


@pytest.mark.parametrize("waves", [1, 2])
@pytest.mark.parametrize("pattern", [12, 13, 14, 15, 16, 17])
def test_port_pattern_answers(lib, pattern, waves):
    """A finite rate between 100 and 5,100 TOP/s: the stream ran on the whole chip and was timed (no pattern of the probe has ever
    been measured outside 2,500 .. 4,700), and no rate above the card's dense int8 peak is reported."""
    rc, tops = _rate(lib, waves, pattern)
    assert rc == 0
    assert math.isfinite(tops) and 100.0 < tops < 5100.0, tops


@pytest.mark.parametrize("pattern", [10, 11])
def test_old_patterns_still_answer(lib, pattern):
    rc, tops = _rate(lib, 1, pattern)
    assert rc == 0
    assert math.isfinite(tops) and 100.0 < tops < 5100.0, tops


@pytest.mark.parametrize("pattern", [4, 9, 18, -1])
def test_unknown_pattern_is_refused(lib, pattern):
    rc, tops = _rate(lib, 2, pattern)
    assert rc != 0
    assert math.isnan(tops)  # nothing was written


def _ports(lib, shape, exchanged, A, Bt):
    D = np.full((shape, shape), -1, dtype=np.int32)
    rc = lib.fpca_debug_mfma_i8_ports(shape, exchanged, A.ctypes.data_as(C.c_void_p), Bt.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return D


@pytest.mark.parametrize("shape", [32, 16])
def test_exchanged_operands_give_the_transposed_tile(lib, shape):
    """k_gemm_i8 issues mfma(slice-columns, genotypes): through the register map of mfma(A, B) the same registers hold (A B')', exactly,
    for v_mfma_i32_32x32x32_i8 and for the v_mfma_i32_16x16x64_i8 of the 16-column remainder (asymmetric operands, full int8 range)."""
    rng = np.random.default_rng(100 + shape)
    k = 1024 // shape
    A = rng.integers(-128, 128, size=(shape, k), dtype=np.int8)
    Bt = rng.integers(-128, 128, size=(shape, k), dtype=np.int8)
    ref = A.astype(np.int32) @ Bt.astype(np.int32).T
    assert not np.array_equal(ref, ref.T)
    plain = _ports(lib, shape, 0, A, Bt)
    assert np.array_equal(plain, ref)
    if shape == 32:  # the existing probe
        D = np.zeros((32, 32), dtype=np.int32)
        assert lib.fpca_debug_mfma_i8_probe(A.ctypes.data_as(C.c_void_p), Bt.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(D, plain)
    assert np.array_equal(_ports(lib, shape, 1, A, Bt), plain.T)


def test_ports_probe_refuses_other_shapes(lib):
    z = np.zeros(1024, dtype=np.int8)
    D = np.zeros(1024, dtype=np.int32)
    assert lib.fpca_debug_mfma_i8_ports(8, 0, z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p)) != 0
