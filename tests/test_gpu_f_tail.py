"""The DEVICE build of the F tail (csrc/f_tail.hpp as k_ucca_finish runs it) on a grid, through fpca_debug_f_sf_dev: r2 in, F and P out,
one lane per value.  fpca_ucca reaches that build only at the r2 a data set yields; here it goes through both branches of f_sf, the
small-argument and Stirling branches of neg_lbeta, down to P ~ 1e-290 and to n = k + 2, at the bounds tests/test_ucca_cpu.py sets for
the host build (tests/f_tail_yardstick.py): F to 1e-14, P to 1e-8 relative of scipy's betaincc(k/2, (n-k-1)/2, r2) wherever that is
>= 1e-290 and 0 <= P < 1e-280 below, the edge values exactly.

The values are the CPU test's R2_GRID plus {-1, 0, 5e-324, 2.2e-308, nextafter(1, 0), 1, 1.5, NaN}, shuffled with a fixed seed so that
every wave holds both branches and the early returns; their number is no multiple of 256; one launch per (n, k), k in
{1, 2, 3, 10, 15, 63, 64, 255, 256} wherever k <= n - 2.

Records (printed by every case, pytest -s; not asserted).  Worst relative error of P against scipy over the points held to 1e-8, and
the worst relative difference between the device and the host build (the library's host code), measured on the MI355X:
    n          points   device     where (k, r2, P)             host       device - host
    k + 2      2,907    1.92e-14   1, 1.68e-12, 1               1.92e-14   5.30e-16
    10           969    1.89e-14   2, 1 - 1e-12, 8.23e-39       1.89e-14   1.87e-15
    957        2,174    2.07e-13   256, 0.925, 4.43e-280        2.48e-13   2.27e-13
    500,000    1,153    3.13e-11   3, 1.04e-05, 0.156           3.13e-11   2.28e-13
    1,000,000  1,117    6.38e-11   1, 4.38e-06, 0.0364          6.38e-11   5.71e-14
The two builds differ by what their lgamma, log, log1p and exp differ by; neither comes near the bound.  The loss at large n is the method's, not the device's: the continued fraction on the I_{1 - r2}(a, b) side of the branch switch takes
the rounded 1 - r2 (f_tail.hpp's header)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_tail_yardstick as Y  # noqa: E402

pytestmark = pytest.mark.gpu

CPU_KS = (1, 2, 10, 15, 63, 256)  # what tests/test_ucca_cpu.py::test_f_tail_matches_scipy runs on the same grid


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


def f_sf_dev(fp, r2, n, k):
    r2 = np.ascontiguousarray(r2, dtype=np.float64)
    F, P = np.full(r2.size, -7.0), np.full(r2.size, -7.0)
    rc = fp.lib().fpca_debug_f_sf_dev(r2.ctypes.data, r2.size, int(n), int(k), F.ctypes.data, P.ctypes.data)
    assert rc == 0, fp.lib().fpca_last_error()
    return F, P


def f_sf_host(fp, r2, n, k):
    F, P = C.c_double(), C.c_double()
    out = np.empty(r2.size)
    for i, x in enumerate(r2):
        assert fp.lib().fpca_debug_f_sf(float(x), int(n), int(k), C.byref(F), C.byref(P)) == 0
        out[i] = P.value
    return out


@pytest.mark.parametrize("n", ["k+2", 10, 957, 500000, 1000000])
def test_device_f_tail_matches_scipy(fp, n):
    r2 = Y.shuffled_points()
    assert r2.size % 256 != 0 and r2.size == Y.R2_GRID.size + Y.R2_EDGES.size
    assert set(CPU_KS) <= set(Y.KS)  # the same grid at no fewer k: at least the points the CPU test checks
    checked, worst_dev, worst_host, worst_diff, where = 0, 0.0, 0.0, 0.0, None
    for k in Y.KS:
        nn = k + 2 if n == "k+2" else n
        if k > nn - 2:
            continue
        F, P = f_sf_dev(fp, r2, nn, k)
        c, _ = Y.check_points(r2, F, P, nn, k)
        checked += c
        big, e_dev = Y.p_errors(r2, P, nn, k)
        Ph = f_sf_host(fp, r2, nn, k)
        _, e_host = Y.p_errors(r2, Ph, nn, k)
        if e_dev.max() > worst_dev:
            i = int(np.argmax(e_dev))
            worst_dev, where = float(e_dev.max()), (k, float(r2[big][i]), float(P[big][i]))
        worst_host = max(worst_host, float(e_host.max()))
        worst_diff = max(worst_diff, float(np.max(np.abs(P[big] - Ph[big]) / Ph[big])))
        # the early returns and NaN come out of both builds alike
        with np.errstate(invalid="ignore"):
            edge = ~((r2 > 0) & (r2 < 1))
        assert np.array_equal(P[edge], Ph[edge], equal_nan=True)
    print("n = %s: %d points held to 1e-8; worst relative error against scipy: device %.2e (k = %d, r2 = %.3g, P = %.3g), host %.2e; "
          "worst device - host %.2e" % ((n, checked, worst_dev) + where + (worst_host, worst_diff)))
    assert checked > 300


def test_device_hook_refusals(fp):
    """Refused as fpca_debug_f_sf refuses; count = 0 returns at once, before any pointer is looked at."""
    r2 = np.array([0.5])
    F, P = np.zeros(1), np.zeros(1)
    call = fp.lib().fpca_debug_f_sf_dev
    assert call(r2.ctypes.data, 1, 10, 9, F.ctypes.data, P.ctypes.data) == -1  # k = n - 1
    assert "needs k >= 1, n >= k + 2" in fp.lib().fpca_last_error().decode()
    assert call(r2.ctypes.data, 1, 10, 0, F.ctypes.data, P.ctypes.data) == -1
    assert call(r2.ctypes.data, 1, 10, 1, None, P.ctypes.data) == -1
    assert call(r2.ctypes.data, 1, 10, 1, F.ctypes.data, None) == -1
    assert call(None, 1, 10, 1, F.ctypes.data, P.ctypes.data) == -1
    assert call(None, 0, 10, 1, F.ctypes.data, P.ctypes.data) == 0
    assert call(r2.ctypes.data, 1, 10, 8, F.ctypes.data, P.ctypes.data) == 0  # n = k + 2
    assert abs(P[0] - Y.reference(0.5, 10, 8)[1]) <= Y.B_P * P[0]
