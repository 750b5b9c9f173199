"""The yardstick of the F tail's grid tests (tests/test_ucca_cpu.py: the host build through fpca_debug_f_sf; tests/test_gpu_f_tail.py:
the device build through fpca_debug_f_sf_dev): the r2 grid, the edge values, and the reference
    F = r2 / (1 - r2) (n - k - 1) / k,     P = scipy.special.betaincc(k / 2, (n - k - 1) / 2, r2),
which takes r2 itself, never a rounded 1 - r2.  scipy against mpmath at 60 digits, every eighth grid point, n in {10, 957, 500,000},
k in {1, 15, 256}: 1e-16 relative -- eight orders below the bound it is used for."""
import numpy as np
from scipy import special

R2_GRID = np.unique(np.concatenate([np.logspace(-12, -1e-4, 160), 1 - np.logspace(-12, -1, 60), np.linspace(0.005, 0.995, 100)]))
# outside (0, 1), on its ends, and the smallest subnormal / normal numbers
R2_EDGES = np.array([-1.0, 0.0, 5e-324, 2.2e-308, np.nextafter(1.0, 0.0), 1.0, 1.5, np.nan])
KS = (1, 2, 3, 10, 15, 63, 64, 255, 256)
B_F, B_P, P_FLOOR, P_UNDER = 1e-14, 1e-8, 1e-290, 1e-280


def shuffled_points(seed=20261020):
    """Grid and edges in one fixed random order: every wave of 64 lanes holds both branches of f_sf and its early returns."""
    r2 = np.concatenate([R2_GRID, R2_EDGES])
    return r2[np.random.default_rng(seed).permutation(r2.size)]


def reference(r2, n, k):
    """F and P for r2 strictly inside (0, 1)."""
    return r2 / (1 - r2) * (n - k - 1) / k, special.betaincc(k / 2.0, (n - k - 1) / 2.0, r2)


def p_errors(r2, P, n, k):
    """(mask of the points inside (0, 1) with a reference P >= 1e-290, the relative errors of P there): a figure, no assertion."""
    r2, P = np.asarray(r2), np.asarray(P)
    with np.errstate(invalid="ignore"):
        big = (r2 > 0) & (r2 < 1)
    Pe = reference(r2[big], n, k)[1]
    big[big] = Pe >= P_FLOOR
    Pe = Pe[Pe >= P_FLOOR]
    return big, np.abs(P[big] - Pe) / Pe


def check_points(r2, F, P, n, k):
    """Every r2 against the reference at the bounds of tests/test_ucca_cpu.py (inside (0, 1)) or against the edge rules of f_sf
    (elsewhere).  Returns (points with P >= 1e-290 held to 1e-8, the worst relative error of P among them)."""
    r2, F, P = np.asarray(r2), np.asarray(F), np.asarray(P)
    nan = np.isnan(r2)
    assert np.all(np.isnan(F[nan]) & np.isnan(P[nan])), (n, k)
    lo = r2 <= 0
    assert np.all((F[lo] == 0.0) & (P[lo] == 1.0)), (n, k, r2[lo], F[lo], P[lo])
    hi = r2 >= 1
    assert np.all((F[hi] == np.inf) & (P[hi] == 0.0)), (n, k, r2[hi], F[hi], P[hi])
    inside = ~(nan | lo | hi)
    x, f, p = r2[inside], F[inside], P[inside]
    Fe, Pe = reference(x, n, k)
    bad = ~(np.abs(f - Fe) <= B_F * Fe)
    assert not bad.any(), (n, k, x[bad], f[bad], Fe[bad])
    big = Pe >= P_FLOOR
    rel = np.abs(p[big] - Pe[big]) / Pe[big]
    bad = ~(rel <= B_P)
    assert not bad.any(), (n, k, x[big][bad], p[big][bad], Pe[big][bad])
    small = ~big
    assert np.all((p[small] >= 0.0) & (p[small] < P_UNDER)), (n, k, x[small], p[small], Pe[small])
    return int(big.sum()), float(rel.max()) if rel.size else 0.0
