"""The yardstick of tests/test_qc_cpu.py and tests/test_gpu_qc.py: include/fpca.h "Genotype census" restated in numpy on the unpacked raw
2-bit codes.  Nothing here calls the feature.
  counts      comparisons of the (P, N) code matrix with 0 .. 3, summed along one axis under a boolean mask
  HWE         hwe_fractions: the exact test in rational arithmetic straight from the multinomial weights n! 2^h / (hr! h! hc!) -- not the
              recurrence; hwe_longdouble: the recurrence of the header in 80-bit arithmetic, vectorised over the SNPs, which also returns
              how close any term of a SNP comes (relative) to the tie boundary w(a) (1 + 2^-20)
  rules       --mind and --geno / --maf / --hwe as array expressions"""
import os
from fractions import Fraction
from math import factorial

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILESETS = ("hapmap3_data", "data_chr1", "hm3_thinned", "kg_thinned")
LD = np.longdouble
TIE = LD(1) + LD(2) ** -20


def pack_codes(codes):
    """codes: (P, N) raw PLINK 2-bit codes -> the packed records."""
    P, N = codes.shape
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    return (c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)).astype(np.uint8)


def unpack_codes(packed, N, P):
    packed = np.asarray(packed, dtype=np.uint8).reshape(P, -1)
    return np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(P, -1)[:, :N]


_codes = {}


def golden_codes(name):
    """(codes (P, N), N, P) of a golden fileset, read once."""
    if name not in _codes:
        prefix = os.path.join(GOLD, name)
        N = open(prefix + ".fam", "rb").read().count(b"\n")
        raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:]
        P = raw.size // ((N + 3) // 4)
        c = unpack_codes(raw, N, P)
        c.setflags(write=False)
        _codes[name] = (c, N, P)
    return _codes[name]


def snp_counts(codes, samples=None):
    """(P, 4) uint32 by raw code over the samples of the boolean mask (None: all)."""
    sub = codes if samples is None else codes[:, np.asarray(samples, dtype=bool)]
    return np.stack([(sub == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)


def sample_counts(codes, snps=None):
    """(N, 4) uint32 by raw code over the SNPs of the boolean mask (None: all)."""
    sub = codes if snps is None else codes[np.asarray(snps, dtype=bool)]
    return np.stack([(sub == c).sum(axis=0) for c in range(4)], axis=1).astype(np.uint32)


# ---- HWE -------------------------------------------------------------------------------------------------------------
def hwe_fractions(c0, c2, c3):
    """The exact p-value as a Fraction, from the weights of the possible heterozygote counts themselves."""
    a, b, c = c2, min(c0, c3), max(c0, c3)
    n, r = a + b + c, 2 * min(c0, c3) + c2
    if n == 0:
        return Fraction(1)
    w = {}
    for h in range(r % 2, r + 1, 2):
        hr = (r - h) // 2
        hc = n - h - hr
        w[h] = Fraction(factorial(n) * 2 ** h, factorial(hr) * factorial(h) * factorial(hc))
    thr = w[a] * (1 + Fraction(1, 2 ** 20))
    return min(Fraction(1), sum(v for v in w.values() if v <= thr) / sum(w.values()))


def _walk(w, h, stop, r, n, down, visit):
    """Advances the walks w (longdouble), h (int64) of all SNPs in place, downwards or upwards, while stop(h) allows; visit(idx, w[idx])
    sees every new term."""
    while True:
        idx = np.flatnonzero(stop(h))
        if idx.size == 0:
            return
        hh = h[idx]
        hr = (r[idx] - hh) // 2
        hc = n[idx] - hh - hr
        if down:
            num, den = (hh * (hh - 1)).astype(LD), (4 * (hr + 1) * (hc + 1)).astype(LD)
            h[idx] = hh - 2
        else:
            num, den = (4 * hr * hc).astype(LD), ((hh + 2) * (hh + 1)).astype(LD)
            h[idx] = hh + 2
        w[idx] = w[idx] * num / den
        if visit is not None:
            visit(idx, w[idx])


def hwe_longdouble(counts):
    """(p as longdouble, the smallest relative distance of any term from the tie boundary) per row of counts (n, 4): the recurrence of
    include/fpca.h, steps 1 - 8, in 80-bit arithmetic."""
    cnt = np.asarray(counts).astype(np.int64)
    a, b, c = cnt[:, 2], np.minimum(cnt[:, 0], cnt[:, 3]), np.maximum(cnt[:, 0], cnt[:, 3])
    n = a + b + c
    r = 2 * b + a
    mid = r * (2 * n - r) // np.maximum(2 * n, 1)
    mid = mid + ((mid ^ r) & 1)
    m = len(n)
    # w(a): the walk from mid to a
    wa, h = np.ones(m, dtype=LD), mid.copy()
    _walk(wa, h, lambda hh: hh > a, r, n, True, None)
    _walk(wa, h, lambda hh: hh < a, r, n, False, None)
    thr = wa * TIE
    tot, tail = np.ones(m, dtype=LD), (1 <= thr).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.abs(LD(1) / thr - 1)

    def visit(idx, w):
        tot[idx] += w
        tail[idx] += np.where(w <= thr[idx], w, LD(0))
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.abs(w / thr[idx] - 1)
        margin[idx] = np.minimum(margin[idx], np.where(np.isnan(d), np.inf, d))

    w, h = np.ones(m, dtype=LD), mid.copy()
    _walk(w, h, lambda hh: hh >= 2, r, n, True, visit)
    w, h = np.ones(m, dtype=LD), mid.copy()
    _walk(w, h, lambda hh: hh <= r - 2, r, n, False, visit)
    p = np.minimum(LD(1), tail / tot)
    p[n == 0] = 1
    margin[n == 0] = np.inf
    return p, margin


def hwe_bound_ok(p, p_ref, counts):
    """The bound of the issue: |p - p_ref| <= 8 n 2^-53 p_ref where p_ref >= 1e-280, 0 <= p <= 1e-279 below; never NaN, never above 1.
    Returns (ok per row, the largest error in units of n 2^-53 p_ref among the rows with p_ref >= 1e-280)."""
    cnt = np.asarray(counts).astype(np.int64)
    n = (cnt[:, 0] + cnt[:, 2] + cnt[:, 3]).astype(LD)
    p = np.asarray(p, dtype=np.float64)
    big = p_ref >= LD("1e-280")
    err = np.abs(p.astype(LD) - p_ref)
    ok = np.where(big, err <= 8 * n * LD(2) ** -53 * p_ref, (p >= 0) & (p <= 1e-279))
    ok &= ~np.isnan(p) & (p <= 1.0) & (p >= 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        units = np.where(big & (n > 0), err / (n * LD(2) ** -53 * p_ref), 0)
    return ok, float(units.max()) if units.size else 0.0


# ---- rules -----------------------------------------------------------------------------------------------------------
def sample_rule(counts, n_snps, mind, samples):
    """--mind on (N, 4) counts: dropped when counts[:, 1] / n_snps > mind (mind >= 1: off); an entry that is False stays False."""
    out = np.asarray(samples, dtype=bool).copy()
    if mind < 1:
        out &= ~(counts[:, 1].astype(np.float64) / np.float64(n_snps) > mind)
    return out


def snp_rule(counts, n, maf, geno, hwe, p_hwe, keep):
    """--geno / --maf / --hwe on (P, 4) counts taken over n samples; p_hwe is read only when hwe > 0."""
    c = counts.astype(np.int64)
    out = np.asarray(keep, dtype=bool).copy()
    if maf > 0:
        ngood = c[:, 0] + c[:, 2] + c[:, 3]
        with np.errstate(invalid="ignore", divide="ignore"):
            p = ((2 * c[:, 0] + c[:, 2]).astype(np.float64) / ngood.astype(np.float64)) / 2.0
            f = np.where(ngood == 0, 0.0, np.minimum(p, 1.0 - p))
        out &= ~(f < maf)
    if geno < 1:
        out &= ~(c[:, 1].astype(np.float64) / np.float64(n) > geno)
    if hwe > 0:
        out &= ~(np.asarray(p_hwe) < hwe)
    return out
