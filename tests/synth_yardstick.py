"""A replica of the synthetic genotype model, written from the description in flashpca_amd/csrc/synth.hpp and include/fpca.h.

It is the yardstick that tests/test_synth_cpu.py holds the library's host generator (fpca_debug_synth_host) to and that
tests/test_gpu_synth.py holds the device generator (k_synth_generate, behind Context.synthetic) to, byte for byte.  It calls nothing of
the library.  It is built differently from the generators on purpose:

  * everything that exists once per SNP -- the ancestral frequency, the population frequencies, the missing-call threshold, the
    square root, the cubic for 2^f, the population boundaries -- is arithmetic on Python integers (arbitrary precision, `>>` floors,
    math.isqrt), so no C integer width, overflow or shift rule is shared with the code under test;
  * the 64-bit hash is numpy uint64 arithmetic (which wraps like the C type) over whole arrays of SNPs or samples;
  * a sample's population comes from numpy.searchsorted over the boundaries, not from the kernel's binary search on the first
    sample of a word followed by a walk;
  * a record is packed from a code per sample, four to a byte, with the pad samples of the last byte at code 01; there are no
    32-bit words, no pitch and no 256-thread sweep here;
  * the five integers a model's doubles are reduced to are computed here with exact half-away-from-zero rounding (what llround
    does), through fractions.

The arguments that describe a model have the names and defaults of flashpca_amd.Context.synthetic.
"""
import functools
import math
from fractions import Fraction

import numpy as np

DEFAULT_SEED = 20260928  # Context.synthetic's
M64 = (1 << 64) - 1
_U = np.uint64


# ---- the counter-based hash -----------------------------------------------------------------------------------------------------
def _mix64(x):
    x = x ^ (x >> _U(30))
    x = x * _U(0xBF58476D1CE4E5B9)
    x = x ^ (x >> _U(27))
    x = x * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def rnd64(seed, stream, snp, idx):
    """64 random bits per (snp, idx); seed and stream are Python integers, snp and idx anything that broadcasts to uint64 arrays."""
    snp = np.atleast_1d(np.asarray(snp, dtype=np.uint64))
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    x0 = _U((seed * 0x9E3779B97F4A7C15 + stream * 0xD1B54A32D192ED03) & M64)
    with np.errstate(over="ignore"):
        x = _mix64(x0 ^ (snp * _U(0xC2B2AE3D27D4EB4F) + _U(0x165667B19E3779F9)))
        return _mix64(x ^ (idx * _U(0x9FB21C651E98DF25) + _U(0x2545F4914F6CDD1D)))


def _ints(a):
    """A numpy integer array as (nested) lists of Python integers."""
    return a.tolist()


def _sum4(h):
    """The four 16-bit fields of a hash word, summed (Python integer)."""
    return (h & 0xFFFF) + ((h >> 16) & 0xFFFF) + ((h >> 32) & 0xFFFF) + (h >> 48)


def _irwin_hall(h3):
    """Twelve 16-bit uniforms from three hash words, recentred: mean 0, sd 1.0 in 16.16."""
    return _sum4(h3[0]) + _sum4(h3[1]) + _sum4(h3[2]) - 6 * 65535


# ---- the model's doubles -> the five integers -----------------------------------------------------------------------------------
def llround(x):
    """Round a double to the nearest integer, halves away from zero, exactly."""
    f = Fraction(x)
    n = math.floor(abs(f) + Fraction(1, 2))
    return n if f >= 0 else -n


class Model:
    def __init__(self, n_pop=40, fst=0.05, missing_rate=0.001, realistic=False, maf_model=None, missing_model=None, conc_frac=0.05,
                 lognormal_sigma=0.0):
        self.n_pop = n_pop
        self.maf_model = int(realistic if maf_model is None else maf_model)
        self.missing_model = int(realistic if missing_model is None else missing_model)
        sig = lognormal_sigma if self.missing_model == 2 else 0.0
        self.fst_fp = llround(fst * 65536.0)                  # 16.16
        self.miss_thr = llround(missing_rate * 65536.0)       # a 16-bit uniform below it is a missing call
        self.conc_fp = llround(conc_frac * 65536.0)
        # the median that gives the asked-for mean, 0.32 fixed point, at most 0.9; sigma as an exponent of two, 16.16
        self.med_q32 = llround(min(missing_rate * math.exp(-0.5 * sig * sig), 0.9) * 4294967296.0)
        self.sig2_fp = llround(sig / math.log(2.0) * 65536.0)

    def fixed(self):
        return dict(fst_fp=self.fst_fp, miss_thr=self.miss_thr, conc_fp=self.conc_fp, med_q32=self.med_q32, sig2_fp=self.sig2_fp)


# ---- per SNP: Python integers ---------------------------------------------------------------------------------------------------
def lognormal_exponent(seed, snps, sig2_fp):
    """(e, f) per SNP: the rate of missing_model 2 is median * 2^(e + f / 65536), e an integer, 0 <= f < 65536."""
    h = _ints(rnd64(seed, 5, np.asarray(snps, dtype=np.uint64)[:, None], np.arange(3)[None, :]))
    out = []
    for h3 in h:
        x = (sig2_fp * _irwin_hall(h3)) >> 16  # the exponent in 16.16, floored
        out.append((x >> 16, x & 0xFFFF))
    return out


def _two_to_f(f):
    """2^(f / 65536) in 16.16 by the header's cubic, whose coefficients sum to 65536: exact at both ends."""
    return 65536 + ((f * (45426 + ((f * (15743 + ((f * 4367) >> 16))) >> 16))) >> 16)


class Thresholds:
    """What the model fixes per SNP before a cell is drawn, as integer arrays over the SNPs asked for:
    pj (P,) ancestral frequency 16.16; pop (P, n_pop) population frequencies = thresholds for 16-bit uniforms; miss (P,) threshold of
    the missing call; e (P,) the integer exponent of the log-normal rate (missing_model 2, else None); pick (P,) the 16-bit uniform
    that is compared with conc_fp (missing_model 1, else None)."""


def thresholds(P, snp_begin=0, seed=DEFAULT_SEED, **model):
    m = Model(**model)
    snps = np.array([snp_begin + r for r in range(P)], dtype=np.uint64)
    t = Thresholds()
    t.model, t.e, t.pick = m, None, None
    # ancestral frequency: 0.05 + 0.90 u (uniform model), 0.001 + 0.499 u^3 (rare-variant spectrum); u = the top 16 bits
    pj = []
    for h in _ints(rnd64(seed, 1, snps, 0)):
        u = h >> 48
        if m.maf_model == 1:
            u3 = (((u * u) >> 16) * u) >> 16
            pj.append(66 + ((u3 * 32702) >> 16))
        else:
            pj.append(3277 + ((u * 58982) >> 16))
    # missing-call threshold
    if m.missing_model == 1:  # conc_frac of the SNPs at 10-30 %, every other SNP at most 0.1 %
        miss, pick = [], []
        for h in _ints(rnd64(seed, 4, snps, 0)):
            pk, lvl = h & 0xFFFF, (h >> 16) & 0xFFFF
            pick.append(pk)
            miss.append(6554 + ((lvl * 13107) >> 16) if pk < m.conc_fp else (lvl * 66) >> 16)
        t.pick = np.array(pick, dtype=np.int64)
    elif m.missing_model == 2:  # median * 2^(sigma / ln 2 * z), capped at 90 %
        miss, es = [], []
        for e, f in lognormal_exponent(seed, snps, m.sig2_fp):
            rate = (m.med_q32 * _two_to_f(f)) >> 16  # 0.32
            # synth.hpp saturates the rate at e >= 20 whatever the median is -- a median of 0 included, where the formula gives 0:
            # the header's code is the specification, so this follows it.  (Its other branch, 0 at e <= -40, is what the shift
            # gives anyway: rate < 2^33.)
            rate = M64 if e >= 20 else rate << e if e >= 0 else rate >> -e
            miss.append(min(rate >> 16, 58982))
            es.append(e)
        t.e = np.array(es, dtype=np.int64)
    else:
        miss = [m.miss_thr] * P
    # population frequencies: p_j + sqrt(fst p_j (1 - p_j)) z_jc, clamped to [0.01 (0.0001 for a rare ancestral frequency), 0.99]
    hp = _ints(rnd64(seed, 2, snps[:, None], np.arange(4 * m.n_pop)[None, :]))
    pop = []
    for p, hrow in zip(pj, hp):
        sd = math.isqrt((m.fst_fp * p * (65536 - p)) >> 16)  # 16.16
        lo = 7 if p < 3277 else 655
        pop.append([min(max(p + ((sd * _irwin_hall(hrow[4 * c:4 * c + 3])) >> 16), lo), 64880) for c in range(m.n_pop)])
    t.pj = np.array(pj, dtype=np.int64)
    t.pop = np.array(pop, dtype=np.int64).reshape(P, m.n_pop)
    t.miss = np.array(miss, dtype=np.int64)
    return t


def boundaries(N, n_pop):
    """First sample of population c, c = 0 .. n_pop: the weight of population c is c + 1."""
    tot = n_pop * (n_pop + 1) // 2
    return [(N * (c * (c + 1) // 2)) // tot for c in range(n_pop + 1)]


def population_of(N, n_pop):
    """The population of every sample: the number of inner boundaries at or below it."""
    inner = np.array(boundaries(N, n_pop)[1:n_pop], dtype=np.int64)
    return np.searchsorted(inner, np.arange(N, dtype=np.int64), side="right")


# ---- per cell: numpy ------------------------------------------------------------------------------------------------------------
def record_codes(N, seed, snp, pop_thr, miss_thr, pop):
    """The PLINK code of every sample of one SNP: 01 missing, else by dosage g = [u1 < p] + [u2 < p]: 2 -> 00, 1 -> 10, 0 -> 11."""
    h = rnd64(seed, 3, snp, np.arange(N, dtype=np.uint64))
    u1, u2, u3 = h & _U(0xFFFF), (h >> _U(16)) & _U(0xFFFF), (h >> _U(32)) & _U(0xFFFF)
    p = np.asarray(pop_thr, dtype=np.uint64)[pop]
    g = (u1 < p).astype(np.int64) + (u2 < p).astype(np.int64)
    code = np.array([3, 2, 0], dtype=np.uint8)[g]
    code[u3 < _U(miss_thr)] = 1
    return code


def pack(codes):
    """Codes of one record -> bytes: sample 4 i + s in bits 2 s, 2 s + 1 of byte i; pad samples are code 01."""
    n = (len(codes) + 3) // 4
    full = np.ones(4 * n, dtype=np.uint8)
    full[:len(codes)] = codes
    q = full.reshape(n, 4)
    return q[:, 0] | (q[:, 1] << 2) | (q[:, 2] << 4) | (q[:, 3] << 6)


def unpack(packed, N):
    """(P, ceil(N / 4)) bytes -> (P, N) codes."""
    packed = np.asarray(packed, dtype=np.uint8)
    return np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(packed.shape[0], -1)[:, :N]


def generate(N, P, snp_begin=0, seed=DEFAULT_SEED, **model):
    """Records [snp_begin, snp_begin + P) of the matrix: uint8 (P, (N + 3) // 4)."""
    t = thresholds(P, snp_begin, seed, **model)
    pop = population_of(N, t.model.n_pop)
    out = np.empty((P, (N + 3) // 4), dtype=np.uint8)
    for r in range(P):
        out[r] = pack(record_codes(N, seed, snp_begin + r, t.pop[r], int(t.miss[r]), pop))
    return out


# ---- the SNPs that take the rare branches of the log-normal rate ----------------------------------------------------------------
BRANCH_SIGMA, BRANCH_LIMIT = 4.0, 200000


@functools.lru_cache(maxsize=None)
def lognormal_branch_snps(seed=DEFAULT_SEED):
    """At sigma = 4, the API's largest: the first SNP indices below BRANCH_LIMIT whose exponent e is >= 20 (the rate saturates) and
    whose e is -3 .. -1 (the rate is shifted down, and BRANCH_MODELS' high mean still leaves a threshold above zero), as (saturating,
    negative); None where there is none."""
    sig2 = Model(missing_model=2, lognormal_sigma=BRANCH_SIGMA).sig2_fp
    sat = neg = None
    for j0 in range(0, BRANCH_LIMIT, 20000):
        for j, (e, _) in enumerate(lognormal_exponent(seed, np.arange(j0, j0 + 20000), sig2), j0):
            if sat is None and e >= 20:
                sat = j
            if neg is None and -3 <= e < 0:
                neg = j
        if sat is not None and neg is not None:
            break
    return sat, neg


# ---- the cases both generators are held to (tests/test_synth_cpu.py: the host entry; tests/test_gpu_synth.py: the kernel) --------
# every maf_model x missing_model, fst 0 / 0.05 / 0.99, missing_rate 0 / 0.001 / 0.5 / 0.999, conc_frac 0 / 0.05 / 1, sigma 0 / 1.5 / 4
MODELS = [
    dict(fst=0.05, missing_rate=0.001),
    dict(realistic=True, conc_frac=0.05),
    dict(missing_model=2, missing_rate=0.02, lognormal_sigma=1.5),
    dict(maf_model=1, missing_model=2, missing_rate=0.5, lognormal_sigma=4.0, fst=0.99),
    dict(missing_model=1, conc_frac=1.0, fst=0.0),
    dict(maf_model=1, missing_rate=0.999),
    dict(missing_model=2, missing_rate=0.0, lognormal_sigma=0.0),
    dict(missing_model=1, conc_frac=0.0, missing_rate=0.5),
    dict(missing_rate=0.5, fst=0.99),
    dict(missing_model=2, missing_rate=0.001, lognormal_sigma=0.0, fst=0.0),
    dict(missing_rate=0.0, fst=0.0),
]
# the kernel writes one 32-bit word (16 samples) per thread and sweeps 256 threads: 4,096 samples a sweep
N_EDGES = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8209)


def _grid():
    cases = []

    def add(tag, N, P, snp_begin=0, seed=DEFAULT_SEED, **kw):
        cases.append((tag, dict(N=N, P=P, snp_begin=snp_begin, seed=seed, **kw)))

    for i, N in enumerate(N_EDGES):  # sample counts around the byte, the word, the wave, the sweep; three populations
        add("N%d-m%d" % (N, i % len(MODELS)), N, 12, n_pop=3, **MODELS[i % len(MODELS)])
    for i, N in enumerate((4095, 4096, 4097, 8209)):  # the same with boundaries of 40 populations in both sweeps
        add("N%d-pop40-m%d" % (N, i + 1), N, 6, n_pop=40, **MODELS[i + 1])
    for i, n_pop in enumerate((1, 2, 3, 12, 40, 64)):
        add("pop%d-N513-m%d" % (n_pop, i), 513, 12, n_pop=n_pop, **MODELS[i])
        add("pop%d-N4097-m%d" % (n_pop, i + 5), 4097, 4, n_pop=n_pop, **MODELS[(i + 5) % len(MODELS)])
    add("pop64-N5-empty-populations", 5, 16, n_pop=64, fst=0.99, missing_rate=0.001)
    add("pop2-N1-empty-population", 1, 16, n_pop=2, fst=0.99, missing_rate=0.0)
    add("pop64-N63-empty-population", 63, 16, n_pop=64, fst=0.99, missing_rate=0.001)
    add("pop7-N100-boundaries-inside-words", 100, 64, n_pop=7, fst=0.99, missing_rate=0.001)
    add("pop7-N100-realistic", 100, 16, n_pop=7, realistic=True, fst=0.99)
    for i, b in enumerate((0, 300, (1 << 32) + 5)):
        for j in (0, 1, 2):
            add("begin%d-m%d" % (b, (i + 3 * j) % len(MODELS)), 65, 8, snp_begin=b, n_pop=12, **MODELS[(i + 3 * j) % len(MODELS)])
    for i, s in enumerate((DEFAULT_SEED, 0, M64)):
        for j in (0, 1, 2):
            add("seed%d-m%d" % (s, j), 513, 8, seed=s, snp_begin=300 * i, n_pop=12, **MODELS[j])
    for i, kw in enumerate(MODELS):  # every model at a shape with boundaries inside words and a second sweep
        add("m%d-N100-pop7" % i, 100, 16, n_pop=7, **kw)
        add("m%d-N4097-pop12" % i, 4097, 4, n_pop=12, **kw)
    return cases


GRID = _grid()
# sigma = 4 at the SNPs of lognormal_branch_snps, P = 1 each: a high mean, and a mean of zero (where the saturating SNP still loses
# 90 % of its calls, see thresholds())
BRANCH_MODELS = [dict(n_pop=3, missing_model=2, missing_rate=0.5, lognormal_sigma=BRANCH_SIGMA),
                 dict(n_pop=3, missing_model=2, missing_rate=0.0, lognormal_sigma=BRANCH_SIGMA)]
