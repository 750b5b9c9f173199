"""The yardstick of tests/test_i8_planes_cpu.py and tests/test_gpu_i8_planes.py: genotypes, operands and references for which every
product of the int8 GEMM path (csrc/kernels_i8.hip: k_slice, k_gemm_i8, k_i8_combine; csrc/missing_routes.hip) is an exact fp64 number,
so that the GPU comparison is np.array_equal -- with operands that live in the LOW digit planes on purpose.  Nothing here calls the library.

Genotypes (stand="binom").  k_bed_stats computes mean = (2 n00 + n10) / ngood and sd = sqrt(pp (1 - pp)), pp = mean / 2.  A SNP whose
called samples hold as many dosage-0 as dosage-2 calls has mean == 1.0 and sd == 0.5 exactly, whatever its heterozygotes: the standardised
matrix is 2 g - 2 in {-2, 0, 2}, 0 for a missing call.  Every SNP is of that kind but one monomorphic SNP (sd 0: a zero row) and, in the
sets that say so, one SNP without a call (mean and sd NaN: a zero row).  Five sets:
  D0  nothing missing                                           route 2
  D1  0 .. 3 missing calls per SNP (0.12 %)                     route 3 for b 16 / 32 / 64; routes 0 and 1 forced
  D2  5 % of the SNPs at 20 %, the others at most one           route 4 (for b 16 / 32 / 64: the list routes have no 48-column gather)
  D3  D1, one SNP without a call, dyadic mean / sd per SNP      the two-matrix kernels, mode 0 (fpca_set_meansd)
  D4  2, 3, 3 or 4 missing calls per ordinary SNP (0.424 %)     route 3 in a context of 6 .. 8 slices (b 16 / 32 / 64) -- but a pass of
                                                                that context on at most 4 slices takes the two-matrix kernels
                                                                (`pass_route`: the cheap passes' break-even is 0.35 %, not 0.5 %)
`route` is hybrid_classify / i8_mode of missing_routes.hip restated; D1's counts are what keeps it on route 3 at every S (with two or three
calls in most SNPs the per-SNP rule of the hybrid route would take the shard at S = 2 and 3: 0.12 % rather than 0.2 %).

Operands.  k_slice cuts m = rint(x 2^(F - e)), F = 8 S - 2, 2^e > the column maximum.  `x` below is the quantity that is sliced: the block B
itself for X'B; T / sd (and mean T / sd, sliced on its own) for X T, so T = x sd.
  full      (S <= 5) integers below 2^(F-1) times a power of two per column: every plane is busy at once; F - 1 <= 37 bits plus the
            summation stay under 53
  windowed  a pin pair +2^(e-1), -2^(e-1) in two adjacent rows fixes e; every other entry is n 2^(e - F + 8 j) with |n| < 2^(8 W - 3): it lives
            in the W digit planes from digit j up only.  W = 5 at S >= 6 (windows from digit 0 and from digit S - 5: every plane lies in one,
            every adjacent pair in a common one); block k gives column c window (c + k) mod 2, so two blocks put every (plane, column) pair
            to use.  W = 3 at S = 4 on the data sets with a list route: there the gathers read the fp32 rows k_slice leaves (float32(x
            2^(1-e))), which hold 24 significant bits -- the one documented approximation of the path; 21-bit entries stay inside it.
The pins cancel inside the int32 accumulators, never in fp64: the two rows are adjacent and even-aligned (one 256-row K chunk), and they
belong to two samples (X'B), two SNPs (X T) with identical genotype records and no missing call (D3: mean 1, sd 1) -- so they vanish from
the per-plane column sums too and stand in no gather list.  (The SNP without a call marks the pin samples missing: in D2 its indicator
row runs on the matrix cores, as in D3, and its output row is zero by its statistics.)
D3: mean = k / 4, k in 2 .. 6, so the second operand of X T is x k / 4: the entries are multiples of 4 units of half the magnitude.

Exactness, order-free: with t = sum_rows sum_planes |digit| 256^(plane) in units of the column's lowest occupied plane (pins apart:
`order_free_total`), every partial sum the kernels form is a multiple of a quarter unit: the G.M sums are below 8 t quarter units, the M
sums below 4 t, mean x the M sums below 6 t (mean <= 1.5), and the combine's (G.M sum) - mean (M sum) below 14 t in D3, 4 t under binom
(mean 1).  tests/test_i8_planes_cpu.py asserts 14 t < 2^53 for D3 and 8 t < 2^53 elsewhere: then every partial of any split, in any order, is
exact.  The reference is int64 arithmetic on the integer operands (`int_matmul`, `reference`).

The GPU cases are listed here too (`child_runs`): the small shape 701 x 523 everywhere, and 2301 x 2099 for the child that needs whole rounds
of tiles AND eight or more K chunks, without which the plan never splits a phase B."""
import functools

import numpy as np

import i8_slice_yardstick as Y

N, P = 701, 523            # N mod 4 = 1: pad bits in the last byte; N_pad 1024 = 4 K chunks / row tiles, P_pad 768 = 3
N_TALL, P_TALL = 2301, 2099  # N_pad 2560: ten 256-row tiles and ten K chunks; P_pad 2304: nine of each -- enough chunks to split
PIN_SAMPLE, PIN_SNP = 300, 270   # the pin rows r, r + 1 (r even: the same 16-row group, the same 256-row chunk)
MONO_SNP, NOCALL_SNP = 5, 400
CODE = {2: 0, "missing": 1, 1: 2, 0: 3}  # dosage -> raw 2-bit code
D_CELL, G_CALL, M2_CELL, SPARSE_BREAK_EVEN = 1.96e-15, 2.0e-12, 1.45e-15, 0.005  # missing_routes.hip
CHEAP_SPARSE_BREAK_EVEN = 0.0035                                                 # ... and the cheap passes' own break-even
LIST_SETS = ("D1", "D2", "D4")  # the sets whose own route has index lists: at <= 4 slices the gathers read fp32 rows


# ---- genotypes ---------------------------------------------------------------------------------------------------------------------------
def _balanced_row(rng, n, called):
    """Raw codes of one SNP: the samples of `called` (bool [n]) hold equally many dosage-0 and dosage-2 calls; the pin samples share one
    genotype."""
    row = np.full(n, CODE["missing"], dtype=np.uint8)
    assert called[PIN_SAMPLE] and called[PIN_SAMPLE + 1]
    gp = int(rng.integers(0, 3))
    rest = np.flatnonzero(called)
    rest = rest[(rest != PIN_SAMPLE) & (rest != PIN_SAMPLE + 1)]
    d = {0: 2, 1: 0, 2: -2}[gp]                      # dosage-2 minus dosage-0 calls the other samples owe
    r = rest.size
    nhet = int(rng.integers(0, max(1, r // 2)))
    if (r - nhet - abs(d)) % 2:
        nhet += 1
    n0 = (r - nhet - d) // 2
    n2 = n0 + d
    assert n0 >= 0 and n2 >= 0 and n0 + n2 + nhet == r
    g = np.concatenate([np.zeros(n0, int), np.full(n2, 2), np.ones(nhet, int)])
    rng.shuffle(g)
    lut = np.array([CODE[0], CODE[1], CODE[2]], dtype=np.uint8)
    row[rest] = lut[g]
    row[PIN_SAMPLE] = row[PIN_SAMPLE + 1] = lut[gp]
    return row


@functools.lru_cache(maxsize=None)
def genotypes(name, n=N, p=P):
    """codes [p][n] uint8 (raw: 0 dosage 2, 1 missing, 2 dosage 1, 3 dosage 0) of data set D0 .. D4."""
    rng = np.random.default_rng({"D0": 11, "D1": 12, "D2": 13, "D3": 12, "D4": 14}[name] + 1000 * n)
    nmiss = np.zeros(p, dtype=int)
    if name in ("D1", "D3"):
        c2, c3 = p * 30 // 523, p * 13 // 523
        c1 = p * 330 // 523
        counts = np.array([0] * (p - c1 - c2 - c3) + [1] * c1 + [2] * c2 + [3] * c3)
        nmiss = rng.permutation(counts)
    elif name == "D2":
        nmiss = (rng.random(p) < 0.5).astype(int)
        ordinary = np.setdiff1d(np.arange(p), [MONO_SNP, PIN_SNP, PIN_SNP + 1, NOCALL_SNP])
        nmiss[rng.choice(ordinary, size=p // 20, replace=False)] = n // 5
    elif name == "D4":
        ordinary = np.setdiff1d(np.arange(p), [MONO_SNP, PIN_SNP, PIN_SNP + 1, NOCALL_SNP])
        nmiss[ordinary] = rng.permutation(np.resize([2, 3, 3, 4], ordinary.size))
    nmiss[[MONO_SNP, PIN_SNP, PIN_SNP + 1, NOCALL_SNP]] = 0
    free = np.setdiff1d(np.arange(n), [PIN_SAMPLE, PIN_SAMPLE + 1])
    codes = np.empty((p, n), dtype=np.uint8)
    for j in range(p):
        called = np.ones(n, dtype=bool)
        called[rng.choice(free, size=nmiss[j], replace=False)] = False
        codes[j] = _balanced_row(rng, n, called)
    codes[PIN_SNP + 1] = codes[PIN_SNP]
    codes[MONO_SNP] = CODE[2]
    if name in ("D2", "D3"):
        codes[NOCALL_SNP] = CODE["missing"]
    codes.setflags(write=False)
    return codes


def pack(codes):
    """The SNP-major 2-bit stream: sample 4 i + s in bits 2 s .. 2 s + 1 of byte i; the pad bits of the last byte are 00 (a dosage-2 call
    if anything read them)."""
    p, n = codes.shape
    c = np.zeros((p, (n + 3) // 4 * 4), dtype=np.uint8)
    c[:, :n] = codes
    c = c.reshape(p, -1, 4)
    return np.ascontiguousarray(c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).reshape(-1)


def dosage_called(codes):
    """GM [p][n] int64 (dosage, 0 where missing) and M (1 where called)."""
    GM = np.where(codes == 0, 2, np.where(codes == 2, 1, 0)).astype(np.int64)
    return GM, (codes != 1).astype(np.int64)


def bed_stats(codes):
    """mean, sd by the formulas of k_bed_stats (stand 'binom'), in its order of operations."""
    n00, n10, n11 = ((codes == c).sum(axis=1).astype(np.float64) for c in (0, 2, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (2 * n00 + n10) / (n00 + n10 + n11)
        pp = mean / 2.0
        sd = np.sqrt(pp * (1 - pp))
    return mean, sd


@functools.lru_cache(maxsize=None)
def meansd(name, n=N, p=P):
    """[p][2] mean, sd as the context holds them: K1's for D0 .. D2, the dyadic values installed with set_meansd for D3."""
    if name != "D3":
        return np.stack(bed_stats(genotypes(name, n, p)), axis=1)
    j = np.arange(p)
    ms = np.stack([np.array([0.5, 0.75, 1.0, 1.25, 1.5])[j % 5], np.array([0.25, 0.5, 1.0, 2.0, 4.0])[(j // 5) % 5]], axis=1)
    ms[[PIN_SNP, PIN_SNP + 1]] = 1.0, 1.0
    ms[MONO_SNP, 1] = 0.0
    return ms


def live_snps(ms):
    return ms[:, 1] > 1e-9  # (False for NaN too: the kernels' own test)


@functools.lru_cache(maxsize=None)
def quarter_matrix(name, n=N, p=P):
    """A [p][n] int64 = called (4 g - 4 mean), zero rows for the SNPs the kernels zero: X = A / (4 sd)."""
    GM, M = dosage_called(genotypes(name, n, p))
    ms = meansd(name, n, p)
    live = live_snps(ms)
    k4 = np.where(live, 4 * np.where(live, ms[:, 0], 0), 0)
    assert np.array_equal(k4, np.rint(k4))
    A = (4 * GM - k4.astype(np.int64)[:, None] * M) * live[:, None]
    A.setflags(write=False)
    return A


def route(nmiss, n, S, b):
    """fpca_missing_mode of an unforced context: i8_mode + hybrid_classify of missing_routes.hip."""
    nmiss = np.asarray(nmiss, dtype=np.int64)
    total, p = int(nmiss.sum()), nmiss.size
    if total == 0:
        return 2
    lists_ok = b in (16, 32, 64)
    if lists_ok:
        thr = D_CELL * S / G_CALL * n
        dense = nmiss > thr
        rest = total - int(nmiss[dense].sum())
        if dense.any():
            ch = G_CALL * rest + D_CELL * n * S * int(dense.sum())
            if ch < M2_CELL * n * S * p and ch < 0.85 * G_CALL * total:
                return 4
    rate = total / (n * p)
    if lists_ok and rate <= SPARSE_BREAK_EVEN:
        return 3
    return 1 if rate < 3e-4 else 0


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def operand_kind(name, S):
    """'full', or the window width W: see the module docstring."""
    if S >= 6:
        return 5
    if S == 4 and name in LIST_SETS:
        return 3  # the list routes read fp32 rows at S <= 4: 24 significant bits
    return "full"


def window_digits(S, W):
    """The lowest digit of each window (digit i has weight 256^i; plane s holds digit S - 1 - s)."""
    offs = list(range(0, S - W, W - 1)) + [S - W]
    assert all(b - a <= W - 1 for a, b in zip(offs, offs[1:]))  # adjacent planes share a window
    return offs


class Operand:
    """x [rows][b] fp64, exact under slicing at S: x = n 2^unit per column, n int64; pin: the first pin row or None; e: the exponents
    k_slice must find; planes [S][b] bool: the planes column c is meant to use."""


def operand(S, b, rows, pin, kind, block, quarter=False, seed=0):
    """Block `block` (0 / 1: the window rotation) of the operand family (S, b, rows, kind).  quarter (D3): entries are multiples of 4 units
    below half the magnitude, so that x k / 4, k <= 6, is of the same kind (and stays below the pins)."""
    rng = np.random.default_rng([S, b, rows, block, seed, 77])
    F = 8 * S - 2
    o = Operand()
    o.S, o.b, o.rows, o.kind, o.block = S, b, rows, kind, block
    ecol = rng.integers(-60, 61, size=b)  # a wide range of column scales
    q = 4 if quarter else 1
    if kind == "full":
        bits = F - 1 - (3 if quarter else 0)
        n = rng.integers(-(2 ** bits) + 1, 2 ** bits, size=(rows, b), dtype=np.int64) * q
        n[pin + 2 + np.arange(b) % 5, np.arange(b)] = (2 ** bits - 1) * q  # every column reaches its top bit (in a row that counts)
        top = np.abs(n).max(axis=0)
        o.n, o.unit, o.pin = n, ecol.astype(np.int64), None
        o.e = o.unit + np.array([int(t).bit_length() for t in top])
        o.planes = np.ones((S, b), dtype=bool)
        o.digit0 = np.zeros(b, dtype=np.int64)
    else:
        W = kind
        offs = window_digits(S, W)
        j = np.array([offs[(c + block) % len(offs)] for c in range(b)])
        bits = 8 * W - 3 - (3 if quarter else 0)
        n = rng.integers(-(2 ** bits) + 1, 2 ** bits, size=(rows, b), dtype=np.int64) * q
        n[[pin, pin + 1]] = 0
        o.n, o.unit, o.pin = n, (ecol - F + 8 * j).astype(np.int64), pin
        o.e = ecol.astype(np.int64)
        o.planes = np.zeros((S, b), dtype=bool)
        for c in range(b):
            o.planes[S - 1 - (j[c] + W - 1):S - j[c], c] = True
        o.digit0 = j
    o.x = np.ldexp(o.n.astype(np.float64), o.unit[None, :].astype(np.int32))
    if o.pin is not None:
        o.x[pin] = np.ldexp(1.0, (o.e - 1).astype(np.int32))
        o.x[pin + 1] = -o.x[pin]
    assert np.all(np.abs(o.n) < 2 ** 53)
    return o


def case_operand(name, S, b, op, block, n=N, p=P):
    """The operand of one GPU case: op 'xt' (X'B: rows = samples) or 'x' (X T: rows = SNPs)."""
    rows, pin = (n, PIN_SAMPLE) if op == "xt" else (p, PIN_SNP)
    return operand(S, b, rows, pin, operand_kind(name, S), block, quarter=(name == "D3"), seed={"xt": 1, "x": 2}[op])


def host_block(name, o, op, n=N, p=P):
    """What the caller passes: B = x for X'B; T = x sd for X T (x / 2 where the kernels' row scale is zero anyway)."""
    if op == "xt":
        return o.x
    ms = meansd(name, n, p)
    sd = np.where(live_snps(ms), ms[:, 1], 0.5)
    return o.x * sd[:, None]


def k3_operands(name, T, n=N, p=P):
    """The two operands k_slice cuts for X T, by k_i8_rowscales' arithmetic: T / sd and mean T / sd."""
    ms = meansd(name, n, p)
    live = live_snps(ms)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.where(live, 1.0 / ms[:, 1], 0.0)
        mu = np.where(live, ms[:, 0] / ms[:, 1], 0.0)
    return T * inv[:, None], T * mu[:, None]


# ---- references --------------------------------------------------------------------------------------------------------------------------
def int_matmul(A, n):
    """A @ n in int64 for |A| <= 8, |n| < 2^60 and at most 2^20 rows, through three 20-bit limbs of n: every limb product is an integer
    below 8 x 2^20 x 2^20 = 2^43, exact in fp64 in any order, so the BLAS product IS the integer product; the limbs are recombined in int64.
    (Plain `A @ n` on int64 arrays gives the same numbers -- tests/test_i8_planes_cpu.py compares the two -- a hundred times slower.)"""
    assert np.max(np.abs(A)) <= 8 and A.shape[1] <= 2 ** 20 and np.max(np.abs(n)) < 2 ** 60
    Af = A.astype(np.float64)
    R = np.zeros((A.shape[0], n.shape[1]), dtype=np.int64)
    rest = n.astype(np.int64)
    for k in range(3):
        limb = rest & (2 ** 20 - 1) if k < 2 else rest  # low limbs in [0, 2^20), the last one signed (|.| < 2^20)
        rest = rest >> 20
        R += (Af @ limb.astype(np.float64)).astype(np.int64) << (20 * k)
    return R


def reference(name, o, op, n=N, p=P):
    """The exact product in fp64 from int64 sums: X'B = (A n) 2^(unit - 2) / sd, X T = (A' n) 2^(unit - 2)."""
    A = quarter_matrix(name, n, p)
    nn = o.n  # (the pins are two equal rows of A times +-2^(e-1): they cancel in the integers as in the int32 accumulators)
    if o.pin is not None:
        cols = A[:, [o.pin, o.pin + 1]] if op == "xt" else A[[o.pin, o.pin + 1]].T
        assert np.array_equal(cols[:, 0], cols[:, 1])
    R = int_matmul(A if op == "xt" else A.T, nn)
    assert np.max(np.abs(R)) < 2 ** 53
    out = np.ldexp(R.astype(np.float64), (o.unit - 2)[None, :].astype(np.int32))
    if op == "xt":
        ms = meansd(name, n, p)
        live = live_snps(ms)
        out = np.where(live[:, None], out / np.where(live, ms[:, 1], 1.0)[:, None], 0.0)
    return out


class PlaneProducts:
    """The digit-level model: the per-plane integer products of both matrices (exact in fp64: |sum| <= 2 x 128 x rows) and the weights,
    recombined as the kernels do -- sum_s w_s (integer matrix x plane s) -- with optional mutations of one plane."""

    def __init__(self, name, x, op, S, n=N, p=P):
        GM, M = dosage_called(genotypes(name, n, p))
        self.name, self.op, self.S, self.n, self.p = name, op, S, n, p
        b = x.shape[1]
        if op == "xt":
            s = Y.Sliced(x, x.shape[0], S, S * b)
            self.sl = (s, s)
            mats = (GM.astype(np.float64), M.astype(np.float64))
        else:
            T = host_block(name, _AsOperand(x), "x", n, p)
            xg, xm = k3_operands(name, T, n, p)
            self.sl = (Y.Sliced(xg, xg.shape[0], S, S * b), Y.Sliced(xm, xm.shape[0], S, S * b))
            mats = (GM.T.astype(np.float64), M.T.astype(np.float64))
        self.prod = [np.stack([mat @ sl.D[s].astype(np.float64) for s in range(S)]) for mat, sl in zip(mats, self.sl)]
        assert max(np.max(np.abs(q)) for q in self.prod) < 2 ** 31  # what the int32 accumulators hold
        self.w = [sl.colw[:S * b].reshape(S, b).copy() for sl in self.sl]

    def output(self, mutation=None, s=None):
        """mutation: None, 'zero' (plane s dropped), 'weight' (its weight times 256) or 'swap' (planes s and s + 1 exchanged)."""
        acc = []
        for prod, w in zip(self.prod, self.w):
            order = list(range(self.S))
            scale = np.ones(self.S)
            if mutation == "zero":
                scale[s] = 0.0
            elif mutation == "weight":
                scale[s] = 256.0
            elif mutation == "swap":
                order[s], order[s + 1] = order[s + 1], order[s]
            acc.append(sum(w[t][None, :] * scale[t] * prod[order[t]] for t in range(self.S)))
        g, m = acc
        if self.op == "x":
            return g - m
        ms = meansd(self.name, self.n, self.p)
        live = live_snps(ms)
        mean, sd = np.where(live, ms[:, 0], 0.0)[:, None], np.where(live, ms[:, 1], 1.0)[:, None]
        return np.where(live[:, None], (g - mean * m) / sd, 0.0)


class _AsOperand:
    def __init__(self, x):
        self.x = x


def order_free_total(sl, pin):
    """Per column: sum over rows (pins apart) and planes of |digit| 256^(digit index - lowest occupied digit index), as Python ints."""
    D = sl.D.astype(np.int64).copy()  # [S][rows][b], D[0] the top digit
    if pin is not None:
        D[:, [pin, pin + 1]] = 0
    S = D.shape[0]
    tot = []
    for c in range(D.shape[2]):
        used = [i for i in range(S) if np.any(D[S - 1 - i, :, c])]
        if not used:
            tot.append(0)
            continue
        tot.append(sum(int(np.abs(D[S - 1 - i, :, c]).sum()) * 256 ** (i - used[0]) for i in used))
    return tot


# ---- the GPU cases (tests/test_gpu_i8_planes.py runs them, tests/test_i8_planes_cpu.py checks their data) -----------------------------
WIDTHS = (16, 32, 48, 64)


def _runs(names_modes, S_list, b_list, tiled_list=(None, 0), tall=False):
    out = []
    for S in S_list:
        for tiled in tiled_list:
            for name, modes in names_modes:
                for mode in modes:
                    for b in b_list:
                        if mode is None and name in ("D1", "D2") and b == 48:
                            continue  # (the list routes have gather kernels for 16 / 32 / 64 columns)
                        out.append(dict(ds=name, S=S, b=b, tiled=tiled, mode=mode, tall=tall))
    return out


def child_runs(child):
    """The runs of one child process: dicts ds, S, b, tiled (None / 0), mode (None = the context's own route / forced), tall."""
    if child.startswith("main"):  # "mainS": every width on every route at S slices
        return _runs((("D0", (None,)), ("D1", (None, 0, 1)), ("D2", (None,)), ("D3", (0,))), (int(child[4:]),), WIDTHS)
    if child == "splits4":
        return _runs((("D0", (None,)), ("D1", (0,))), (3, 7, 8), (16, 64), (None,))
    if child == "rows512":
        return [r for r in _runs((("D0", (None,)), ("D1", (None,))), (2, 4, 7), (16, 32)) if (r["b"], r["S"]) in ((16, 4), (16, 7), (32, 2))]
    if child == "ncu24":
        return _runs((("D0", (None,)), ("D1", (0,))), (7,), (16, 32, 64), (None,), tall=True)
    raise KeyError(child)


CHILDREN = ["main%d" % S for S in range(2, 9)] + ["splits4", "rows512", "ncu24"]
CHILD_ENV = {"splits4": {"FPCA_I8_SPLITS": "4"}, "rows512": {"FPCA_I8_ROWS": "512"}, "ncu24": {"FPCA_I8_NCU": "24"}}


def dims(tall):
    return (N_TALL, P_TALL) if tall else (N, P)


def run_id(run):
    return "%s-S%d-b%d-%s-m%s%s" % (run["ds"], run["S"], run["b"], "tl" if run["tiled"] is None else "rm", "d" if run["mode"] is None else run["mode"],
                                    "-tall" if run["tall"] else "")


def expected_mode(run):
    n, p = dims(run["tall"])
    if run["mode"] is not None:
        return run["mode"]
    GM, M = dosage_called(genotypes(run["ds"], n, p))
    return route((M == 0).sum(axis=1), n, run["S"], run["b"])


def data_keys():
    """Every (ds, S, b, op, tall) whose operands some GPU case multiplies (a pass on Sc slices multiplies the operands made for Sc)."""
    keys = set()
    for child in CHILDREN:
        for r in child_runs(child):
            for op in ("xt", "x"):
                keys.add((r["ds"], r["S"], r["b"], op, r["tall"]))
    for child in CHEAP_CHILDREN:
        for r in cheap_runs(child):
            for op in ("xt", "x"):
                keys.add((r["ds"], r["Sc"], r["b"], op, r["tall"]))
    return sorted(keys)


# ---- passes on fewer slices than the context holds (tests/test_gpu_i8_cheap_passes.py; checked by tests/test_i8_planes_cpu.py) ----------
# The eigensolver's cheap passes run K2 and K3 on Sc < S slices inside the context made for S (fpca_ctx::i8_Sc), exact passes between
# them.  A run here is dict(ds, S = the context's slices, Sc = the slices of this pass, b, tiled, mode, tall, q = its place in the
# context's sequence); Sc == S is an exact pass.  Its operand is case_operand(ds, Sc, ...), its reference that operand's: neither
# depends on S.
@functools.lru_cache(maxsize=None)
def nmiss_of(name, n=N, p=P):
    return (dosage_called(genotypes(name, n, p))[1] == 0).sum(axis=1)


def pass_route(nmiss, n, S_ctx, Sc, b):
    """The route of ONE pass: `route` of the context, but a pass on at most 4 slices of a context that holds more leaves the lists for
    the two-matrix kernels above the cheap passes' own break-even (i8_mode of missing_routes.hip, its last rule before I8M_SPARSE).  The
    cost model of the hybrid classification keeps the context's slice count."""
    nmiss = np.asarray(nmiss, dtype=np.int64)
    r = route(nmiss, n, S_ctx, b)
    if r == 3 and Sc < S_ctx and Sc <= 4 and int(nmiss.sum()) / (n * nmiss.size) > CHEAP_SPARSE_BREAK_EVEN:
        return 0
    return r


CHEAP_CHILDREN = {"cheap7": (7, (None, 0)), "cheap8": (8, (None,)), "cheap6": (6, (None,))}  # child -> context slices, layouts
CHEAP_SETS = (("D0", None), ("D1", None), ("D2", None), ("D4", None), ("D3", 0))
# The default layout: the pass is the outer loop -- (slices, the width the pass starts at; the widths go round from there).
PASSES = {7: ((7, 16), (4, 16), (7, 16), (3, 16), (6, 32), (4, 16), (5, 16), (2, 16), (7, 16)),
          8: ((8, 16), (3, 16), (5, 16), (4, 16), (8, 32), (2, 16), (7, 16), (8, 16)),
          6: ((6, 16), (4, 16), (5, 16), (3, 16), (6, 32), (2, 16), (6, 16))}
# FPCA_I8_TILED=0: the width is the outer loop -- (width, the passes at it); shortened.
PASSES_RM = {7: ((16, (7, 4, 6)), (32, (3, 7, 5)), (48, (5,)), (64, (5, 2, 7)))}


def pass_sequence(S_ctx, tiled, ds):
    """[(Sc, b)] one context runs, in order."""
    widths = [b for b in WIDTHS if not (b == 48 and ds in LIST_SETS)]  # (the list routes have gather kernels for 16 / 32 / 64 columns)
    if tiled is not None:
        return [(Sc, b) for b, scs in PASSES_RM[S_ctx] if b in widths for Sc in scs]
    seq = []
    for Sc, b0 in PASSES[S_ctx]:
        k = widths.index(b0)
        seq += [(Sc, b) for b in widths[k:] + widths[:k]]
    return seq


def cheap_runs(child):
    """The runs of a child of tests/test_gpu_i8_cheap_passes.py; consecutive runs of one (ds, tiled) share one context."""
    S_ctx, layouts = CHEAP_CHILDREN[child]
    return [dict(ds=ds, S=S_ctx, Sc=Sc, b=b, tiled=tiled, mode=mode, tall=False, q=q)
            for tiled in layouts for ds, mode in CHEAP_SETS for q, (Sc, b) in enumerate(pass_sequence(S_ctx, tiled, ds))]


def pass_run_id(run):
    return "%s-S%d-%s-m%s-q%02d-c%d-b%d" % (run["ds"], run["S"], "tl" if run["tiled"] is None else "rm", "d" if run["mode"] is None else run["mode"],
                                            run["q"], run["Sc"], run["b"])


def expected_pass_modes(run):
    """(what fpca_missing_mode answers: the exact passes' route; the route of this pass)."""
    if run["mode"] is not None:
        return run["mode"], run["mode"]
    n, p = dims(run["tall"])
    nm = nmiss_of(run["ds"], n, p)
    return route(nm, n, run["S"], run["b"]), pass_route(nm, n, run["S"], run["Sc"], run["b"])


# The witness.  The operands of a pass on Sc slices are exact at Sc, hence exact at S too: a hook that changed nothing would pass every
# comparison.  So every run and product applies one more block:
#   Sc < S   block 0 with a quarter of the Sc quantum, 2^(e_c - F_Sc - 2), taken off the magnitude of a few entries (added to a zero).
#            On Sc slices the quarter rounds away -- m = rint(m0 -+ 1/4) = m0, the column maximum and with it e_c are untouched -- so
#            the result equals block 0's bit for bit; on the context's S slices (8 (S - Sc) more bits) the quarter is a digit.
#   Sc == S  block 0 on a grid three bits finer, n' = 8 n + w at unit - 3, w = 1 in the witness entries of the columns whose window
#            starts above digit 0 (there unit - 3 is still on the S grid): exact at S, compared with its own int64 reference, and
#            different from block 0's.  (That an exact pass runs on no FEWER slices needs no witness: from S = 6 on every block has a
#            window from digit 0.)
# The entries lie in rows no gather reads -- the gathers read the UNROUNDED operand (fp64 rows, fp32 rows at <= 4 slices), where a
# quarter would survive: samples without a missing call in any listed SNP (X'B), SNPs without a missing call (X T) -- whose matrix rows
# count (live, no pin, and not the rows that hold a full operand's maxima).  An entry is used only where fp64 holds the sum exactly (a
# large entry of a high window and a quarter 56 bits below e_c do not fit).  D3 is left out: its second operand x k / 4 breaks the grid.
WITNESS_SETS = ("D0", "D1", "D2", "D4")
WITNESS_ROWS = 3


@functools.lru_cache(maxsize=None)
def witness_rows(name, op, n=N, p=P):
    codes = genotypes(name, n, p)
    called = codes != CODE["missing"]
    nmiss = (~called).sum(axis=1)
    if op == "x":
        ok = (nmiss == 0) & live_snps(meansd(name, n, p))
        pin = PIN_SNP
    else:  # (SNPs missing in more than a tenth of the samples ride the matrix cores on the hybrid route -- rounded slices -- or are dead)
        ok = called[nmiss <= n // 10].all(axis=0)
        pin = PIN_SAMPLE
    ok[pin:pin + 7] = False
    rows = np.flatnonzero(ok)[:WITNESS_ROWS]
    assert rows.size >= 1
    return rows


def witness_operand(name, S_ctx, Sc, b, op, n=N, p=P):
    """The witness block of a run (an Operand; .witnessed [rows][b] bool: the entries that carry it, rows = witness_rows)."""
    o = case_operand(name, Sc, b, op, 0, n, p)
    rows = witness_rows(name, op, n, p)
    w = Operand()
    w.__dict__.update(o.__dict__)
    if Sc < S_ctx:
        d = np.ldexp(1.0, (o.e - (8 * Sc - 2) - 2).astype(np.int32))[None, :]
        old = o.x[rows]
        step = np.where(old > 0, -d, d)  # towards zero: no magnitude grows, the maximum least of all
        new = old + step
        w.witnessed = (new - old == step) & (np.abs(new) > 0)  # (exact in fp64, or the entry is left alone)
        w.x = o.x.copy()
        w.x[rows] = np.where(w.witnessed, new, old)
        w.n = None  # (no integer form at Sc: never compared with a reference of its own)
    else:
        assert o.pin is not None
        w.witnessed = np.broadcast_to(o.digit0 >= 1, (rows.size, b)).copy()
        w.n = 8 * o.n
        w.n[rows] += w.witnessed
        w.unit = o.unit - 3
        w.x = np.ldexp(w.n.astype(np.float64), w.unit[None, :].astype(np.int32))
        w.x[o.pin], w.x[o.pin + 1] = o.x[o.pin], o.x[o.pin + 1]
    return w


def total_in_units(sl, pin, unit):
    """Per column: sum over rows (pins apart) and planes of |digit| 256^i 2^(e - F) in units of 2^unit, as Python ints; asserts that every
    digit's term is a whole number of units (`order_free_total` measured in the operand's own unit, not in that of its lowest plane)."""
    D = sl.D.astype(np.int64).copy()
    if pin is not None:
        D[:, [pin, pin + 1]] = 0
    S = D.shape[0]
    tot = []
    for c in range(D.shape[2]):
        t = 0
        for i in range(S):
            col = D[S - 1 - i, :, c]
            if not col.any():
                continue
            sh = 8 * i + int(sl.e[c]) - sl.F - int(unit[c])  # this plane's weight is 2^sh units
            if sh < 0:
                assert not (col & ((1 << -sh) - 1)).any(), (c, i, sh)
                t += int(np.abs(col).sum()) >> -sh
            else:
                t += int(np.abs(col).sum()) << sh
        tot.append(t)
    return tot


# The chained product, Y = X X' B as the solver runs it (apply_xxt_dev -> xt_i8(chain) -> x_i8(have_max)): the K2 combine leaves the column
# maxima of the two K3 operands, which are then cut on the pass's slices -- and DO round at 4 and 3 slices.  The reference restates the
# path instead of tolerating it.  B = integers below 2^CHAIN_BITS = 2^22 times a power of two per column (`chain_block`): K2 is exact at
# every slice count from 3 (F = 22) and so are the fp32 rows of its gathers, T = X'B in int64.  T / sd and mean T / sd are cut by the slicer's own model at Sc slices with the exponents of their own column
# maxima; on the list routes the indicator term reads the rows the contract leaves for the gathers -- the unrounded operand, in fp32 at
# <= 4 slices (24 significant bits) -- and on the hybrid route the dense SNPs' rows are cut on their own.  Y in int64 from those.
CHAIN_PASSES = (7, 4, 7, 3, 7)
CHAIN_SETS = ("D0", "D1", "D2", "D4")
CHAIN_WIDTHS = (16, 32, 64)
CHAIN_BITS = 22
CHAIN_S = 7


def chain_runs():
    return [dict(ds=ds, S=CHAIN_S, Sc=Sc, b=b, tiled=None, mode=None, tall=False, q=q)
            for ds in CHAIN_SETS for q, (Sc, b) in enumerate((Sc, b) for Sc in CHAIN_PASSES for b in CHAIN_WIDTHS)]


@functools.lru_cache(maxsize=None)
def chain_block(name, b, k, n=N, p=P):
    """Block k (0 / 1) of the chained product's input on data set `name`: .n int64 [n][b], .unit [b], .x = n 2^unit.  Column c leans on
    one SNP j of the set, n = 3 x 2^20 (g_j - 1) + 20 random bits, so that row j of X'B is about 4 x 3 x 2^20 x (600 homozygotes) > 2^32
    units while the other rows stay near 2^27: the column maximum then puts the quantum of a 4-slice pass at 8 units, and T / sd, a
    multiple of 4, rounds.  (With entries below 2^20 the largest |A n| is 4 x 701 x 2^20 < 2^32: nothing could round at 4 slices.)"""
    rng = np.random.default_rng([b, k, n, 99])
    codes = genotypes(name, n, p)
    GM, M = dosage_called(codes)
    hom = ((GM != 1) & (M == 1)).sum(axis=1) * live_snps(meansd(name, n, p))
    hom[[PIN_SNP, PIN_SNP + 1]] = 0
    lean = np.argsort(-hom, kind="stable")[2 * np.arange(b) + k]
    o = Operand()
    o.b, o.unit = b, rng.integers(-60, 61, size=b).astype(np.int64)
    o.n = 3 * 2 ** 20 * ((GM[lean] - 1) * M[lean]).T + rng.integers(-(2 ** 20) + 1, 2 ** 20, size=(n, b), dtype=np.int64)
    assert np.abs(o.n).max() < 2 ** CHAIN_BITS
    o.x = np.ldexp(o.n.astype(np.float64), o.unit[None, :].astype(np.int32))
    o.x.setflags(write=False)
    return o


def hybrid_dense(nmiss, n, S_ctx):
    """The SNPs whose indicator rows the hybrid route sends to the matrix cores (hybrid_classify)."""
    return np.asarray(nmiss) > D_CELL * S_ctx / G_CALL * n


class ChainModel:
    """Y [n][b] fp64 and what the exactness bounds need: .T, .units (the unit every term of K3 is a whole multiple of), .ops = the
    Sliced K3 operands (T / sd, mean T / sd, and the dense SNPs' rows of the latter on the hybrid route), .gathered = per column the sum
    of |rows the gathers may add| in units, .route."""


def _to_units(v, unit):
    """fp64 -> int64 in units of 2^unit per column, asserted exact."""
    y = np.ldexp(v, (-unit)[None, :].astype(np.int32))
    r = np.rint(y)
    assert np.array_equal(r, y) and np.max(np.abs(r), initial=0) < 2 ** 60
    return r.astype(np.int64)


def _dequant(sl):
    mf = sl.m.astype(np.float64)
    assert np.array_equal(mf.astype(np.int64), sl.m)
    return np.ldexp(mf, (sl.e - sl.F)[None, :].astype(np.int32))


def chain_model(name, blk, S_ctx, Sc, n=N, p=P):
    b = blk.b
    GM, M = dosage_called(genotypes(name, n, p))
    E = 1 - M
    ms = meansd(name, n, p)
    live = live_snps(ms)
    nmiss = nmiss_of(name, n, p)
    c = ChainModel()
    c.route = pass_route(nmiss, n, S_ctx, Sc, b)
    # K2, exact: T = (A n) 2^(unit - 2) / sd
    R = int_matmul(quarter_matrix(name, n, p), blk.n)
    assert np.max(np.abs(R)) < 2 ** 53
    T = np.ldexp(R.astype(np.float64), (blk.unit - 2)[None, :].astype(np.int32))
    c.T = np.where(live[:, None], T / np.where(live, ms[:, 1], 1.0)[:, None], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = np.where(live, 1.0 / ms[:, 1], 0.0)
        mu = np.where(live, ms[:, 0] / ms[:, 1], 0.0)
    slg, slm = Y.Sliced(c.T, p, Sc, Sc * b, rowscale=inv), Y.Sliced(c.T, p, Sc, Sc * b, rowscale=mu)
    c.ops = [slg, slm]
    c.units = units = blk.unit  # (binom: sd 1/2, mean 1 -- T / sd = (A n) 2^unit; rounding to slices or to fp32 only coarsens the grid)
    Xg, Xm = _to_units(_dequant(slg), units), _to_units(_dequant(slm), units)
    # the rows the gathers read: the unrounded second operand, through fp32 at <= 4 slices
    rows = slm.x if Sc > 4 else np.ldexp(slm.slice_copy32().astype(np.float64), (slm.e - 1)[None, :].astype(np.int32))
    Cp = _to_units(rows, units)
    c.gathered = [0] * b
    if c.route == 2:
        assert not E.any()
        Eterm = 0
    elif c.route in (0, 1):  # the two-matrix kernels: the indicator meets the digits
        Eterm = int_matmul(E.T, Xm)
    else:
        dense = hybrid_dense(nmiss, n, S_ctx) if c.route == 4 else np.zeros(p, dtype=bool)
        Eterm = int_matmul(E[~dense].T, Cp[~dense])
        c.gathered = [int(v) for v in np.abs(Cp[~dense]).sum(axis=0)]
        if dense.any():  # their rows of mean T / sd, cut on their own with their own column maxima
            sld = Y.Sliced(np.ascontiguousarray(slm.x[dense]), int(dense.sum()), Sc, Sc * b)
            c.ops.append(sld)
            Eterm = Eterm + int_matmul(E[dense].T, _to_units(_dequant(sld), units))
    Yi = int_matmul(GM.T, Xg) - (Xm.sum(axis=0)[None, :] - Eterm)
    assert np.max(np.abs(Yi)) < 2 ** 53
    c.Y = np.ldexp(Yi.astype(np.float64), units[None, :].astype(np.int32))
    return c
