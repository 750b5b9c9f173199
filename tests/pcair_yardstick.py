"""numpy / plain-Python restatements for the PC-AiR tests (tests/test_pcair_cpu.py, tests/test_gpu_pcair.py), written from the text of
include/fpca.h and never calling the feature: the two-population pedigree data, the census of related and divergent pairs from a phi
matrix, and the partition rule as a loop that also records which tie-break decided each removal."""
import numpy as np


def pcair_codes(N, P, seed, F=0.1):
    """(P, N) raw codes: the pedigree of tests/test_gpu_king.py (pedigree_codes) over TWO Balding-Nichols populations with F = 0.1 -- the
    first 3N/5 samples in population A, the others in B.  The same planted trio, sibs and duplicates (one at index N - 1, one copy with
    missing calls), one cross-population child (sample 12, of 11 in A and N - 2 in B), the all-homozygous sample 9, the no-call sample 44,
    and the same missing-call pattern by 32-sample block."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, P)
    a, b = p * (1 - F) / F, (1 - p) * (1 - F) / F
    pa, pb = rng.beta(a, b), rng.beta(a, b)
    nA = 3 * N // 5
    freq = np.where(np.arange(N)[:, None] < nA, pa[None, :], pb[None, :])
    d = rng.binomial(2, freq)  # founders everywhere first

    def child(u, v):
        return rng.binomial(1, d[u] / 2.0) + rng.binomial(1, d[v] / 2.0)

    d[2], d[3] = child(0, 1), child(0, 1)
    d[40], d[41] = child(33, 36), child(33, 36)
    d[12] = child(11, N - 2)                   # one parent in each population
    d[5] = d[4]
    d[N - 1] = d[6]
    d[48] = d[7]
    d[9] = 2 * rng.binomial(1, pa)
    codes = np.array([3, 2, 0], dtype=np.uint8)[d]  # (N, P)
    s = np.arange(N)
    odd = (s // 32) % 2 == 1
    rate = np.where(odd & (s % 4 == 0), 0.01, 0.0)
    rate = np.where(odd & (s % 8 == 4), 0.20, rate)
    codes[rng.random((N, P)) < rate[:, None]] = 1
    codes[44] = 1
    return np.ascontiguousarray(codes.T), dict(nA=nA, nocall=44, hom=9, rate=rate, cross=(11, 12, N - 2))


def classes_numpy(phi, kin_thr, div_thr, keep=None, exclude=None):
    """(related, divergent, nan): three boolean N x N matrices over the pairs i < j (strict upper triangle) of the kept samples.  related:
    phi > kin_thr; divergent: phi < div_thr and not related and not in `exclude` ((i, j) arrays, either order); NaN is neither."""
    N = phi.shape[0]
    k = np.ones(N, dtype=bool) if keep is None else np.asarray(keep) != 0
    among = np.triu(k[:, None] & k[None, :], 1)
    with np.errstate(invalid="ignore"):
        rel = (phi > kin_thr) & among
        div = (phi < div_thr) & ~rel & among
    if exclude is not None:
        ex = np.zeros((N, N), dtype=bool)
        ei, ej = np.asarray(exclude[0], dtype=np.int64), np.asarray(exclude[1], dtype=np.int64)
        ex[np.minimum(ei, ej), np.maximum(ei, ej)] = True
        div &= ~ex
    return rel, div, np.isnan(phi) & among


def census_numpy(phi, kin_thr, div_thr, keep=None, exclude=None):
    """(n_rel, n_div) as uint32: every pair credited to both of its samples."""
    rel, div, _ = classes_numpy(phi, kin_thr, div_thr, keep, exclude)
    return (rel.sum(0) + rel.sum(1)).astype(np.uint32), (div.sum(0) + div.sum(1)).astype(np.uint32)


DEGREE, NDIV, KINSUM, INDEX = "degree", "n_div", "kin sum", "index"


def partition_python(N, i, j, kin, n_div, keep, decided=None, tied=None):
    """The rule of include/fpca.h with nothing but loops.  decided / tied (dicts, optional): how many removals each level decided, and how
    many times more than one candidate was left after it."""
    keep = [bool(k) for k in keep]
    edges = {}
    for a, b, k in zip(i, j, kin):
        a, b = int(a), int(b)
        key = (min(a, b), max(a, b))
        if keep[a] and keep[b] and key not in edges:  # the first kin listed for a pair
            edges[key] = float(k)
    while edges:
        nb = [[] for _ in range(N)]
        for (a, b), k in edges.items():
            nb[a].append((b, k))
            nb[b].append((a, k))
        top = max(len(x) for x in nb)
        cand = [v for v in range(N) if len(nb[v]) == top]
        level = DEGREE
        if len(cand) > 1:
            if tied is not None:
                tied[DEGREE] = tied.get(DEGREE, 0) + 1
            low = min(int(n_div[v]) for v in cand)
            cand = [v for v in cand if int(n_div[v]) == low]
            level = NDIV
        if len(cand) > 1:
            if tied is not None:
                tied[NDIV] = tied.get(NDIV, 0) + 1
            sums = {}
            for v in cand:
                s = 0.0
                for _, k in sorted(nb[v]):  # ascending order of the neighbour's index
                    s += k
                sums[v] = s
            low = min(sums.values())
            cand = [v for v in cand if sums[v] == low]
            level = KINSUM
        if len(cand) > 1:
            if tied is not None:
                tied[KINSUM] = tied.get(KINSUM, 0) + 1
            cand = [max(cand)]
            level = INDEX
        if decided is not None:
            decided[level] = decided.get(level, 0) + 1
        v = cand[0]
        keep[v] = False
        edges = {e: k for e, k in edges.items() if v not in e}
    return np.array(keep, dtype=bool)
