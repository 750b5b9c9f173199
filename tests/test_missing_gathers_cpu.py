"""The host-side decisions behind the missing-call list routes of the exact-integer mode, ported to Python, and the test
matrices of tests/test_gpu_missing_gathers.py.  No device.

 * gather_variant: which gather kernel kern::sparse_rows_sum / sparse_rows_sum_f32 launch (csrc/missing_kernels.hip sparse_rows_sum_variant):
   1 = k_sparse_rows_sum, 2 = k_sparse_rows_sum_batched, 3 = k_sparse_rows_sum_short.  K2 calls with (short_lists, avg_len) = (False, 0),
   K3 with (True, listed calls per sample); FPCA_GATHER (test build) forces a kernel.  Checked against a table.
 * hybrid_classify: the cost model that decides per SNP whether its missing calls are listed or go to the matrix cores, and whether the
   shard takes the hybrid route at all (csrc/missing_routes.hip hybrid_classify).
 * missing_pattern: the two matrices of the GPU tests -- tall (16,450 samples x 130 SNPs: a SNP's record is 257 sixteen-byte pieces and
   two codes, one more than k_fill_missing walks in a step) and wide (610 x 16,450: the same for a sample's record in the sample-major
   copy).  The tests here check that each matrix holds what the GPU tests are about, that it qualifies for the hybrid route at 7 and at 4
   slices with SNPs on both sides of the threshold, and that listed calls remain; route_cases() names, for every operator case of the
   GPU file, the route and the gather kernel of both stages.

A sample missing at every SNP and a SNP without a missing call cannot both exist: the sample is missing at every SNP but that one, and
the sample without a missing call has one at the SNP that is missing everywhere."""
import numpy as np
import pytest

G_CALL, D_CELL, M2_CELL = 2.0e-12, 1.96e-15, 1.45e-15  # csrc/missing_routes.hip

TALL = (16450, 130)  # N samples, P SNPs
WIDE = (610, 16450)
STEP = 16384  # codes k_fill_missing walks per step: 256 threads x 64 codes


def gather_variant(b, rowscale, short_lists, avg_len, forced=0):
    """The kernel a gather launch takes; forced: the value of FPCA_GATHER (0 = unset)."""
    if forced:
        variant = forced
    elif avg_len > 0 and avg_len <= 24.0 and b <= 32 and not rowscale:
        variant = 3
    else:
        variant = 2 if (rowscale or short_lists) else 1
    if variant == 3 and b <= 32 and not rowscale:
        return 3
    return 1 if variant == 1 else 2


def hybrid_classify(nmiss, N, S):
    """nmiss: missing calls per SNP.  Returns (the shard takes the hybrid route, indices of the SNPs that go dense, listed calls left)."""
    nmiss = np.asarray(nmiss, dtype=np.int64)
    thr = D_CELL * S / G_CALL * float(N)
    dense = np.nonzero(nmiss.astype(np.float64) > thr)[0]
    total = int(nmiss.sum())
    rest = total - int(nmiss[dense].sum())
    if dense.size == 0 or rest >= 2 ** 31:
        return False, dense, rest
    ch = G_CALL * float(rest) + D_CELL * float(N) * S * float(dense.size)
    two = M2_CELL * float(N) * S * float(nmiss.size)
    ok = ch < two and ch < 0.85 * (G_CALL * float(total))
    return bool(ok), dense, rest


def dense_threshold(N, S):
    return D_CELL * S / G_CALL * float(N)


# ---- the test matrices ----------------------------------------------------------------------------------
J_CLEAN, J_ALL, J_ENDS, J_MID = 3, 5, 7, 9        # SNPs: no missing call; missing everywhere; first and last sample; around the step
I_ALL, I_CLEAN, I_ENDS, I_MID = 2, 4, 6, 8        # samples: the same, by sample
J_EXACT0, J_HEAVY0 = 20, 30                       # SNPs with a chosen number of calls; SNPs missing in 40 % (wide) or 3 % (tall) of the samples
_PATTERNS = {}


def _around(n):
    """Positions of a record of n codes on both sides of every boundary the list kernel has: its step if the record is longer than one,
    else a thread's 64 codes and a dword's 16; and the ragged last piece."""
    pos = [STEP - 1, STEP, STEP + 1] if n > STEP + 1 else [15, 16, 63, 64]
    last = (n - 1) // 64 * 64
    return sorted(set(pos + [last - 1, last]))


def exact_counts(N):
    """Call counts on both sides of the dense threshold at 4 and at 7 slices."""
    return sorted({int(dense_threshold(N, S)) + d for S in (4, 7) for d in (0, 1)})


def missing_pattern(shape, seed=20261019):
    """(codes [P][N] uint8 PLINK codes, 1 = missing; info)."""
    if shape in _PATTERNS:
        return _PATTERNS[shape]
    N, P = shape
    rng = np.random.default_rng(seed + N)
    miss = rng.random((P, N)) < 0.001
    n_heavy = 3 if P < 1000 else 64
    heavy = np.arange(J_HEAVY0, J_HEAVY0 + n_heavy)
    miss[heavy] = rng.random((n_heavy, N)) < (0.03 if P < 1000 else 0.4)
    others = np.setdiff1d(np.arange(N), [I_ALL, I_CLEAN, I_ENDS, I_MID, 0, N - 1])
    exact = {}
    for n, k in enumerate(exact_counts(N)):  # SNPs with exactly k calls, the one of sample I_ALL included
        j = J_EXACT0 + n
        miss[j] = False
        miss[j, rng.choice(others, size=k - 1, replace=False)] = True
        exact[j] = k
    miss[J_ENDS, [0, N - 1]] = True
    miss[J_MID, _around(N)] = True
    miss[[0, P - 1], I_ENDS] = True
    miss[_around(P), I_MID] = True
    miss[:, I_ALL] = True
    miss[:, I_CLEAN] = False
    miss[J_ALL] = True
    miss[J_CLEAN] = False
    freq = rng.uniform(0.1, 0.5, size=P)
    dosage = rng.binomial(2, freq[:, None], size=(P, N))
    codes = np.array([3, 2, 0], dtype=np.uint8)[dosage]  # dosage 0 -> code 3, 1 -> 2, 2 -> 0
    codes[miss] = 1
    _PATTERNS[shape] = codes, dict(N=N, P=P, exact=exact, heavy=heavy)
    return _PATTERNS[shape]


def pack_codes(codes):
    """[P][N] codes -> PLINK records, P x ceil(N / 4) bytes: sample 4 i + s in bits 2 s .. 2 s + 1 of byte i, pad bits 0."""
    P, N = codes.shape
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    return np.ascontiguousarray(c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6))


def unpack_codes(packed, N, P):
    b = np.asarray(packed, dtype=np.uint8).reshape(P, (N + 3) // 4)
    return np.stack([(b >> (2 * s)) & 3 for s in range(4)], axis=2).reshape(P, -1)[:, :N]


def csr_of(mask):
    """(ptr, idx) of the True entries of every row, ascending -- np.nonzero of the rows."""
    r, c = np.nonzero(mask)
    ptr = np.zeros(mask.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=mask.shape[0]), out=ptr[1:])
    return ptr, c.astype(np.int64)


def hybrid_view(miss, N, S):
    """The missing-call mask [P][N] as the hybrid route's lists see it: the rows of the dense SNPs cleared."""
    ok, dense, rest = hybrid_classify(miss.sum(axis=1), N, S)
    assert ok
    view = miss.copy()
    view[dense] = False
    assert int(view.sum()) == rest
    return view, dense


def operands(N, P, b):
    """The blocks of the operator cases: two integer blocks in [-4, 4] and two normal ones for X'B and X X'B (N rows), two normal ones for
    X T (P rows) -- the same in every process."""
    rng = np.random.default_rng(1000 * N + b)
    Bi, Bi2 = (rng.integers(-4, 5, size=(N, b)).astype(np.float64) for _ in range(2))
    Bn, Bn2 = rng.standard_normal((N, b)), rng.standard_normal((N, b))
    Tn, Tn2 = rng.standard_normal((P, b)), rng.standard_normal((P, b))
    return dict(xt=(Bi, Bi2), xxt=(Bn, Bn2), x=(Tn, Tn2))


# Every operator case of the GPU file: shape, slices, width, route -> the kernel of K2's gather (by SNP: short_lists False, no length) and of
# K3's (by sample: short_lists True, listed calls per sample), per value of FPCA_GATHER.  Routes 1 and 0 gather nothing.
def route_cases():
    out = []
    for shape in (TALL, WIDE):
        miss = missing_pattern(shape)[0] == 1
        for S in (7, 4):
            listed = {3: int(miss.sum()), 4: hybrid_classify(miss.sum(axis=1), shape[0], S)[2]}
            for b in (16, 32, 64):
                for route in (4, 3, 1, 0):
                    for forced in (0, 1, 2, 3):
                        k2 = k3 = 0
                        if route in (3, 4):
                            k2 = gather_variant(b, False, False, 0.0, forced)
                            k3 = gather_variant(b, False, True, listed[route] / shape[0], forced)
                        out.append(dict(shape=shape, S=S, b=b, route=route, forced=forced, k2=k2, k3=k3, listed=listed.get(route, 0)))
    return out


# ---- tests -------------------------------------------------------------------------------------------
VARIANT_TABLE = [
    # b, rowscale, short_lists, avg_len, forced -> kernel
    (16, False, False, 0.0, 0, 1), (32, False, False, 0.0, 0, 1), (64, False, False, 0.0, 0, 1),   # K2
    (16, False, True, 0.0, 0, 2), (32, False, True, 30.0, 0, 2), (64, False, True, 100.0, 0, 2),   # K3, long lists or no length
    (16, False, True, 12.5, 0, 3), (32, False, True, 24.0, 0, 3), (32, False, True, 1e-3, 0, 3),   # K3, a dozen entries
    (16, False, False, 12.5, 0, 3),                                                                # (the length decides, not the flag)
    (32, False, True, 24.000001, 0, 2), (16, False, True, -1.0, 0, 2),
    (64, False, True, 12.5, 0, 2), (64, False, False, 12.5, 0, 1),                                 # no short kernel for 64 columns
    (16, True, False, 0.0, 0, 2), (16, True, False, 12.5, 0, 2), (32, True, True, 12.5, 0, 2),     # a per-row factor: batched
    (16, False, True, 12.5, 1, 1), (16, False, False, 0.0, 2, 2), (32, False, False, 0.0, 3, 3),   # forced
    (64, False, False, 0.0, 3, 2), (16, True, False, 0.0, 3, 2), (16, True, True, 12.5, 1, 1), (16, False, False, 0.0, 5, 2),
]


@pytest.mark.parametrize("b,rowscale,short_lists,avg_len,forced,want", VARIANT_TABLE)
def test_gather_variant_table(b, rowscale, short_lists, avg_len, forced, want):
    assert gather_variant(b, rowscale, short_lists, avg_len, forced) == want


def test_cost_model_thresholds():
    """The figures the comments of hybrid_classify quote: a SNP goes dense above 0.69 % of the samples at 7 slices; uniform rates never
    qualify (no SNP above the threshold, or no gain over the alternatives)."""
    assert abs(dense_threshold(100000, 7) / 100000 - 0.00686) < 1e-5
    assert int(dense_threshold(610, 7)) == 4 and int(dense_threshold(610, 4)) == 2 and dense_threshold(130, 7) < 1
    ok, dense, rest = hybrid_classify(np.full(1000, 3), 610, 7)
    assert not ok and dense.size == 0 and rest == 3000
    ok, dense, rest = hybrid_classify(np.full(1000, 50), 610, 7)  # every SNP dense: the two-matrix kernels are cheaper
    assert not ok and dense.size == 1000 and rest == 0
    nm = np.full(1000, 1)
    nm[:10] = 300
    ok, dense, rest = hybrid_classify(nm, 610, 7)
    assert ok and list(dense) == list(range(10)) and rest == 990


@pytest.mark.parametrize("shape", [TALL, WIDE])
def test_pattern_holds_every_edge(shape):
    codes, info = missing_pattern(shape)
    N, P = shape
    assert codes.shape == (P, N) and N % 4 == 2 and P % 4 == 2  # the last byte of a record is partial either way
    assert max(N, P) == 257 * 64 + 2
    miss = codes == 1
    assert np.array_equal(unpack_codes(pack_codes(codes), N, P), codes)
    rate = (miss.sum() - miss[info["heavy"]].sum() - N - P) / (N * P)
    assert 0.0005 < rate < 0.002, rate  # the background
    by_snp, by_smp = miss.sum(axis=1), miss.sum(axis=0)
    assert by_snp[J_CLEAN] == 0 and by_snp[J_ALL] == N
    assert by_smp[I_ALL] == P - 1 and by_smp[I_CLEAN] == 1
    assert miss[J_ENDS, 0] and miss[J_ENDS, N - 1] and miss[0, I_ENDS] and miss[P - 1, I_ENDS]  # first and last code of a record ...
    assert miss[:, N - 1].sum() >= 2 and miss[P - 1].sum() >= 2                                  # ... the last one just below ncols
    n, rec = (N, miss[J_MID]) if N > P else (P, miss[:, I_MID])
    assert n > STEP and rec[STEP - 1] and rec[STEP] and rec[STEP + 1]  # both sides of the step of k_fill_missing
    assert rec[n // 64 * 64 - 1] and rec[n // 64 * 64]                  # ... and of the ragged last piece
    assert rec[:STEP].sum() > 3 and rec[STEP:].sum() >= 4                # the carry from the first step is not zero
    long_records = miss if N > P else miss.T
    assert (long_records[:, :STEP].any(axis=1) & long_records[:, STEP:].any(axis=1)).sum() > 10
    for j, k in info["exact"].items():
        assert by_snp[j] == k


@pytest.mark.parametrize("shape", [TALL, WIDE])
@pytest.mark.parametrize("S", [7, 4])
def test_pattern_takes_the_hybrid_route(shape, S):
    codes, info = missing_pattern(shape)
    N, P = shape
    miss = codes == 1
    by_snp = miss.sum(axis=1)
    ok, dense, rest = hybrid_classify(by_snp, N, S)
    thr = int(dense_threshold(N, S))
    print(shape, S, "threshold", dense_threshold(N, S), "dense SNPs", dense.size, "listed", rest, "of", int(miss.sum()))
    assert ok and 0 < dense.size < P // 4
    assert rest > 1000 and rest < miss.sum()  # listed calls remain
    assert J_ALL in dense and set(info["heavy"]) <= set(dense) and J_CLEAN not in dense
    at, above = [j for j, k in info["exact"].items() if k == thr], [j for j, k in info["exact"].items() if k == thr + 1]
    assert at and above and not set(at) & set(dense) and set(above) <= set(dense)  # both sides of the threshold
    view, d2 = hybrid_view(miss, N, S)
    assert np.array_equal(d2, dense) and not view[dense].any() and view[:, I_ALL].sum() == P - 1 - dense.size


def test_route_cases_cover_both_k3_kernels():
    cases = route_cases()
    assert len(cases) == 2 * 2 * 3 * 4 * 4
    for c in cases:
        if c["route"] in (0, 1):
            assert (c["k2"], c["k3"]) == (0, 0)
            continue
        per_sample = c["listed"] / c["shape"][0]
        if c["forced"]:
            want = c["forced"] if (c["forced"] != 3 or c["b"] <= 32) else 2
            assert (c["k2"], c["k3"]) == (want, want), c
            continue
        assert c["k2"] == 1, c
        if c["shape"] == TALL:  # about 1.2 calls per sample on the plain lists, a tenth of that on the hybrid view: the short kernel
            assert 0 < per_sample <= 24 and c["k3"] == (3 if c["b"] <= 32 else 2), c
        else:                   # dozens per sample: the batched kernel
            assert per_sample > 24 and c["k3"] == 2, c
    tall3 = [c for c in cases if c["shape"] == TALL and c["route"] == 3 and c["S"] == 7 and c["b"] == 16 and not c["forced"]][0]
    assert 1.0 < tall3["listed"] / TALL[0] < 1.5
