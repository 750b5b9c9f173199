"""KING-robust kinship (fpca_king_block / fpca_king_pairs / fpca_king_cutoff; Context.king_block / king_pairs / king_cutoff, king_cutoff(),
flashpca(unrelated=)) on the GPU against a numpy yardstick that never calls the feature: the raw 2-bit codes are unpacked, the planes
x (dosage), m (call indicator) and q = x^2 are float64 matrices, the sums of a pair come from BLAS products -- integers below 2^53, so
exact -- and phi = (double)(2 hmin - D) / (double)(4 hmin) of include/fpca.h is one correctly rounded divide of two integers, which numpy
reproduces BIT FOR BIT: every comparison here is array_equal with NaN equal to NaN, over every pair.  The cutoff rule is restated in numpy
from the text of include/fpca.h (the largest current degree goes, the largest index among equals).
The generated pedigrees hold founders, parent-offspring trios, full sibs, duplicates, one sample without any call and one all-homozygous
sample (NaN rows); missing rates 0, 1 % and 20 % on samples of every second 32-sample block, so that whole blocks are free of missing calls
and take the x.x-only path.  The golden counts were recorded on the CPU from the restatement.  Every test prints what it measured
(pytest -s).
Measured on the MI355X (profiles/king_test_figures.txt): every block -- the square and six rectangles on each of the three shapes, the four
golden filesets -- equals numpy bit for bit; all lists and masks (3 thresholds x 3 shapes x {all, 30 % pre-cleared}; 5 thresholds x 4
filesets) equal the restatement's and the filesets keep the counts of GOLDEN; slabs of 64 / 128 rows and the forced five-product path
change nothing; flashpca(unrelated=0.0884) on hapmap3_data keeps 887 of 957, eigenvalues 2.2e-15, |u'u_ref| - 1 1.6e-15, U'U - I 3.6e-15,
pve 4.9e-17, held-out projection 4.2e-16, loadings 1.4e-15; after maf= / ld= 887 kept on 13,544 SNPs; keep= (672) plus unrelated= 630.  The
16 tests take 6.2 s together."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
ENOMEM = -4


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


# ---- data ------------------------------------------------------------------------------------------------------
def pack_codes(codes):
    """codes: (P, N) raw PLINK 2-bit codes -> the packed records."""
    P, N = codes.shape
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    return (c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)).astype(np.uint8)


def unpack_codes(packed, N, P):
    packed = np.asarray(packed, dtype=np.uint8).reshape(P, -1)
    return np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(P, -1)[:, :N]


def read_bed_codes(prefix):
    N = open(prefix + ".fam", "rb").read().count(b"\n")
    raw = np.fromfile(prefix + ".bed", dtype=np.uint8)[3:]
    P = raw.size // ((N + 3) // 4)
    return unpack_codes(raw, N, P), N, P


def pedigree_codes(N, P, seed):
    """(P, N) codes and the planted samples.  Sample s of an even 32-sample block (0 .. 31, 64 .. 95, ...) has no missing call; in the odd
    blocks every fourth sample has 1 % and every eighth 20 % of its calls missing."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, P)
    d = rng.binomial(2, p[None, :], (N, P))  # founders everywhere first

    def child(a, b):
        return rng.binomial(1, d[a] / 2.0) + rng.binomial(1, d[b] / 2.0)

    d[2], d[3] = child(0, 1), child(0, 1)     # a trio and a full sib: 0 - 2, 1 - 2 parent-offspring, 2 - 3 sibs
    d[40], d[41] = child(33, 36), child(33, 36)  # the same inside an odd block, among samples with missing calls
    d[5] = d[4]                                # duplicates without a missing call
    d[N - 1] = d[6]                            # ... across the whole range (the last sample: a ragged tile)
    d[48] = d[7]                               # a duplicate of which one copy has 1 % of its calls missing
    d[9] = 2 * rng.binomial(1, p)              # all homozygous: het = 0, every pair with it is NaN
    codes = np.array([3, 2, 0], dtype=np.uint8)[d]  # (N, P)
    s = np.arange(N)
    odd = (s // 32) % 2 == 1
    rate = np.where(odd & (s % 4 == 0), 0.01, 0.0)
    rate = np.where(odd & (s % 8 == 4), 0.20, rate)
    codes[rng.random((N, P)) < rate[:, None]] = 1
    codes[44] = 1  # no call at all
    return np.ascontiguousarray(codes.T), dict(dups=[(4, 5), (6, N - 1)], nocall=44, hom=9, rate=rate)


# 70 x 300     one 128-byte chunk per sample that is mostly pad SNPs; a ragged second tile (samples 64 .. 69)
# 130 x 1000   two chunks; three tiles, the last of two samples
# 257 x 2100   P_pad / 4 = 576 is not a multiple of 128: the pitch is rounded up to 640, the last 64 bytes are the preset; five chunks,
#              five tiles, the last of one sample
SHAPES = {"70x300": (70, 300, 1), "130x1000": (130, 1000, 2), "257x2100": (257, 2100, 3)}


# ---- the yardstick -------------------------------------------------------------------------------------------------
def king_numpy(codes):
    """phi[N][N] for every ordered pair, the diagonal included: the formula of include/fpca.h."""
    x = np.array([2.0, 0.0, 1.0, 0.0])[codes].T  # (N, P); 0 where missing
    m = (codes != 1).astype(np.float64).T
    q = x * x
    xm, qm, xx = x @ m.T, q @ m.T, x @ x.T  # [i][j]: sum x_i m_j, sum q_i m_j, sum x_i x_j
    assert max(a.max() for a in (xm, qm, xx)) < 2.0 ** 53
    xm, qm, xx = (a.astype(np.int64) for a in (xm, qm, xx))
    het = 2 * xm - qm          # het[i][j] = heterozygous calls of i among the SNPs j is called at (i's own missing calls have x = q = 0)
    D = qm + qm.T - 2 * xx
    hmin = np.minimum(het, het.T)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = (2 * hmin - D).astype(np.float64) / (4 * hmin).astype(np.float64)
    phi[hmin == 0] = np.nan
    return phi


def pairs_numpy(phi, thr, keep=None):
    """(i, j, phi) of the pairs i < j above thr among the kept samples, sorted by (i, j)."""
    N = phi.shape[0]
    with np.errstate(invalid="ignore"):
        above = np.triu(phi > thr, 1)  # (NaN: never)
    if keep is not None:
        above &= keep[:, None] & keep[None, :]
    i, j = np.nonzero(above)  # row-major: sorted by (i, j)
    return i.astype(np.uint32), j.astype(np.uint32), phi[i, j]


def cutoff_numpy(phi, thr, keep=None):
    """The rule of include/fpca.h: while an edge remains the sample of largest current degree goes, the largest index among equals."""
    N = phi.shape[0]
    keep = np.ones(N, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    with np.errstate(invalid="ignore"):
        A = np.triu(phi > thr, 1)
    A = (A | A.T) & keep[:, None] & keep[None, :]
    deg = A.sum(axis=1)
    while deg.max() > 0:
        v = N - 1 - int(np.argmax(deg[::-1]))  # the last index holding the maximum
        keep[v] = False
        deg -= A[:, v]
        A[v, :] = A[:, v] = False
        deg[v] = 0
    return keep


_CASE = {}


def case(name):
    """One generated shape: codes, phi of every pair from numpy -- computed once and left unchanged."""
    if name not in _CASE:
        N, P, seed = SHAPES[name]
        codes, planted = pedigree_codes(N, P, seed)
        _CASE[name] = dict(N=N, P=P, codes=codes, phi=king_numpy(codes), packed=pack_codes(codes), **planted)
    return _CASE[name]


def open_case(fp, c, accum="fp64"):
    return fp.Context.from_packed(c["packed"], c["N"], c["P"], accum=accum)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def same_pairs(got, want):
    return all(same(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


def rectangles(N):
    """Six rectangles off the 64-sample tiles and the 32-sample blocks; three reach below the diagonal, one is a single pair."""
    return [(5, 40, 3, N - 10), (33, N - 33, 0, 31), (N - 7, 7, N - 10, 10), (0, 1, N - 1, 1), (N - 1, 1, 0, N), (31, 34, 31, 34)]


# ---- 1. the block, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_block_bit_for_bit(fp, name):
    c = case(name)
    N, ref = c["N"], c["phi"]
    # the planted samples, in the yardstick itself
    for a, b in c["dups"]:
        assert c["rate"][a] == 0 and c["rate"][b] == 0 and ref[a, b] == 0.5 and ref[b, a] == 0.5  # duplicates without missing calls: exactly 1/2
    assert np.isnan(ref[c["hom"]]).all() and np.isnan(ref[:, c["hom"]]).all() and np.isnan(ref[c["nocall"]]).all()
    ok = np.ones(N, dtype=bool)
    ok[[c["hom"], c["nocall"]]] = False
    assert np.isfinite(ref[np.ix_(ok, ok)]).all() and np.all(np.diag(ref)[ok] == 0.5)
    assert 0.15 < ref[0, 2] < 0.35 and 0.15 < ref[1, 2] < 0.35 and 0.1 < ref[2, 3] < 0.4 and 0.1 < ref[40, 41] < 0.4 and abs(ref[0, 1]) < 0.1
    assert c["rate"][48] == 0.01 and ref[7, 48] == 0.5  # missing calls in one copy: identical over the shared SNPs, still exactly 1/2
    with open_case(fp, c) as ctx:
        got = ctx.king_block(0, N, 0, N)
        eq = same(got, ref)
        print("%s king_block(0, %d, 0, %d): %d finite, %d NaN, equal to numpy bit for bit: %s" % (
            name, N, N, np.isfinite(got).sum(), np.isnan(got).sum(), eq))
        assert eq, (name, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5])
        for a, b in c["dups"]:
            assert got[a, b] == 0.5
        assert np.array_equal(got, got.T, equal_nan=True)
        for i0, ni, j0, nj in rectangles(N):
            got = ctx.king_block(i0, ni, j0, nj)
            eq = same(got, np.ascontiguousarray(ref[i0:i0 + ni, j0:j0 + nj]))
            print("%s king_block(%d, %d, %d, %d): equal to numpy bit for bit: %s" % (name, i0, ni, j0, nj, eq))
            assert eq, (name, i0, ni, j0, nj)


# ---- 2. the pair list and the cutoff --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_pairs_and_cutoff(fp, name):
    c = case(name)
    N, ref = c["N"], c["phi"]
    pre = np.random.default_rng(7).random(N) >= 0.3  # a pre-cleared random 30 %
    pre[[0, 2, 4, 5]] = True
    pre[3] = False
    counts = []
    with open_case(fp, c, accum="auto") as ctx:  # (the int8 mode's own sample-major copy may be resident: it is not what the call reads)
        B = np.random.default_rng(4).standard_normal((N, 16))
        before = ctx.apply_xt(B)
        for thr in (0.3, 0.1, -1.0):
            for label, keep in (("all", None), ("70%", pre)):
                want = pairs_numpy(ref, thr, keep)
                got = ctx.king_pairs(thr, keep=keep)
                eq = same_pairs(got, want)
                wmask, gmask = cutoff_numpy(ref, thr, keep), ctx.king_cutoff(thr, keep=keep)
                print("%s thr %g keep=%s: yardstick lists %d pairs, the device %d, lists equal: %s; cutoff keeps %d and %d of %d, masks equal: %s" % (
                    name, thr, label, want[0].size, got[0].size, eq, wmask.sum(), gmask.sum(), N, np.array_equal(gmask, wmask)))
                assert eq, (name, thr, label)
                assert gmask.dtype == np.bool_ and np.array_equal(gmask, wmask), (name, thr, label)
                if keep is not None:
                    assert not gmask[~pre].any() and pre[got[0]].all() and pre[got[1]].all()
                    assert not ((got[0] == 2) & (got[1] == 3)).any()  # sample 3 is cleared: the sib pair is not listed
                else:
                    counts.append(want[0].size)
        after = ctx.apply_xt(B)
        assert np.array_equal(before, after)  # the context computes what it computed
    # the cases are not vacuous: duplicates only; then the first-degree pairs too; then every pair that has a value
    nvalid = N - 2
    assert 3 <= counts[0] < counts[1] < counts[2] == nvalid * (nvalid - 1) // 2, counts
    i, j, _ = pairs_numpy(ref, 0.1)
    assert ((i == 2) & (j == 3)).any() and ((i == 0) & (j == 2)).any() and ((i == 40) & (j == 41)).any()


def test_slabs_and_the_general_path_change_nothing(fp, monkeypatch):
    """The test build's switches: the triangle in slabs of 64 and 128 rows (one and two row tiles per launch; the default is one launch),
    and the five-product path forced where the x.x-only path would run -- the same lists, masks and block bits."""
    c = case("257x2100")
    N, ref = c["N"], c["phi"]
    want = {thr: pairs_numpy(ref, thr) for thr in (0.1, -1.0)}
    with fp.test_hooks():
        with open_case(fp, c) as ctx:
            for rows in ("64", "128", "100000"):
                monkeypatch.setenv("FPCA_KING_SLAB_ROWS", rows)
                for thr in (0.1, -1.0):
                    got = ctx.king_pairs(thr)
                    print("slabs of %s rows, thr %g: %d pairs, equal to the yardstick: %s" % (rows, thr, got[0].size, same_pairs(got, want[thr])))
                    assert same_pairs(got, want[thr])
                assert np.array_equal(ctx.king_cutoff(0.1), cutoff_numpy(ref, 0.1))
            monkeypatch.delenv("FPCA_KING_SLAB_ROWS")
            monkeypatch.setenv("FPCA_KING_FORCE_GENERAL", "1")
            got, blk = ctx.king_pairs(-1.0), ctx.king_block(0, N, 0, N)
            monkeypatch.delenv("FPCA_KING_FORCE_GENERAL")
            print("forced general path: %d pairs, list equal %s, block equal %s" % (got[0].size, same_pairs(got, want[-1.0]), same(blk, ref)))
            assert same_pairs(got, want[-1.0]) and same(blk, ref)


def test_fast_path_is_taken_and_gives_the_same_bits(fp):
    """A source without a single missing call (every block takes the x.x-only path, pad SNPs on both sides) against numpy."""
    N, P = 100, 700
    rng = np.random.default_rng(21)
    d = rng.binomial(2, rng.uniform(0.1, 0.9, P)[None, :], (N, P))
    d[50] = d[10]
    codes = np.ascontiguousarray(np.array([3, 2, 0], dtype=np.uint8)[d].T)
    ref = king_numpy(codes)
    assert ref[10, 50] == 0.5 and np.isfinite(ref).all()
    with fp.Context.from_packed(pack_codes(codes), N, P) as ctx:
        got = ctx.king_block(0, N, 0, N)
        lst = ctx.king_pairs(0.0)
    print("no missing call: block equal to numpy %s, %d pairs above 0, list equal %s" % (same(got, ref), lst[0].size, same_pairs(lst, pairs_numpy(ref, 0.0))))
    assert same(got, ref) and same_pairs(lst, pairs_numpy(ref, 0.0)) and lst[0].size > 0


def test_overflow_names_the_count(fp, monkeypatch):
    c = case("130x1000")
    ref = c["phi"]
    need = pairs_numpy(ref, 0.1)[0].size
    assert need > 3
    with open_case(fp, c) as ctx:
        with pytest.raises(fp.FpcaError, match="%d pairs are above the threshold, the arrays hold 3" % need) as e:
            ctx.king_pairs(0.1, max_pairs=3)
        assert e.value.code == ENOMEM
        # the C call itself: *n_pairs is the number needed
        import ctypes as C

        n = C.c_uint64(0)
        i = np.zeros(3, dtype=np.uint32)
        j = np.zeros(3, dtype=np.uint32)
        p = np.zeros(3)
        rc = fp.lib().fpca_king_pairs(ctx.h, None, 0.1, 3, i.ctypes.data, j.ctypes.data, p.ctypes.data, C.byref(n))
        assert rc == ENOMEM and n.value == need
        i, j, p = np.zeros(need, dtype=np.uint32), np.zeros(need, dtype=np.uint32), np.zeros(need)
        rc = fp.lib().fpca_king_pairs(ctx.h, None, 0.1, need, i.ctypes.data, j.ctypes.data, p.ctypes.data, C.byref(n))
        assert rc == 0 and n.value == need  # exactly enough room
    nall = pairs_numpy(ref, -1.0)[0].size
    with fp.test_hooks():
        monkeypatch.setenv("FPCA_KING_MAX_PAIRS", "10")
        with open_case(fp, c) as ctx:
            with pytest.raises(fp.FpcaError, match="%d pairs are above the threshold, the call keeps room for 10" % nall) as e:
                ctx.king_cutoff(-1.0)
            assert e.value.code == ENOMEM
            assert np.array_equal(ctx.king_cutoff(0.3), cutoff_numpy(ref, 0.3))  # fewer than 10 pairs: served
        monkeypatch.delenv("FPCA_KING_MAX_PAIRS")
    print("overflow: %d pairs needed against 3, %d against the internal 10: both refused with the count" % (need, nall))


# ---- 3. golden filesets -------------------------------------------------------------------------------------------------
# pairs above thr / samples kept, recorded on the CPU from the restatement
GOLDEN = {
    "hapmap3_data": ((957, 14389), {0.177: (47, 920), 0.0884: (106, 887), 0.0442: (192, 868), 0.0: (18646, 329), 0.354: (0, 957)}),
    "data_chr1": ((957, 1129), {0.177: (62, 912), 0.0884: (134, 883), 0.0442: (2809, 666), 0.0: (49853, 246), 0.354: (2, 955)}),
    "hm3_thinned": ((957, 14079), {0.177: (47, 920), 0.0884: (107, 887), 0.0442: (202, 866), 0.0: (25510, 283), 0.354: (0, 957)}),
    "kg_thinned": ((1092, 14079), {0.177: (27, 1072), 0.0884: (41, 1063), 0.0442: (61, 1048), 0.0: (16899, 510), 0.354: (0, 1092)}),
}
_GOLD = {}


def golden(name):
    if name not in _GOLD:
        codes, N, P = read_bed_codes(os.path.join(GOLD, name))
        _GOLD[name] = dict(codes=codes, N=N, P=P, phi=king_numpy(codes))
    return _GOLD[name]


@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_filesets(fp, name):
    g = golden(name)
    (N, P), table = GOLDEN[name]
    assert (g["N"], g["P"]) == (N, P)
    ref = g["phi"]
    nan_pairs = int(np.isnan(ref[np.triu_indices(N, 1)]).sum())
    assert nan_pairs == 0
    with fp.Context.from_bed(os.path.join(GOLD, name + ".bed"), N, accum="auto") as ctx:
        blk = ctx.king_block(0, N, 0, N)
        assert same(blk, ref), name
        for thr, (npairs, nkept) in table.items():
            want = pairs_numpy(ref, thr)
            wmask = cutoff_numpy(ref, thr)
            got = ctx.king_pairs(thr)
            gmask = ctx.king_cutoff(thr)
            print("%s thr %g: yardstick %d pairs / %d kept, the device %d / %d, lists equal %s, masks equal %s" % (
                name, thr, want[0].size, wmask.sum(), got[0].size, gmask.sum(), same_pairs(got, want), np.array_equal(gmask, wmask)))
            assert (want[0].size, int(wmask.sum())) == (npairs, nkept), (name, thr)
            assert same_pairs(got, want) and np.array_equal(gmask, wmask), (name, thr)
    assert np.array_equal(fp.king_cutoff(os.path.join(GOLD, name), 0.0884), cutoff_numpy(ref, 0.0884))  # the fileset entry point


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
def subset_oracle(O, codes, keep, stand="binom2"):
    """tests/test_gpu_subset.py: X of the re-packed kept samples, their mean / sd, X of the others under that mean / sd, trace."""
    P = codes.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(packed=pack_codes(codes[:, keep]), N=int(keep.sum()), P=P, stand=stand)
        Xs, ms = od.dense(), od.meansd()
        oh = O.OracleData(packed=pack_codes(codes[:, ~keep]), N=int((~keep).sum()), P=P, stand=stand)
        oh.set_preloaded_meansd(ms)
        Xh = oh.dense()
    return Xs, ms, Xh, float(np.sum(Xs * Xs))


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def test_flashpca_unrelated_against_the_oracle(fp, O):
    """The tolerances of tests/test_gpu_subset.py (check_pca): eigenvalues 1e-9 relative against dense eigh, |u'u_ref| within 1e-8 of 1,
    U'U within 1e-10 of I, pve 1e-11, the kept rows of the projection U sqrt(d) to 1e-14, the held-out rows X_h V / sqrt(P) and the
    loadings to 1e-11, center / scale array_equal."""
    g = golden("hapmap3_data")
    codes, N, P, k = g["codes"], g["N"], g["P"], 10
    want = cutoff_numpy(g["phi"], 0.0884)
    assert want.sum() == 887
    r = fp.flashpca(HM3, ndim=k, tol=1e-8, do_loadings=True, unrelated=0.0884)
    keep = r["unrelated_kept"]
    assert keep.dtype == np.bool_ and np.array_equal(keep, want)
    nk = int(keep.sum())
    assert r["vectors"].shape == (nk, k) and r["projection"].shape == (nk, k) and r["projection_all"].shape == (N, k) and "snps_kept" not in r
    Xs, ms_ref, Xh, tr_ref = subset_oracle(O, codes, keep)
    w, Q = np.linalg.eigh(Xs @ Xs.T)
    w, Q = w[::-1][:k] / P, Q[:, ::-1][:, :k]
    U, d, V, Pall = r["vectors"], r["values"], r["loadings"], r["projection_all"]
    e_d = float(np.max(np.abs(d - w) / w))
    e_u = float(np.max(np.abs(np.abs(np.sum(U * Q, axis=0)) - 1.0)))
    e_o = float(np.max(np.abs(U.T @ U - np.eye(k))))
    e_pve = float(np.max(np.abs(r["pve"] - w / (tr_ref / P))))
    e_px = relmax(Pall[~keep], Xh @ V / np.sqrt(P))
    v_ref = Xs.T @ U / np.sqrt(d) / np.sqrt(P)
    e_v = float(np.max(np.abs(V - v_ref)) / np.max(np.abs(v_ref)))
    print("flashpca(unrelated=0.0884): %d of %d samples; eigenvalues %.2e, |u'u_ref| - 1 %.2e, U'U - I %.2e, pve %.2e, held-out projection %.2e, "
          "loadings %.2e" % (nk, N, e_d, e_u, e_o, e_pve, e_px, e_v))
    assert e_d <= 1e-9 and e_u <= 1e-8 and e_o <= 1e-10 and e_pve <= 1e-11 and e_px <= 1e-11 and e_v <= 1e-11
    assert np.allclose(r["projection"], U * np.sqrt(d), rtol=1e-14, atol=0) and np.array_equal(Pall[keep], r["projection"])
    assert np.array_equal(r["center"], ms_ref[:, 0], equal_nan=True) and np.array_equal(r["scale"], ms_ref[:, 1], equal_nan=True)
    # the same as keep= with that mask
    f = fp.flashpca(HM3, ndim=k, tol=1e-8, do_loadings=True, keep=keep)
    for key in ("values", "vectors", "projection", "projection_all", "loadings", "center", "scale"):
        assert np.array_equal(f[key], r[key], equal_nan=True), key


def test_flashpca_unrelated_after_snp_filters_and_with_keep(fp):
    g = golden("hapmap3_data")
    N = g["N"]
    r = fp.flashpca(HM3, ndim=5, maf=0.05, ld=(1000, 50, 0.05), unrelated=0.0884)
    snps = r["snps_kept"]
    direct = fp.king_cutoff(HM3, 0.0884, maf=0.05, ld=(1000, 50, 0.05))
    want = cutoff_numpy(king_numpy(g["codes"][snps]), 0.0884)  # the yardstick on the compacted fileset
    print("flashpca(maf=0.05, ld=(1000, 50, 0.05), unrelated=0.0884): %d of %d SNPs, %d of %d samples; equal to king_cutoff() %s, to the yardstick %s" % (
        snps.sum(), g["P"], r["unrelated_kept"].sum(), N, np.array_equal(r["unrelated_kept"], direct), np.array_equal(direct, want)))
    assert 0 < snps.sum() < g["P"] and np.array_equal(r["unrelated_kept"], direct) and np.array_equal(direct, want)
    assert r["vectors"].shape == (int(direct.sum()), 5) and r["projection_all"].shape == (N, 5)
    # keep= plus unrelated=: the cutoff runs among the kept samples and never revives a cleared one
    keep = np.random.default_rng(31).random(N) < 0.7
    r = fp.flashpca(HM3, ndim=5, keep=keep, unrelated=0.0884)
    want = cutoff_numpy(g["phi"], 0.0884, keep)
    print("keep= (%d samples) plus unrelated=: %d kept, equal to the yardstick %s" % (keep.sum(), r["unrelated_kept"].sum(), np.array_equal(r["unrelated_kept"], want)))
    assert np.array_equal(r["unrelated_kept"], want) and not r["unrelated_kept"][~keep].any() and want.sum() < keep.sum()
    assert r["vectors"].shape == (int(want.sum()), 5)
    assert np.array_equal(fp.king_cutoff(HM3, 0.0884, keep=keep), want)
    # the existing refusals stay
    with pytest.raises(ValueError, match="cannot be combined with keep"):
        fp.flashpca(HM3, ndim=2, maf=0.05, keep=keep, unrelated=0.0884)
    with pytest.raises(ValueError, match="numeric matrix"):
        fp.flashpca(np.zeros((8, 5)), ndim=1, unrelated=0.0884)


# ---- 5. refusals and state -------------------------------------------------------------------------------------------------
def test_refusals(fp):
    c = case("70x300")
    N, ref = c["N"], c["phi"]

    def refused(call, msg, code=-1):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == code
        print("refused: %s" % str(e.value)[:110])

    with open_case(fp, c) as ctx:
        refused(lambda: ctx.king_block(0, N + 1, 0, N), "are not a non-empty rectangle")
        refused(lambda: ctx.king_block(0, N, N, 1), "are not a non-empty rectangle")
        refused(lambda: ctx.king_block(3, 0, 0, N), "are not a non-empty rectangle")
        refused(lambda: ctx.king_pairs(float("nan")), "fpca_king_pairs: the threshold is NaN")
        refused(lambda: ctx.king_cutoff(float("nan")), "fpca_king_cutoff: the threshold is NaN")
        L = fp.lib()
        assert L.fpca_king_block(ctx.h, 0, N, 0, N, None) == -1 and L.fpca_king_cutoff(ctx.h, 0.1, None, None) == -1
        assert L.fpca_king_pairs(ctx.h, None, 0.1, 5, None, None, None, None) == -1
        with pytest.raises(ValueError):
            ctx.king_cutoff(0.1, keep=np.ones(N + 1, dtype=bool))
        with pytest.raises(ValueError):
            ctx.king_pairs(0.1, keep=np.ones(N - 1, dtype=bool))
        mask = np.arange(N) % 3 != 0
        ctx.set_sample_mask(mask)
        for call, fn in ((lambda: ctx.king_block(0, N, 0, N), "fpca_king_block"), (lambda: ctx.king_pairs(0.1), "fpca_king_pairs"),
                         (lambda: ctx.king_cutoff(0.1), "fpca_king_cutoff")):
            refused(call, fn + ": a sample mask is set .* pass the mask as `keep` instead")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        for call in (lambda: ctx.king_block(0, N, 0, N), lambda: ctx.king_pairs(0.1), lambda: ctx.king_cutoff(0.1)):
            refused(call, "one shard of several")
        ctx.set_rank(1, 0)
        # a preloaded mean/sd is not refused: nothing here reads it
        ctx.set_meansd(ctx.stats()[0])
        assert same(ctx.king_block(0, N, 0, N), ref) and np.array_equal(ctx.king_cutoff(0.1, keep=mask), cutoff_numpy(ref, 0.1, mask))
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.king_block(0, 50, 0, 50), "fpca_king_block: this context holds a dense matrix")
        refused(lambda: dense.king_pairs(0.1), "fpca_king_pairs: this context holds a dense matrix")
        refused(lambda: dense.king_cutoff(0.1), "fpca_king_cutoff: this context holds a dense matrix")
    # a 2 GiB block: one sample row of 2^28 + 1 columns cannot exist here, so the limit is met through a wide context of few SNPs
    big_n = 2 ** 14 + 1
    with fp.Context.from_packed(np.full(((big_n + 3) // 4) * 2, 0xFF, dtype=np.uint8), big_n, 2) as wide:
        buf = np.zeros(1)
        assert fp.lib().fpca_king_block(wide.h, 0, big_n, 0, big_n, buf.ctypes.data) == -1  # 16385^2 doubles > 1 GiB
        msg = fp.lib().fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "16385 x 16385 doubles is over the limit of 1073741824 bytes" in msg
