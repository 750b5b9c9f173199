"""The KING relationship table (fpca_king_counts_block / fpca_king_related / fpca_king_cutoff_shared / fpca_king_classify;
Context.king_counts_block / king_related / king_cutoff_shared, king_related(), flashpca(unrelated_min_shared=)) on the GPU against a numpy
yardstick that never calls the feature and does not use the identity the kernel rests on: the raw 2-bit codes are unpacked, IBS0 is COUNTED
as a0 a2' + a2 a0' with a0 = (code 3) and a2 = (code 0), shared is m m', hethet is h h', and het_i / het_j / D / phi are those of
tests/test_gpu_king.py -- float64 BLAS products of 0/1/2 matrices, integers below 2^53, so exact; phi is one correctly rounded divide of two
integers, which numpy reproduces bit for bit.  Every comparison is array_equal with NaN equal to NaN, over every pair.  The pedigrees are
those of tests/test_gpu_king.py by the same recipe, restated here.  Every test prints what it measured (pytest -s).
Measured on the MI355X (profiles/king_rel_test_figures.txt): the six counts of every block -- the square and six rectangles on each of the
three shapes -- equal direct counting and phi equals numpy and king_block bit for bit; all tables and masks (3 thresholds x 4 values of
min_shared x {all, 30 % pre-cleared} x 3 shapes) equal the restatement's, 32,385 / 28,680 / 24,976 / 0 pairs at 257 x 2,100 and thr -1;
slabs of 64 / 128 rows and the forced seven-product path change nothing; the pedigrees give 3 duplicates, 8 parent-offspring and 2 full-sib
pairs, the planted ones; the four golden filesets keep the per-type counts of GOLDEN over the whole triangle; flashpca(unrelated=0.0884,
unrelated_min_shared=14389) keeps all 957 samples of hapmap3_data (no pair shares every SNP) against 887 without the filter; the four
entry points that own scratch acquire 4, 8, 8 and 9 times and give everything back.  The 19 tests take 2.4 s together."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
ENOMEM = -4
PO_IBS0 = 0.005


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


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
    """The recipe of tests/test_gpu_king.py: (P, N) codes.  Founders; two trios with a sib each (0, 1 -> 2, 3 without missing calls; 33, 36 ->
    40, 41 in a block with missing calls); three duplicates (4 = 5, 6 = N - 1, 7 = 48 of which 48 has 1 % missing); sample 9 all
    homozygous; sample 44 without any call.  A sample of an even 32-sample block has no missing call; in the odd blocks every fourth sample
    has 1 % and every eighth 20 % of its calls missing."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, P)
    d = rng.binomial(2, p[None, :], (N, P))

    def child(a, b):
        return rng.binomial(1, d[a] / 2.0) + rng.binomial(1, d[b] / 2.0)

    d[2], d[3] = child(0, 1), child(0, 1)
    d[40], d[41] = child(33, 36), child(33, 36)
    d[5] = d[4]
    d[N - 1] = d[6]
    d[48] = d[7]
    d[9] = 2 * rng.binomial(1, p)
    codes = np.array([3, 2, 0], dtype=np.uint8)[d]  # (N, P)
    s = np.arange(N)
    odd = (s // 32) % 2 == 1
    rate = np.where(odd & (s % 4 == 0), 0.01, 0.0)
    rate = np.where(odd & (s % 8 == 4), 0.20, rate)
    codes[rng.random((N, P)) < rate[:, None]] = 1
    codes[44] = 1
    return np.ascontiguousarray(codes.T)


# 70 x 300     one 128-byte chunk per sample that is mostly pad SNPs; a ragged second tile (samples 64 .. 69)
# 130 x 1000   two chunks; three tiles, the last of two samples
# 257 x 2100   P_pad / 4 = 576 is not a multiple of 128: the pitch is rounded up to 640; five chunks, five tiles, the last of one sample
SHAPES = {"70x300": (70, 300, 1), "130x1000": (130, 1000, 2), "257x2100": (257, 2100, 3)}
NOCALL, HOM = 44, 9


def planted(N):
    po = [(0, 2), (1, 2), (0, 3), (1, 3), (33, 40), (36, 40), (33, 41), (36, 41)]
    return dict(po=po, fs=[(2, 3), (40, 41)], dup=[(4, 5), (6, N - 1), (7, 48)])


# ---- the yardstick -------------------------------------------------------------------------------------------------
def rel_numpy(codes):
    """counts[N][N][6] (shared, ibs0, hethet, het_i, het_j, D) and phi[N][N] for every ordered pair, the diagonal included."""
    x = np.array([2.0, 0.0, 1.0, 0.0])[codes].T  # (N, P); 0 where missing
    m = (codes != 1).astype(np.float64).T
    h = (codes == 2).astype(np.float64).T
    a0 = (codes == 3).astype(np.float64).T
    a2 = (codes == 0).astype(np.float64).T
    q = x * x
    prods = dict(xm=x @ m.T, qm=q @ m.T, xx=x @ x.T, mm=m @ m.T, hh=h @ h.T, opp=a0 @ a2.T + a2 @ a0.T)
    assert max(a.max() for a in prods.values()) < 2.0 ** 53
    xm, qm, xx, mm, hh, opp = (prods[k].astype(np.int64) for k in ("xm", "qm", "xx", "mm", "hh", "opp"))
    het = 2 * xm - qm          # het[i][j]: heterozygous calls of i among the SNPs j is called at
    D = qm + qm.T - 2 * xx
    hmin = np.minimum(het, het.T)
    with np.errstate(invalid="ignore", divide="ignore"):
        phi = (2 * hmin - D).astype(np.float64) / (4 * hmin).astype(np.float64)
    phi[hmin == 0] = np.nan
    counts = np.stack([mm, opp, hh, het, het.T, D], axis=-1)
    assert counts.min() >= 0 and counts.max() < 2 ** 32
    return np.ascontiguousarray(counts.astype(np.uint32)), phi


def classify_numpy(phi, counts, po_ibs0=PO_IBS0):
    """include/fpca.h: 255 no value, 5 duplicate, 1 parent-offspring / 2 full sibs, 3 second, 4 third degree, 0 unrelated."""
    shared, ibs0 = counts[..., 0].astype(np.float64), counts[..., 1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = ibs0 / shared
        t = np.select([np.isnan(phi) | (shared == 0), phi > 0.354, (phi > 0.177) & (frac < po_ibs0), phi > 0.177, phi > 0.0884, phi > 0.0442],
                      [255, 5, 1, 2, 3, 4], 0)
    return t.astype(np.uint8)


def table_numpy(counts, phi, thr, min_shared=0, keep=None, po_ibs0=PO_IBS0):
    """The table of Context.king_related, restated: pairs i < j with phi > thr and shared >= min_shared among the kept, sorted by (i, j)."""
    with np.errstate(invalid="ignore"):
        above = np.triu(phi > thr, 1)  # (NaN: never)
    above &= counts[..., 0] >= min_shared
    if keep is not None:
        above &= keep[:, None] & keep[None, :]
    i, j = np.nonzero(above)  # row-major: sorted by (i, j)
    c = counts[i, j]
    ci = c.astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ibs = 1.0 - (ci[:, 5] - 2 * ci[:, 1]).astype(np.float64) / (2 * ci[:, 0]).astype(np.float64)
    return dict(i=i.astype(np.uint32), j=j.astype(np.uint32), phi=phi[i, j], shared=c[:, 0], ibs0=c[:, 1], hethet=c[:, 2], het_i=c[:, 3],
                het_j=c[:, 4], dist=c[:, 5], ibs=ibs, type=classify_numpy(phi[i, j], c, po_ibs0))


FIELDS = ("i", "j", "phi", "shared", "ibs0", "hethet", "het_i", "het_j", "dist", "ibs", "type")


def cutoff_numpy(N, i, j, keep=None):
    """The rule of include/fpca.h on a list of pairs: while an edge remains the sample of largest current degree goes, the largest index
    among equals."""
    keep = np.ones(N, dtype=bool) if keep is None else np.asarray(keep, dtype=bool).copy()
    A = np.zeros((N, N), dtype=bool)
    A[i, j] = True
    A = (A | A.T) & keep[:, None] & keep[None, :]
    deg = A.sum(axis=1)
    while deg.max() > 0:
        v = N - 1 - int(np.argmax(deg[::-1]))  # the last index holding the maximum
        keep[v] = False
        deg -= A[:, v]
        A[v, :] = A[:, v] = False
        deg[v] = 0
    return keep


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same_table(got, want):
    return set(got) == set(FIELDS) and all(same(got[k], want[k]) for k in FIELDS)


_CASE = {}


def case(name):
    """One generated shape: codes, counts and phi of every pair from numpy -- computed once and left unchanged."""
    if name not in _CASE:
        N, P, seed = SHAPES[name]
        codes = pedigree_codes(N, P, seed)
        counts, phi = rel_numpy(codes)
        counts.setflags(write=False)
        phi.setflags(write=False)
        _CASE[name] = dict(N=N, P=P, codes=codes, counts=counts, phi=phi, packed=pack_codes(codes))
    return _CASE[name]


def open_case(fp, c, accum="fp64"):
    return fp.Context.from_packed(c["packed"], c["N"], c["P"], accum=accum)


def rectangles(N):
    """Six rectangles off the 64-sample tiles and the 32-sample blocks; three reach below the diagonal, one is a single pair."""
    return [(5, 40, 3, N - 10), (33, N - 33, 0, 31), (N - 7, 7, N - 10, 10), (0, 1, N - 1, 1), (N - 1, 1, 0, N), (31, 34, 31, 34)]


def preclear(N):
    pre = np.random.default_rng(7).random(N) >= 0.3  # a pre-cleared random 30 %
    pre[[0, 2, 4, 5]] = True
    pre[3] = False
    return pre


# ---- 1. blocks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_counts_block_equals_direct_counting(fp, name):
    c = case(name)
    N, P, ref, rphi = c["N"], c["P"], c["counts"], c["phi"]
    calls = (c["codes"] != 1).sum(axis=0)
    # the yardstick itself: what a diagonal and the row of a sample without calls hold
    d = np.arange(N)
    assert np.array_equal(ref[d, d, 0], calls) and not ref[d, d, 1].any() and not ref[d, d, 5].any()
    assert not ref[NOCALL, :, 0].any() and np.isnan(rphi[NOCALL]).all() and np.isnan(rphi[HOM]).all()
    with open_case(fp, c) as ctx:
        got, phi = ctx.king_counts_block(0, N, 0, N)
        old = ctx.king_block(0, N, 0, N)
        eq_c, eq_p, eq_o = same(got, ref), same(phi, rphi), same(phi, old)
        print("%s king_counts_block(0, %d, 0, %d): counts equal to direct counting %s; phi equal to numpy %s, to king_block %s; ibs0 up to %d, "
              "shared %d .. %d off the no-call sample" % (name, N, N, eq_c, eq_p, eq_o, got[..., 1].max(), np.delete(got[..., 0], NOCALL, 0).min(), P))
        assert eq_c, (name, np.argwhere(got != ref)[:5])
        assert eq_p and eq_o
        # symmetry with het_i / het_j exchanged; the diagonal; the sample without a call
        assert np.array_equal(got, got.transpose(1, 0, 2)[..., [0, 1, 2, 4, 3, 5]])
        assert np.array_equal(got[d, d, 0], calls) and not got[d, d, 1].any() and not got[d, d, 5].any()
        assert np.array_equal(got[d, d, 2], got[d, d, 3]) and np.array_equal(got[d, d, 3], got[d, d, 4])  # h h = het on the diagonal
        assert not got[NOCALL, :, 0].any() and not got[:, NOCALL, 0].any() and np.isnan(phi[NOCALL]).all() and np.isnan(phi[:, NOCALL]).all()
        for i0, ni, j0, nj in rectangles(N):
            got, phi = ctx.king_counts_block(i0, ni, j0, nj)
            eq = same(got, np.ascontiguousarray(ref[i0:i0 + ni, j0:j0 + nj])) and same(phi, np.ascontiguousarray(rphi[i0:i0 + ni, j0:j0 + nj]))
            eq_o = same(phi, ctx.king_block(i0, ni, j0, nj))
            print("%s king_counts_block(%d, %d, %d, %d): equal to numpy %s, phi equal to king_block %s" % (name, i0, ni, j0, nj, eq, eq_o))
            assert eq and eq_o, (name, i0, ni, j0, nj)


# ---- 2. lists and masks ----------------------------------------------------------------------------------------------
# pairs the yardstick lists at min_shared = 0, floor(0.9 P), P, P + 1 (all samples): every filter value bites, none but the last is vacuous
CONDITIONS = {("257x2100", -1.0): [32385, 28680, 24976, 0], ("70x300", 0.1): [21, 18, 14, 0]}


@pytest.mark.parametrize("name", list(SHAPES))
def test_related_and_cutoff_shared(fp, name):
    c = case(name)
    N, P, counts, phi = c["N"], c["P"], c["counts"], c["phi"]
    pre = preclear(N)
    filters = [0, (9 * P) // 10, P, P + 1]
    with open_case(fp, c, accum="auto") as ctx:
        for thr in (0.3, 0.1, -1.0):
            sizes = []
            for label, keep in (("all", None), ("70%", pre)):
                for ms in filters:
                    want = table_numpy(counts, phi, thr, ms, keep)
                    got = ctx.king_related(thr, keep=keep, min_shared=ms)
                    eq = same_table(got, want)
                    print("%s thr %g keep=%s min_shared %d: yardstick lists %d pairs, the device %d, tables equal: %s" % (
                        name, thr, label, ms, want["i"].size, got["i"].size, eq))
                    assert eq, (name, thr, label, ms)
                    if keep is None:
                        sizes.append(want["i"].size)
                    else:
                        assert pre[got["i"]].all() and pre[got["j"]].all()
                    if ms == 0:  # exactly king_pairs' list
                        old = ctx.king_pairs(thr, keep=keep)
                        assert same(got["i"], old[0]) and same(got["j"], old[1]) and same(got["phi"], old[2]), (name, thr, label)
                # the masks
                m0, mold = ctx.king_cutoff_shared(thr, 0, keep=keep), ctx.king_cutoff(thr, keep=keep)
                ms = filters[1]
                w = table_numpy(counts, phi, thr, ms, keep)
                wmask, gmask = cutoff_numpy(N, w["i"], w["j"], keep), ctx.king_cutoff_shared(thr, ms, keep=keep)
                print("%s thr %g keep=%s: cutoff_shared(0) keeps %d, king_cutoff %d, equal %s; min_shared %d keeps %d, the restated rule %d, equal %s" % (
                    name, thr, label, m0.sum(), mold.sum(), np.array_equal(m0, mold), ms, gmask.sum(), wmask.sum(), np.array_equal(gmask, wmask)))
                assert m0.dtype == np.bool_ and np.array_equal(m0, mold) and np.array_equal(gmask, wmask), (name, thr, label)
                if keep is not None:
                    assert not gmask[~pre].any()
            if (name, thr) in CONDITIONS:
                assert sizes == CONDITIONS[(name, thr)], sizes
            assert sizes[0] >= sizes[1] >= sizes[2] > sizes[3] == 0, sizes  # (nobody shares P + 1 SNPs)


def test_slabs_and_the_general_path_change_nothing(fp, monkeypatch):
    """The test build's switches: the triangle in slabs of 64 and 128 rows, and the seven-product path forced where the two-product path
    would run -- the same tables, masks and block bits."""
    c = case("257x2100")
    N, P, counts, phi = c["N"], c["P"], c["counts"], c["phi"]
    ms = (9 * P) // 10
    want = {(thr, m): table_numpy(counts, phi, thr, m) for thr in (0.1, -1.0) for m in (0, ms)}
    w = want[(0.1, ms)]
    wmask = cutoff_numpy(N, w["i"], w["j"])
    with fp.test_hooks():
        with open_case(fp, c) as ctx:
            for rows in ("64", "128", "100000"):
                monkeypatch.setenv("FPCA_KING_SLAB_ROWS", rows)
                for key, wt in want.items():
                    got = ctx.king_related(key[0], min_shared=key[1])
                    print("slabs of %s rows, thr %g, min_shared %d: %d pairs, equal to the yardstick: %s" % (rows, key[0], key[1], got["i"].size, same_table(got, wt)))
                    assert same_table(got, wt)
                assert np.array_equal(ctx.king_cutoff_shared(0.1, ms), wmask)
            monkeypatch.delenv("FPCA_KING_SLAB_ROWS")
            monkeypatch.setenv("FPCA_KING_FORCE_GENERAL", "1")
            got = ctx.king_related(-1.0, min_shared=ms)
            blk, bphi = ctx.king_counts_block(0, N, 0, N)
            monkeypatch.delenv("FPCA_KING_FORCE_GENERAL")
            print("forced general path: %d pairs, table equal %s, counts equal %s, phi equal %s" % (
                got["i"].size, same_table(got, want[(-1.0, ms)]), same(blk, counts), same(bphi, phi)))
            assert same_table(got, want[(-1.0, ms)]) and same(blk, counts) and same(bphi, phi)


def test_two_product_path_gives_the_same_integers(fp):
    """A source without a single missing call: every block takes the x.x / h.h path, pad SNPs on both sides."""
    N, P = 100, 700
    rng = np.random.default_rng(21)
    d = rng.binomial(2, rng.uniform(0.1, 0.9, P)[None, :], (N, P))
    d[50] = d[10]
    codes = np.ascontiguousarray(np.array([3, 2, 0], dtype=np.uint8)[d].T)
    counts, phi = rel_numpy(codes)
    assert phi[10, 50] == 0.5 and np.isfinite(phi).all() and (counts[..., 0] == P).all() and counts[..., 1].max() > 0
    with fp.Context.from_packed(pack_codes(codes), N, P) as ctx:
        got, gphi = ctx.king_counts_block(0, N, 0, N)
        lst = ctx.king_related(0.0)
    want = table_numpy(counts, phi, 0.0)
    print("no missing call: counts equal to numpy %s, phi %s, %d pairs above 0, table equal %s" % (same(got, counts), same(gphi, phi), lst["i"].size, same_table(lst, want)))
    assert same(got, counts) and same(gphi, phi) and same_table(lst, want) and lst["i"].size > 0


def test_overflow_names_the_count(fp):
    c = case("130x1000")
    ms = (9 * c["P"]) // 10
    need = table_numpy(c["counts"], c["phi"], 0.1, ms)["i"].size
    assert need > 3
    with open_case(fp, c) as ctx:
        with pytest.raises(fp.FpcaError, match="%d pairs qualify, the arrays hold 3" % need) as e:
            ctx.king_related(0.1, min_shared=ms, max_pairs=3)
        assert e.value.code == ENOMEM
        n = C.c_uint64(0)
        i, j, p, k = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint32), np.zeros(3), np.zeros((3, 6), dtype=np.uint32)
        rc = fp.lib().fpca_king_related(ctx.h, None, 0.1, ms, 3, i.ctypes.data, j.ctypes.data, p.ctypes.data, k.ctypes.data, C.byref(n))
        assert rc == ENOMEM and n.value == need and not i.any() and not k.any()  # the arrays are not written
        assert ctx.king_related(0.1, min_shared=ms, max_pairs=need)["i"].size == need  # exactly enough room
    print("overflow: %d pairs needed against 3: refused with the count" % need)


# ---- 3. types ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_types_on_the_pedigrees(fp, name):
    c = case(name)
    N, counts, phi = c["N"], c["counts"], c["phi"]
    types = classify_numpy(phi, counts)
    iu = np.triu_indices(N, 1)
    tu = types[iu]
    pl = planted(N)
    frac = counts[..., 1] / np.maximum(counts[..., 0], 1)
    print("%s yardstick: dup %d, parent-offspring %d, full sibs %d, second %d, third %d, no value %d; IBS0 fraction of the sibs %s" % (
        name, (tu == 5).sum(), (tu == 1).sum(), (tu == 2).sum(), (tu == 3).sum(), (tu == 4).sum(), (tu == 255).sum(),
        ", ".join("%.4f" % frac[a, b] for a, b in pl["fs"])))
    assert ((tu == 5).sum(), (tu == 1).sum(), (tu == 2).sum()) == (3, 8, 2)
    for a, b in pl["po"]:
        assert types[a, b] == 1 and counts[a, b, 1] == 0, (a, b)
    for a, b in pl["fs"]:
        assert types[a, b] == 2 and 0.010 <= frac[a, b] <= 0.024, (a, b, frac[a, b])
    for a, b in pl["dup"]:
        assert types[a, b] == 5 and counts[a, b, 1] == 0 and counts[a, b, 5] == 0, (a, b)
    with open_case(fp, c) as ctx:
        t = ctx.king_related(0.177)
    got = {(int(a), int(b)): int(k) for a, b, k in zip(t["i"], t["j"], t["type"])}
    want = dict([(p, 1) for p in pl["po"]] + [(p, 2) for p in pl["fs"]] + [(p, 5) for p in pl["dup"]])
    print("%s device, phi > 0.177: %s" % (name, sorted(got.items())))
    assert got == want
    # a threshold of 1 makes every first-degree pair parent-offspring, 0 none: po_ibs0 reaches the classification
    with open_case(fp, c) as ctx:
        assert sorted(ctx.king_related(0.177, po_ibs0=1.0)["type"]) == [1] * 10 + [5] * 3
        assert sorted(ctx.king_related(0.177, po_ibs0=0.0)["type"]) == [2] * 10 + [5] * 3


# dup / parent-offspring / full sibs / second / third degree over the whole triangle and the fewest SNPs a pair shares, recorded on the
# CPU from the yardstick (consistent with GOLDEN of tests/test_gpu_king.py: 47 / 106 / 192 pairs above 0.177 / 0.0884 / 0.0442 for hapmap3_data)
GOLDEN = {
    "hapmap3_data": ((957, 14389), (0, 21, 26, 59, 86), 14080),
    "data_chr1": ((957, 1129), (2, 24, 36, 72, 2675), 1048),
    "hm3_thinned": ((957, 14079), (0, 21, 26, 60, 95), 13779),
    "kg_thinned": ((1092, 14079), (0, 10, 17, 14, 20), 14079),  # no missing call
}
_GOLD = {}


def golden(name):
    if name not in _GOLD:
        codes, N, P = read_bed_codes(os.path.join(GOLD, name))
        counts, phi = rel_numpy(codes)
        _GOLD[name] = dict(codes=codes, N=N, P=P, counts=counts, phi=phi)
    return _GOLD[name]


@pytest.mark.parametrize("name", list(GOLDEN))
def test_golden_filesets(fp, name):
    g = golden(name)
    (N, P), per_type, min_shared = GOLDEN[name]
    assert (g["N"], g["P"]) == (N, P)
    counts, phi = g["counts"], g["phi"]
    iu = np.triu_indices(N, 1)
    tu = classify_numpy(phi, counts)[iu]
    ref = tuple(int((tu == t).sum()) for t in (5, 1, 2, 3, 4))
    ref_min = int(counts[..., 0][iu].min())
    assert not (tu == 255).any()
    want = table_numpy(counts, phi, -1.0)  # every pair: none is NaN, none is at or below -1
    assert want["i"].size == N * (N - 1) // 2
    with fp.Context.from_bed(os.path.join(GOLD, name + ".bed"), N, accum="auto") as ctx:
        got = ctx.king_related(-1.0)
    dev = tuple(int((got["type"] == t).sum()) for t in (5, 1, 2, 3, 4))
    print("%s: yardstick dup / PO / FS / 2nd / 3rd %s, fewest shared %d; the device %s, %d; whole-triangle tables equal %s" % (
        name, ref, ref_min, dev, got["shared"].min(), same_table(got, want)))
    assert ref == per_type and ref_min == min_shared, (name, ref, ref_min)
    assert same_table(got, want) and dev == per_type and int(got["shared"].min()) == min_shared
    # the fileset entry point, at its default threshold: third degree and closer
    t = fp.king_related(os.path.join(GOLD, name))
    assert same_table(t, table_numpy(counts, phi, 0.0442)) and t["i"].size == sum(per_type)


# ---- 4. flashpca(unrelated=, unrelated_min_shared=) --------------------------------------------------------------------------
def test_flashpca_unrelated_min_shared(fp):
    g = golden("hapmap3_data")
    N, P, counts, phi = g["N"], g["P"], g["counts"], g["phi"]
    assert P == 14389
    a = fp.flashpca(HM3, ndim=5, unrelated=0.0884)
    b = fp.flashpca(HM3, ndim=5, unrelated=0.0884, unrelated_min_shared=0)
    assert set(a) == set(b)
    for key in a:
        if key != "info":
            assert same(a[key], b[key]), key
    w = table_numpy(counts, phi, 0.0884, P)
    wmask = cutoff_numpy(N, w["i"], w["j"])
    r = fp.flashpca(HM3, ndim=5, unrelated=0.0884, unrelated_min_shared=P)
    print("flashpca(unrelated=0.0884): %d of %d kept; unrelated_min_shared=0 the same arrays; unrelated_min_shared=%d: %d pairs of 106 left, %d kept, "
          "mask equal to the restated one %s" % (a["unrelated_kept"].sum(), N, P, w["i"].size, r["unrelated_kept"].sum(), np.array_equal(r["unrelated_kept"], wmask)))
    assert a["unrelated_kept"].sum() == 887 and w["i"].size < 106  # (the filter bites: no pair of the fileset shares all P SNPs)
    assert np.array_equal(r["unrelated_kept"], wmask) and wmask.sum() > 887 and r["vectors"].shape == (int(wmask.sum()), 5)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(fp):
    c = case("70x300")
    N = c["N"]

    def refused(call, msg, code=-1):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == code
        print("refused: %s" % str(e.value)[:110])

    with open_case(fp, c) as ctx:
        refused(lambda: ctx.king_counts_block(0, N + 1, 0, N), "are not a non-empty rectangle")
        refused(lambda: ctx.king_counts_block(3, 0, 0, N), "are not a non-empty rectangle")
        refused(lambda: ctx.king_related(float("nan")), "fpca_king_related: the threshold is NaN")
        refused(lambda: ctx.king_cutoff_shared(float("nan")), "fpca_king_cutoff_shared: the threshold is NaN")
        L = fp.lib()
        assert L.fpca_king_counts_block(ctx.h, 0, N, 0, N, None, None) == -1 and L.fpca_king_cutoff_shared(ctx.h, 0.1, 0, None, None) == -1
        assert L.fpca_king_related(ctx.h, None, 0.1, 0, 5, None, None, None, None, None) == -1
        with pytest.raises(ValueError):
            ctx.king_related(0.1, keep=np.ones(N - 1, dtype=bool))
        with pytest.raises(ValueError):
            ctx.king_related(0.1, min_shared=-1)
        ctx.set_sample_mask(np.arange(N) % 3 != 0)
        for call, fn in ((lambda: ctx.king_counts_block(0, N, 0, N), "fpca_king_counts_block"), (lambda: ctx.king_related(0.1), "fpca_king_related"),
                         (lambda: ctx.king_cutoff_shared(0.1), "fpca_king_cutoff_shared")):
            refused(call, fn + ": a sample mask is set .* pass the mask as `keep` instead")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        for call in (lambda: ctx.king_counts_block(0, N, 0, N), lambda: ctx.king_related(0.1), lambda: ctx.king_cutoff_shared(0.1)):
            refused(call, "one shard of several")
        ctx.set_rank(1, 0)
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.king_counts_block(0, 50, 0, 50), "fpca_king_counts_block: this context holds a dense matrix")
        refused(lambda: dense.king_related(0.1), "fpca_king_related: this context holds a dense matrix")
    # above 1 GiB: 6,689^2 x 24 bytes of counts; 2^14 + 1 samples have 134 million pairs x 24 bytes
    big_n = 2 ** 14 + 1
    with fp.Context.from_packed(np.full(((big_n + 3) // 4) * 2, 0xFF, dtype=np.uint8), big_n, 2) as wide:
        buf = np.zeros(6, dtype=np.uint32)
        assert fp.lib().fpca_king_counts_block(wide.h, 0, 6689, 0, 6689, buf.ctypes.data, None) == -1
        msg = fp.lib().fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "6689 x 6689 x 6 counts is over the limit of 1073741824 bytes" in msg
        n = C.c_uint64(0)
        assert fp.lib().fpca_king_related(wide.h, None, 0.1, 0, 1 << 40, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, C.byref(n)) == -1
        msg = fp.lib().fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "pairs x 6 counts is over the limit of 1073741824 bytes" in msg


# ---- 6. scratch ----------------------------------------------------------------------------------------------------------
# The pattern of tests/test_gpu_scratch.py, its _run restated: the live counts of the owners are back at the baseline after a success and
# after every injected FPCA_ENOMEM, the message names the entry point, and the first un-failed call returns what the first call returned.
SN, SP = 600, 520


@pytest.fixture(scope="module")
def env(built_lib):
    import flashpca_amd as fp

    with fp.test_hooks() as L:
        with fp.Context.synthetic(SN, SP, n_pop=4, missing_rate=0.01, accum="fp64") as ctx:
            rng = np.random.default_rng(11)
            yield dict(fp=fp, L=L, ctx=ctx, B=rng.standard_normal((SN, 16)), keep=rng.random(SN) < 0.7)
        L.fpca_debug_scratch_fail_at(0)


def _live(L):
    out = (C.c_uint64 * 3)()
    assert L.fpca_debug_scratch_live(out) == 0
    return tuple(int(v) for v in out)


def _state(ctx, B):
    ms, tr = ctx.stats()
    return ms, np.float64(tr), ctx.apply_xxt(B)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def _run(env, entry, call):
    """call() -> tuple of arrays; raises FpcaError on failure"""
    fp, L, ctx = env["fp"], env["L"], env["ctx"]
    L.fpca_debug_scratch_fail_at(0)
    before = _live(L)
    ref = call()
    base = _live(L)
    assert base == before, "%s leaks on the success path: %s -> %s" % (entry, before, base)
    state = _state(ctx, env["B"])
    assert _live(L) == base
    first_ok, out = None, None
    for n in range(1, 66):
        assert L.fpca_debug_scratch_fail_at(n) == 0
        try:
            out = call()
        except fp.FpcaError as e:
            assert e.code == ENOMEM, "%s, acquisition %d: %s" % (entry, n, e)
            assert entry in str(e), "%s, acquisition %d: the message does not name the entry point: %s" % (entry, n, e)
            assert _live(L) == base, "%s leaks when acquisition %d fails: %s -> %s" % (entry, n, base, _live(L))
            continue
        finally:
            L.fpca_debug_scratch_fail_at(0)
        first_ok = n
        break
    print("%s: %d acquisitions" % (entry, (first_ok or 0) - 1))
    assert first_ok is not None and 2 <= first_ok <= 64, "%s: first success at n = %s" % (entry, first_ok)
    assert _live(L) == base
    assert _same(out, ref), "%s: the results after the injected failures differ" % entry
    assert _same(_state(ctx, env["B"]), state), "%s: the context's statistics or operator changed" % entry


def test_scratch_is_given_back(env):
    ctx = env["ctx"]
    _run(env, "fpca_king_counts_block", lambda: ctx.king_counts_block(3, 130, 60, 200))

    def related():
        t = ctx.king_related(-0.05, keep=env["keep"], min_shared=500)
        assert t["i"].size > 0
        return tuple(t[k] for k in FIELDS)

    _run(env, "fpca_king_related", related)
    _run(env, "fpca_king_cutoff_shared", lambda: (ctx.king_cutoff_shared(-0.02, 500, keep=env["keep"]),))

    def bench():
        ms, macs = ctx.bench_king_rel(2)
        return np.all(ms > 0), macs

    _run(env, "fpca_bench_king_rel", bench)
