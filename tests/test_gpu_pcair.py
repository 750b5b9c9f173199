"""PC-AiR's partition (fpca_king_census / fpca_pcair_king / fpca_pcair_pairs; Context.king_census / pcair_partition, pcair_partition(),
pcair()) on the GPU against restatements that never call the feature (tests/pcair_yardstick.py): the census is counted from king_numpy's
phi matrix (tests/test_gpu_king.py; it equals the device's phi bit for bit, so the classes of every pair are the device's) and the rule is
a plain-Python loop written from include/fpca.h.  Everything is array_equal: no tolerance, no pair left out.
The data is a two-population version of test_gpu_king.py's pedigree on its three shapes (Balding-Nichols, F = 0.1, the first 3N/5 samples
in population A): related, divergent and NaN pairs all occur, which every case asserts in the yardstick before it compares.  Every test
prints what it measured (pytest -s).
Measured on the MI355X: at +-2^-5.5 the shapes hold 308 / 1,571 / 137, 568 / 5,494 / 257 and 912 / 20,131 / 511 related / divergent / NaN
pairs; every census (5 threshold pairs x {all, 30 % pre-cleared} x 3 shapes, and with an exclusion list of 250 pairs that removes 350 - 376
divergent credits) equals the yardstick's; slabs of 64 / 128 rows and the forced five-product path change nothing; the partition keeps
32 of 70, 69 of 130 and 161 of 257, equal to the restated rule, with removals decided at every one of its four levels; on hapmap3_data
(maf 0.05: 13,964 SNPs) 396 related and 348,366 divergent pairs, pcair keeps 819 of 957, its second round (1,194 PC-Relate pairs) 808,
king_cutoff(2^-5.5) 820.  The 14 tests take 2.8 s together."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from pcair_yardstick import census_numpy, classes_numpy, partition_python, pcair_codes
from test_gpu_king import SHAPES, king_numpy, pack_codes, pairs_numpy, read_bed_codes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
ENOMEM = -4
T = 2 ** -5.5
INF = float("inf")
THRESHOLDS = [(T, -T), (0.1, -0.1), (INF, -T), (-1.0, -2.0), (-0.1, 0.1)]


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


_CASE = {}


def case(name):
    """One generated shape: codes, phi of every pair from numpy, a pre-cleared 30 % -- computed once and left unchanged."""
    if name not in _CASE:
        N, P, seed = SHAPES[name]
        codes, planted = pcair_codes(N, P, seed)
        pre = np.random.default_rng(7).random(N) >= 0.3
        pre[[0, 2, 4, 5]] = True
        pre[3] = False
        _CASE[name] = dict(N=N, P=P, codes=codes, phi=king_numpy(codes), packed=pack_codes(codes), pre=pre, **planted)
        rel, div, nan = classes_numpy(_CASE[name]["phi"], T, -T)
        print("%s at +-2^-5.5: %d related, %d divergent, %d NaN pairs of %d" % (name, rel.sum(), div.sum(), nan.sum(), N * (N - 1) // 2))
    return _CASE[name]


def open_case(fp, c, accum="fp64"):
    return fp.Context.from_packed(c["packed"], c["N"], c["P"], accum=accum)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def not_vacuous(c, keep=None):
    rel, div, nan = classes_numpy(c["phi"], T, -T, keep)
    assert rel.sum() > 0 and div.sum() > 0 and nan.sum() > 0, (rel.sum(), div.sum(), nan.sum())
    return rel, div, nan


def exclusion_list(c, seed):
    """200 random pairs (either order) and 50 of the yardstick's divergent pairs at +-2^-5.5."""
    N = c["N"]
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N, 200)
    b = (a + 1 + rng.integers(0, N - 1, 200)) % N
    di, dj = np.nonzero(classes_numpy(c["phi"], T, -T)[1])
    pick = rng.choice(di.size, 50, replace=False)
    return np.concatenate([a, dj[pick]]), np.concatenate([b, di[pick]])  # the divergent ones listed larger index first


# ---- 1. the census, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_census_bit_for_bit(fp, name):
    c = case(name)
    N, ref, pre = c["N"], c["phi"], c["pre"]
    not_vacuous(c)
    not_vacuous(c, pre)
    ex = exclusion_list(c, 3)
    with open_case(fp, c, accum="auto") as ctx:  # (the int8 mode's own sample-major copy may be resident: it is not what the call reads)
        B = np.random.default_rng(4).standard_normal((N, 16))
        before = ctx.apply_xt(B)
        for kin_thr, div_thr in THRESHOLDS:
            for label, keep in (("all", None), ("70%", pre)):
                want = census_numpy(ref, kin_thr, div_thr, keep)
                got = ctx.king_census(kin_thr, div_thr, keep=keep)
                eq = same(got[0], want[0]) and same(got[1], want[1])
                print("%s (%g, %g) keep=%s: yardstick %d related / %d divergent credits, the device %d / %d, equal: %s" % (
                    name, kin_thr, div_thr, label, want[0].sum(), want[1].sum(), got[0].sum(), got[1].sum(), eq))
                assert eq, (name, kin_thr, div_thr, label)
                if keep is not None:
                    assert not got[0][~pre].any() and not got[1][~pre].any()  # cleared samples count 0
        # (-1, -2): everything with a value is related, nothing is divergent; (-0.1, 0.1): the thresholds cross and related wins
        r, d = ctx.king_census(-1.0, -2.0)
        nvalid = N - 2
        assert not d.any() and r.sum() == nvalid * (nvalid - 1) and r[c["hom"]] == 0 and r[c["nocall"]] == 0
        r, d = census_numpy(ref, -0.1, 0.1)
        assert r.sum() > 0 and d.sum() > 0
        with np.errstate(invalid="ignore"):
            assert d.sum() == 2 * np.triu(ref <= -0.1, 1).sum()  # only what is not related is left to be divergent
        # the exclusion list
        for label, keep in (("all", None), ("70%", pre)):
            base = ctx.king_census(T, -T, keep=keep)
            want = census_numpy(ref, T, -T, keep, exclude=ex)
            got = ctx.king_census(T, -T, keep=keep, exclude=ex)
            removed = int(base[1].sum()) - int(got[1].sum())
            print("%s keep=%s: an exclusion list of %d pairs removes %d divergent credits; equal to the yardstick: %s" % (
                name, label, ex[0].size, removed, same(got[0], want[0]) and same(got[1], want[1])))
            assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[0], base[0])
            if keep is None:
                assert removed >= 50
        # the same pairs listed twice, and reversed: nothing changes
        once = ctx.king_census(T, -T, exclude=ex)
        twice = ctx.king_census(T, -T, exclude=(np.concatenate([ex[0], ex[1]]), np.concatenate([ex[1], ex[0]])))
        assert same(once[0], twice[0]) and same(once[1], twice[1])
        after = ctx.apply_xt(B)
        assert np.array_equal(before, after)  # the context computes what it computed


# ---- 2. slabs and paths -----------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
d = np.load(sys.argv[2])
for k, v in json.loads(sys.argv[3]).items():
    os.environ[k] = v
out = {}
with fp.test_hooks():
    with fp.Context.from_packed(d["packed"], int(d["N"]), int(d["P"])) as ctx:
        ex = (d["ei"], d["ej"])
        out["rel"], out["div"] = ctx.king_census(float(d["kin_thr"]), float(d["div_thr"]), keep=d["keep"], exclude=ex)
        out["mask"], out["prel"], out["pdiv"] = ctx.pcair_partition(float(d["kin_thr"]), float(d["div_thr"]), counts=True)
np.savez(sys.argv[4], **out)
print("CHILD ok")
"""


def test_slabs_and_the_general_path_change_nothing(fp):
    """The test build's switches, each in a child process: the triangle in slabs of 64 and 128 rows (five and three launches over the 257
    samples where the default is one), and the five-product path forced where the x.x-only path would run (the even 32-sample blocks
    hold no missing call) -- the arrays of the default, which two calls in one process give twice."""
    c = case("257x2100")
    N, P, pre = c["N"], c["P"], c["pre"]
    not_vacuous(c, pre)
    ex = exclusion_list(c, 5)
    with open_case(fp, c) as ctx:
        first = ctx.king_census(T, -T, keep=pre, exclude=ex) + ctx.pcair_partition(T, -T, counts=True)
        second = ctx.king_census(T, -T, keep=pre, exclude=ex) + ctx.pcair_partition(T, -T, counts=True)
    assert all(same(a, b) for a, b in zip(first, second))
    want = census_numpy(c["phi"], T, -T, pre, exclude=ex)
    assert same(first[0], want[0]) and same(first[1], want[1])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.npz")
        np.savez(src, packed=c["packed"], N=N, P=P, keep=pre, ei=ex[0], ej=ex[1], kin_thr=T, div_thr=-T)
        for label, switches in (("slabs of 64 rows", {"FPCA_KING_SLAB_ROWS": "64"}), ("slabs of 128 rows", {"FPCA_KING_SLAB_ROWS": "128"}),
                                ("the general path forced", {"FPCA_KING_FORCE_GENERAL": "1"})):
            out = os.path.join(tmp, "out.npz")
            r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, src, json.dumps(switches), out], capture_output=True, text=True, env=env, timeout=120)
            assert r.returncode == 0 and "CHILD ok" in r.stdout, r.stderr[-2000:]
            res = dict(np.load(out))
            eq = all(same(res[k], v) for k, v in zip(("rel", "div", "mask", "prel", "pdiv"), first))
            print("%s: census, mask and the partition's counts equal to the default's: %s" % (label, eq))
            assert eq, label


# ---- 3. the fused list and the partition -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_partition_from_the_fused_pass(fp, name):
    c = case(name)
    N, ref, pre = c["N"], c["phi"], c["pre"]
    with open_case(fp, c) as ctx:
        for kin_thr, div_thr in ((T, -T), (0.1, -0.1)):
            for label, keep in (("all", None), ("70%", pre)):
                rel = classes_numpy(ref, kin_thr, div_thr, keep)[0]
                assert rel.sum() > 0
                mask, n_rel, n_div = ctx.pcair_partition(kin_thr, div_thr, keep=keep, counts=True)
                i, j, phi = ctx.king_pairs(kin_thr, keep=keep)
                listed = (np.bincount(i, minlength=N) + np.bincount(j, minlength=N)).astype(np.uint32)
                wrel, wdiv = census_numpy(ref, kin_thr, div_thr, keep)
                yi, yj, yphi = pairs_numpy(ref, kin_thr, keep)
                decided = {}
                want = partition_python(N, yi, yj, yphi, wdiv, np.ones(N, dtype=bool) if keep is None else keep, decided)
                print("%s (%g, %g) keep=%s: %d related pairs, the partition keeps %d of %d (the rule restated %d; decided by %s); masks equal: %s" % (
                    name, kin_thr, div_thr, label, i.size, mask.sum(), N if keep is None else keep.sum(), want.sum(), decided, np.array_equal(mask, want)))
                assert same(n_rel, listed) and same(n_rel, wrel) and same(n_div, wdiv)
                assert mask.dtype == np.bool_ and np.array_equal(mask, want), (name, kin_thr, label)
                both = rel | rel.T
                assert not both[np.ix_(mask, mask)].any()  # no pair among the kept samples is related
                assert 0 < mask.sum() < N
                if keep is not None:
                    assert not mask[~pre].any()  # a cleared entry stays cleared
                assert np.array_equal(ctx.pcair_partition(kin_thr, div_thr, keep=keep), mask)  # counts=False: the mask alone


# ---- 4. relatives from outside ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_partition_from_outside_pairs(fp, name):
    c = case(name)
    N, ref, pre = c["N"], c["phi"], c["pre"]
    not_vacuous(c)
    yi, yj, yphi = pairs_numpy(ref, 0.2)
    assert yi.size >= 5
    # the issue's case, and the same with 30 of the yardstick's divergent pairs listed as relatives too (kin 2^-4): those must leave n_div
    di, dj = np.nonzero(classes_numpy(ref, T, -T)[1])
    pick = np.random.default_rng(9).choice(di.size, 30, replace=False)
    more = (np.concatenate([yi, dj[pick].astype(np.uint32)]), np.concatenate([yj, di[pick].astype(np.uint32)]), np.concatenate([yphi, np.full(30, 0.0625)]))
    with open_case(fp, c) as ctx:
        plain = ctx.king_census(INF, -T)[1]
        for what, pairs in (("pairs above 0.2", (yi, yj, yphi)), ("plus 30 divergent pairs", more)):
            for label, keep in (("all", None), ("70%", pre)):
                got = ctx.pcair_partition(kin_thr=123.0, div_thr=-T, keep=keep, kin_pairs=pairs, counts=True)  # (kin_thr is unused)
                wdiv = census_numpy(ref, INF, -T, keep, exclude=(pairs[0], pairs[1]))[1]
                want = partition_python(N, pairs[0], pairs[1], pairs[2], wdiv, np.ones(N, dtype=bool) if keep is None else keep)
                print("%s, %s, keep=%s: %d pairs, %d divergent credits, %d kept (restated %d); equal: %s" % (
                    name, what, label, pairs[0].size, got[2].sum(), got[0].sum(), want.sum(), np.array_equal(got[0], want) and same(got[2], wdiv)))
                assert got[1] is None and same(got[2], wdiv) and np.array_equal(got[0], want)
                if keep is None:
                    assert int(plain.sum()) - int(got[2].sum()) == (0 if pairs is not more else 60)
                    assert not (got[0][pairs[0]] & got[0][pairs[1]]).any()  # no listed pair is left whole
                else:
                    assert not got[0][~pre].any()


# ---- 5. overflow and refusals -----------------------------------------------------------------------------------------------
def test_overflow_names_the_count(fp, monkeypatch):
    c = case("130x1000")
    need = int(classes_numpy(c["phi"], T, -T)[0].sum())
    assert need > 10
    with fp.test_hooks():
        monkeypatch.setenv("FPCA_KING_MAX_PAIRS", "10")
        with open_case(fp, c) as ctx:
            with pytest.raises(fp.FpcaError, match="fpca_pcair_king: %d pairs are above the threshold, the call keeps room for 10" % need) as e:
                ctx.pcair_partition(T, -T)
            assert e.value.code == ENOMEM
            few = int(classes_numpy(c["phi"], 0.3, -T)[0].sum())
            assert 0 < few <= 10
            yi, yj, yphi = pairs_numpy(c["phi"], 0.3)
            want = partition_python(c["N"], yi, yj, yphi, census_numpy(c["phi"], 0.3, -T)[1], np.ones(c["N"], dtype=bool))
            assert np.array_equal(ctx.pcair_partition(0.3, -T), want)  # no more than 10 pairs: served
            r, d = ctx.king_census(T, -T)  # the census alone keeps no list: nothing to overflow
            assert r.sum() == 2 * need
        monkeypatch.delenv("FPCA_KING_MAX_PAIRS")
    print("overflow: %d related pairs against the internal 10: refused with the count" % need)


def test_refusals(fp):
    c = case("70x300")
    N = c["N"]

    def refused(call, msg, code=-1):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == code
        print("refused: %s" % str(e.value)[:110])

    nan = float("nan")
    some = (np.array([0, 1], dtype=np.uint32), np.array([2, 3], dtype=np.uint32), np.array([0.25, 0.25]))
    with open_case(fp, c) as ctx:
        refused(lambda: ctx.king_census(nan, -T), "fpca_king_census: a threshold is NaN")
        refused(lambda: ctx.king_census(T, nan), "fpca_king_census: a threshold is NaN")
        refused(lambda: ctx.pcair_partition(nan, -T), "fpca_pcair_king: a threshold is NaN")
        refused(lambda: ctx.pcair_partition(T, nan), "fpca_pcair_king: a threshold is NaN")
        refused(lambda: ctx.pcair_partition(T, nan, kin_pairs=some), "fpca_pcair_pairs: a threshold is NaN")
        refused(lambda: ctx.king_census(exclude=([0, 1], [2, N])), "fpca_king_census: the exclusion list pair 1 names sample %d of %d" % (N, N))
        refused(lambda: ctx.king_census(exclude=([0, 5], [2, 5])), "fpca_king_census: the exclusion list pair 1 pairs sample 5 with itself")
        refused(lambda: ctx.pcair_partition(kin_pairs=([0, N], [2, 1], [0.25, 0.25])), "fpca_pcair_pairs: the kinship list pair 1 names sample %d of %d" % (N, N))
        refused(lambda: ctx.pcair_partition(kin_pairs=([0, 4], [2, 4], [0.25, 0.25])), "fpca_pcair_pairs: the kinship list pair 1 pairs sample 4 with itself")
        refused(lambda: ctx.pcair_partition(kin_pairs=([0], [2], [nan])), "fpca_pcair_pairs: the kinship of pair 0 is not finite")
        L = fp.lib()
        u32 = np.zeros(N, dtype=np.uint32)
        assert L.fpca_king_census(ctx.h, None, T, -T, None, None, 0, None, u32.ctypes.data) == -1
        assert L.fpca_king_census(ctx.h, None, T, -T, None, None, 3, u32.ctypes.data, u32.ctypes.data) == -1
        assert L.fpca_pcair_king(ctx.h, T, -T, None, None, None, None) == -1 and L.fpca_pcair_pairs(ctx.h, -T, 0, None, None, None, None, None, None) == -1
        for bad in (lambda: ctx.king_census(keep=np.ones(N + 1, dtype=bool)), lambda: ctx.pcair_partition(keep=np.ones(N - 1, dtype=bool)),
                    lambda: ctx.king_census(exclude=([0, 1], [2])), lambda: ctx.king_census(exclude=([-1], [2])),
                    lambda: ctx.pcair_partition(kin_pairs=([0], [2])), lambda: ctx.pcair_partition(kin_pairs=([0], [2], [0.25, 0.5]))):
            with pytest.raises(ValueError):
                bad()
        mask = np.arange(N) % 3 != 0
        ctx.set_sample_mask(mask)
        for call, fn in ((lambda: ctx.king_census(), "fpca_king_census"), (lambda: ctx.pcair_partition(), "fpca_pcair_king"),
                         (lambda: ctx.pcair_partition(kin_pairs=some), "fpca_pcair_pairs"), (lambda: ctx.bench_king_census(1), "fpca_bench_king_census")):
            refused(call, fn + ": a sample mask is set .* pass the mask as `keep` instead")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        for call in (lambda: ctx.king_census(), lambda: ctx.pcair_partition(), lambda: ctx.pcair_partition(kin_pairs=some)):
            refused(call, "one shard of several")
        ctx.set_rank(1, 0)
        # +inf is no refusal: no relatives from KING, everyone stays
        got = ctx.pcair_partition(INF, -T, counts=True)
        assert got[0].all() and not got[1].any() and same(got[2], census_numpy(c["phi"], INF, -T)[1])
        ms = ctx.bench_king_census(2)
        assert ms.shape == (2,) and np.all(ms > 0)
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.king_census(), "fpca_king_census: this context holds a dense matrix")
        refused(lambda: dense.pcair_partition(), "fpca_pcair_king: this context holds a dense matrix")
        refused(lambda: dense.pcair_partition(kin_pairs=some), "fpca_pcair_pairs: this context holds a dense matrix")


# ---- 6. the golden fileset ----------------------------------------------------------------------------------------------------
_HM3 = {}


def hm3_round1(fp):
    if "r" not in _HM3:
        _HM3["r"] = fp.pcair(HM3, ndim=5, maf=0.05)
    return _HM3["r"]


def test_golden_pcair_is_flashpca_on_the_partition(fp):
    r = hm3_round1(fp)
    N = 957
    snps, unrel = r["snps_kept"], r["unrelated_kept"]
    assert snps.dtype == np.bool_ and unrel.dtype == np.bool_ and unrel.shape == (N,) and 0 < snps.sum() < snps.size
    f = fp.flashpca(HM3, ndim=5, snps=snps, keep=unrel)
    for key in ("values", "vectors", "projection", "projection_all", "pve", "center", "scale"):
        assert f[key].shape == r[key].shape and np.array_equal(f[key], r[key], equal_nan=True), key
    assert f["loadings"] is None and r["loadings"] is None  # (not asked for)
    assert np.array_equal(f["snps_kept"], snps) and "unrelated_kept_1" not in r
    assert r["vectors"].shape == (int(unrel.sum()), 5) and r["projection_all"].shape == (N, 5)
    # the partition against the restatement on the compacted fileset, and the entry point that returns the mask alone
    codes = read_bed_codes(HM3)[0][snps]
    phi = king_numpy(codes)
    wrel, wdiv = census_numpy(phi, T, -T)
    yi, yj, yphi = pairs_numpy(phi, T)
    want = partition_python(N, yi, yj, yphi, wdiv, np.ones(N, dtype=bool))
    assert same(r["n_rel"], wrel) and same(r["n_div"], wdiv) and np.array_equal(unrel, want)
    assert np.array_equal(fp.pcair_partition(HM3, maf=0.05), unrel)
    with fp.Context.from_bed(HM3 + ".bed", N) as full:
        with full.snp_subset(snps) as sub:
            left = sub.king_pairs(T, keep=unrel)
            cut = sub.king_cutoff(T)
    assert left[0].size == 0  # no pair of the unrelated set is above the threshold
    assert r["n_div"].sum() > 0  # HapMap3 holds several continental groups: the fixture exercises divergence
    print("hapmap3_data, maf 0.05 (%d SNPs): %d related and %d divergent pairs at +-2^-5.5; pcair keeps %d of %d, king_cutoff(2^-5.5) keeps %d" % (
        snps.sum(), r["n_rel"].sum() // 2, r["n_div"].sum() // 2, unrel.sum(), N, cut.sum()))


def test_golden_second_round(fp):
    r1 = hm3_round1(fp)
    r = fp.pcair(HM3, ndim=5, maf=0.05, iterations=2)
    N = 957
    first, final = r["unrelated_kept_1"], r["unrelated_kept"]
    assert np.array_equal(first, r1["unrelated_kept"]) and np.array_equal(r["snps_kept"], r1["snps_kept"])
    assert final.dtype == np.bool_ and final.shape == (N,) and 0 < final.sum() < N
    assert r["vectors"].shape == (int(final.sum()), 5) and r["projection_all"].shape == (N, 5)
    # the second round is reproducible from its parts: PC-Relate on round 1's PCs, its pairs as the relatives
    t = fp.pcrelate_related(HM3, r1["projection_all"][:, :4], train=first, thr=T, snps=r["snps_kept"])
    assert t["i"].size > 0 and np.array_equal(fp.pcair_partition(HM3, snps=r["snps_kept"], kin_pairs=(t["i"], t["j"], t["kin"])), final)
    assert not (final[t["i"]] & final[t["j"]]).any()  # no PC-Relate pair above the threshold inside the final mask
    f = fp.flashpca(HM3, ndim=5, snps=r["snps_kept"], keep=final)
    for key in ("values", "vectors", "projection_all"):
        assert np.array_equal(f[key], r[key]), key
    print("hapmap3_data, second round: %d PC-Relate pairs above 2^-5.5; round 1 keeps %d, round 2 keeps %d of %d" % (t["i"].size, first.sum(), final.sum(), N))
