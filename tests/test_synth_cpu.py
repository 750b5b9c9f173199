"""The synthetic genotype model on the CPU: the library's host generator (fpca_debug_synth_host: the functions of csrc/synth.hpp, the
argument checks and fixed-point conversion of fpca_create_synthetic_model) against the replica of tests/synth_yardstick.py, bit for
bit; then what the header and include/fpca.h SAY about the model against what its per-SNP thresholds are.  No device is involved:
tests/test_gpu_synth.py holds the kernel to the same replica on the same grid.

The model properties run on the replica's thresholds over the first 20,000 SNPs of the default seed.  Their margins are four
sampling errors at 20,000 SNPs: sqrt(q (1 - q) / P) for a fraction q, 1.2533 sigma / sqrt(P) for the median of ln(rate), sigma /
sqrt(2 P) for the sd of ln(rate).  Seeds are fixed, so every outcome is a fixed one.

The realised mean of the log-normal thresholds is recorded in profiles/synth_model_figures.txt; `python tests/test_synth_cpu.py`
rewrites that file (figures()), and test_lognormal_mean_is_the_recorded_fraction_of_the_nominal_one holds the model to it.
"""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_yardstick as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "synth_model_figures.txt")
P = 20000
LOGNORMAL = [(0.02, 1.5), (0.01, 2.0), (0.001, 2.0), (0.02, 0.3), (0.001, 0.5)]  # (nominal mean, sigma): bench.py's and the route test's
EINVAL = -1


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


def split(case):
    kw = dict(case)
    return kw.pop("N"), kw.pop("P"), kw.pop("snp_begin"), kw.pop("seed"), kw


_thr_cache = {}


def thr(**model):
    """The replica's thresholds of the first 20,000 SNPs of the default seed, one population unless asked otherwise."""
    model.setdefault("n_pop", 1)
    key = tuple(sorted(model.items()))
    if key not in _thr_cache:
        _thr_cache[key] = Y.thresholds(P, **model)
    return _thr_cache[key]


# ---- bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for _, c in Y.GRID], ids=[t for t, _ in Y.GRID])
def test_host_generator_equals_the_replica_on_the_gpu_grid(case, fp):
    N, n, begin, seed, kw = split(case)
    got, fixed = fp.debug_synth_host(N, n, begin, seed, **kw)
    assert fixed == Y.Model(**kw).fixed()
    assert got.shape == (n, (N + 3) // 4) and np.array_equal(got, Y.generate(N, n, begin, seed, **kw))


def test_host_generator_equals_the_replica_on_a_wide_sweep(fp):
    """Wider than the GPU side repeats: 1500 random shapes and models -- every n_pop, N on both sides of n_pop, seeds and SNP
    indices over the whole 64-bit range, every model with random knobs -- and one long record per model."""
    rng = np.random.default_rng(20260928)
    for i in range(1500):
        n_pop = int(rng.integers(1, 65))
        N = int(rng.integers(1, 400)) if i % 3 else int(rng.integers(1, n_pop + 2))
        n = int(rng.integers(1, 4))
        seed = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        begin = int(rng.integers(0, (1 << 64) - 4, dtype=np.uint64)) if i % 2 else int(rng.integers(0, 1 << 20))
        kw = dict(n_pop=n_pop, fst=float(rng.choice([0.0, 0.05, 0.3, 0.99, rng.random() * 0.999])),
                  missing_rate=float(rng.choice([0.0, 0.001, 0.02, 0.5, 0.999, rng.random() * 0.999])),
                  maf_model=int(rng.integers(0, 2)), missing_model=int(rng.integers(0, 3)), conc_frac=float(rng.choice([0.0, 0.05, 1.0, rng.random()])),
                  lognormal_sigma=float(rng.choice([0.0, 0.3, 1.5, 4.0, rng.random() * 4])))
        got, fixed = fp.debug_synth_host(N, n, begin, seed, **kw)
        assert fixed == Y.Model(**kw).fixed(), (i, kw)
        assert np.array_equal(got, Y.generate(N, n, begin, seed, **kw)), (i, N, n, begin, seed, kw)
    for i, kw in enumerate(Y.MODELS):
        got, _ = fp.debug_synth_host(20001, 1, 7 * i, Y.DEFAULT_SEED, n_pop=64, **kw)
        assert np.array_equal(got, Y.generate(20001, 1, 7 * i, Y.DEFAULT_SEED, n_pop=64, **kw)), kw


def test_old_entry_is_the_model_with_zeroed_knobs(fp):
    """fpca_create_synthetic(n_pop, fst, missing_rate) hands fpca_create_synthetic_model a zeroed struct: on the host entry, the
    zeroed knobs give what the defaults of the Python wrapper give, whatever conc_frac and sigma say while their models are off."""
    a, fa = fp.debug_synth_host(513, 8, 300, 5, n_pop=12, fst=0.05, missing_rate=0.001, maf_model=0, missing_model=0, conc_frac=0.0, lognormal_sigma=0.0)
    b, fb = fp.debug_synth_host(513, 8, 300, 5, n_pop=12, fst=0.05, missing_rate=0.001, conc_frac=0.7, lognormal_sigma=3.0)
    assert np.array_equal(a, b) and np.array_equal(a, Y.generate(513, 8, 300, 5, n_pop=12))
    assert fa["sig2_fp"] == fb["sig2_fp"] == 0 and fa["med_q32"] == fb["med_q32"] == Y.llround(0.001 * 4294967296.0)


def test_rounding_of_the_five_integers_is_half_away_from_zero(fp):
    """llround on exact halves: 0.5 / 65536 -> 1, 1.5 / 65536 -> 2, 2.5 / 65536 -> 3 (half-to-even would give 0, 2, 2)."""
    for k in (0, 1, 2, 1000, 32767):
        x = (k + 0.5) / 65536.0
        _, f = fp.debug_synth_host(1, 0, 0, 0, n_pop=1, fst=x, missing_rate=x, conc_frac=x, missing_model=1)
        assert (f["fst_fp"], f["miss_thr"], f["conc_fp"]) == (k + 1, k + 1, k + 1) == tuple(Y.Model(fst=x, missing_rate=x, conc_frac=x).fixed()[n] for n in ("fst_fp", "miss_thr", "conc_fp"))
    _, f = fp.debug_synth_host(1, 0, 0, 0, n_pop=1, missing_rate=0.999, missing_model=2, lognormal_sigma=0.0)
    assert f["med_q32"] == Y.llround(0.9 * 4294967296.0)  # the median is capped at 0.9 before it is scaled


# ---- the branches of the log-normal rate ----------------------------------------------------------------------------------------
def test_lognormal_branches_are_reached_and_agree(fp):
    """At sigma = 4, the API's largest, an exponent e >= 20 (the rate saturates: the threshold is the 90 % cap whatever the median,
    a median of zero included) and an e < 0 (the rate is shifted down) both occur among the first 200,000 SNPs.  The third branch,
    e <= -40, cannot be reached through the API: |z| <= 6 sd and sigma / ln 2 <= 5.78, so |x| <= 34.7 and e >= -35.  (What it returns,
    0, is what the shift by 40 or more of a rate below 2^33 gives anyway.)  tests/test_gpu_synth.py generates the same two SNPs."""
    sat, neg = Y.lognormal_branch_snps()
    assert sat is not None and neg is not None and sat < Y.BRANCH_LIMIT and neg < Y.BRANCH_LIMIT
    sig2 = Y.Model(missing_model=2, lognormal_sigma=4.0).sig2_fp
    assert 6 * 65536 * sig2 < 35 << 32  # |x| = |sig2_fp z| >> 16 stays below 35 in 16.16
    for m in Y.BRANCH_MODELS:
        ts, tn = Y.thresholds(1, sat, **m), Y.thresholds(1, neg, **m)
        assert ts.e[0] >= 20 and ts.miss[0] == 58982 and -3 <= tn.e[0] < 0
        assert (tn.miss[0] > 0) == (m["missing_rate"] > 0)
        for j in (sat, neg):
            got, _ = fp.debug_synth_host(513, 1, j, Y.DEFAULT_SEED, **m)
            assert np.array_equal(got, Y.generate(513, 1, j, Y.DEFAULT_SEED, **m))
    # at a nominal mean of zero the saturating record still loses 90 % of its calls
    got, _ = fp.debug_synth_host(4000, 1, sat, Y.DEFAULT_SEED, **Y.BRANCH_MODELS[1])
    assert abs((Y.unpack(got, 4000) == 1).mean() - 0.9) < 6 * math.sqrt(0.09 / 4000)


# ---- what the header and fpca.h state ---------------------------------------------------------------------------------------------
def lognormal_figures(mean, sigma, fp=None):
    """The realised mean of the thresholds over the nominal one, its sampling error, and the rest of a line of the figures file.
    With fp, the two integers that set the distribution are the host entry's, checked against the replica's."""
    kw = dict(missing_model=2, missing_rate=mean, lognormal_sigma=sigma)
    t = thr(**kw)
    if fp is not None:
        _, f = fp.debug_synth_host(1, 0, 0, Y.DEFAULT_SEED, n_pop=1, **kw)
        assert (f["med_q32"], f["sig2_fp"]) == (t.model.med_q32, t.model.sig2_fp)
    rate = t.miss / 65536.0
    return dict(mean=mean, sigma=sigma, med_q32=t.model.med_q32, sig2_fp=t.model.sig2_fp, ratio=rate.mean() / mean,
                se=rate.std(ddof=1) / math.sqrt(P) / mean, median=float(np.median(rate)), zero=int((t.miss == 0).sum()),
                capped=int((t.miss == 58982).sum()), ratio4096=rate[:4096].mean() / mean)


def figures(fp):
    """The text of profiles/synth_model_figures.txt."""
    out = ["synthetic genotype model (csrc/synth.hpp): realised figures of the per-SNP thresholds over the first %d SNPs of the default seed %d"
           % (P, Y.DEFAULT_SEED),
           "from tests/synth_yardstick.py, which tests/test_synth_cpu.py holds fpca_debug_synth_host to bit for bit; written by `python tests/test_synth_cpu.py`",
           "missing_model 2 -- the nominal mean is missing_rate; the median is set to mean exp(-sigma^2 / 2), the Irwin-Hall normal ends at 6 sd, the rate"
           " is capped at 90 % and the 16-bit threshold floors small rates:"]
    for mean, sigma in LOGNORMAL + [(0.01, 1.5)]:
        g = lognormal_figures(mean, sigma, fp)
        out.append("lognormal mean %g sigma %g: med_q32 %d, sig2_fp %d; realised mean %.6f = %.4f of the nominal mean (sampling error %.4f); "
                   "median %.6f, nominal %.6f; thresholds floored to zero %d, capped %d; over the first 4096 SNPs %.4f of the nominal mean"
                   % (mean, sigma, g["med_q32"], g["sig2_fp"], g["ratio"] * mean, g["ratio"], g["se"], g["median"], mean * math.exp(-sigma * sigma / 2),
                      g["zero"], g["capped"], g["ratio4096"]))
    for conc in (0.0, 0.05, 0.25, 1.0):
        t = thr(missing_model=1, conc_frac=conc)
        hi = t.pick < t.model.conc_fp
        rng = "none" if not hi.any() else "%.2f .. %.2f %%" % (100 * t.miss[hi].min() / 65536.0, 100 * t.miss[hi].max() / 65536.0)
        rest = "none" if hi.all() else "<= %.4f %%" % (100 * t.miss[~hi].max() / 65536.0)
        out.append("concentrated conc_frac %g: %.2f %% of the SNPs affected, at %s; the rest %s; overall %.2f %%" % (conc, 100 * hi.mean(), rng, rest, 100 * t.miss.mean() / 65536.0))
    a, b = thr(maf_model=1).pj / 65536.0, thr().pj / 65536.0
    out.append("rare-variant spectrum: %.1f %% of the SNPs below 6 %%, %.1f %% below 0.2 %%, range [%.5f, %.5f]" % (100 * (a < 0.06).mean(), 100 * (a < 0.002).mean(), a.min(), a.max()))
    out.append("uniform spectrum: range [%.5f, %.5f]" % (b.min(), b.max()))
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("mean,sigma", LOGNORMAL)
def test_lognormal_median_and_spread_are_the_stated_ones(mean, sigma):
    """synth.hpp: rate_j = median 2^(sigma / ln 2 z_j), the median the one that gives the asked-for mean: mean exp(-sigma^2 / 2).
    The threshold is the rate floored to 1 / 65536, so the true median lies in [median, median + 1) thresholds."""
    t = thr(missing_model=2, missing_rate=mean, lognormal_sigma=sigma)
    want = math.log(mean) - sigma * sigma / 2
    med = float(np.median(t.miss))
    margin = 4 * 1.2533 * sigma / math.sqrt(P)
    print("mean %g sigma %g: ln median %.4f .. %.4f, stated %.4f, margin %.4f" % (mean, sigma, math.log(med / 65536), math.log((med + 1) / 65536), want, margin))
    assert math.log(med / 65536) <= want + margin and math.log((med + 1) / 65536) >= want - margin
    whole = bool((t.miss > 0).all() and (t.miss < 58982).all())  # nothing floored to zero, nothing capped
    assert whole == ((mean, sigma) in [(0.02, 0.3), (0.001, 0.5)])  # (the two narrow settings: this part of the test is not vacuous)
    if whole:
        sd = float(np.log((t.miss + 0.5) / 65536.0).std(ddof=1))  # (+ 0.5: the middle of the interval the floor leaves the rate in)
        print("sd of ln rate %.4f, stated %g, margin %.4f" % (sd, sigma, 4 * sigma / math.sqrt(2 * P)))
        assert abs(sd - sigma) <= 4 * sigma / math.sqrt(2 * P)


@pytest.mark.parametrize("mean,sigma", LOGNORMAL)
def test_lognormal_mean_is_the_recorded_fraction_of_the_nominal_one(mean, sigma, fp):
    """include/fpca.h: missing_rate is the NOMINAL mean of missing_model 2.  The tail that would carry the rest of the mean is cut
    three times (6 sd, the 90 % cap, small rates floored), so the realised mean is below it: by what, profiles/synth_model_figures.txt
    records, and the documents quote that file."""
    rec = {(float(m.group(1)), float(m.group(2))): (float(m.group(3)), float(m.group(4))) for m in re.finditer(
        r"^lognormal mean (\S+) sigma (\S+):.* = (\S+) of the nominal mean \(sampling error (\S+)\)", open(FIGURES).read(), flags=re.M)}
    g = lognormal_figures(mean, sigma, fp)
    ratio, se = rec[(mean, sigma)]
    print("mean %g sigma %g: realised / nominal %.4f, recorded %.4f, sampling error %.4f" % (mean, sigma, g["ratio"], ratio, g["se"]))
    assert g["ratio"] <= 1.0
    assert abs(g["ratio"] - ratio) <= g["se"] and abs(se - g["se"]) <= 0.1 * g["se"]
    assert 0.86 <= ratio <= 1.0  # "0.87-1.00 of it" (include/fpca.h, synth.hpp, Context.synthetic)


@pytest.mark.parametrize("conc_frac", [0.0, 0.05, 0.25, 1.0])
def test_concentrated_model_is_the_stated_one(conc_frac):
    """synth.hpp: a fraction conc_frac of the SNPs lose 10-30 % of their calls, every other SNP at most 0.1 %."""
    t = thr(missing_model=1, conc_frac=conc_frac)
    conc_fp, pick, miss_thr = t.model.conc_fp, t.pick, t.miss
    hi = pick < conc_fp
    assert np.all((miss_thr[hi] >= 6554) & (miss_thr[hi] <= 19660))
    assert np.all(miss_thr[~hi] <= 65)
    assert abs(hi.mean() - conc_frac) <= 4 * math.sqrt(conc_frac * (1 - conc_frac) / P)
    assert hi.any() == (conc_frac > 0) and hi.all() == (conc_frac == 1)


def test_allele_frequency_spectra_are_the_stated_ones():
    """synth.hpp: the rare-variant spectrum is 0.001 + 0.499 u^3 -- "half of the SNPs below 6 %, an eighth below 0.2 %" (exactly:
    49.1 % and 12.6 %), inside [0.001, 0.5); the uniform one is 0.05 + 0.90 u, inside [0.05, 0.95)."""
    a, b = thr(maf_model=1).pj, thr().pj
    for bound, stated in ((0.06, 0.5), (0.002, 0.125)):
        q = float((a / 65536.0 < bound).mean())
        print("rare spectrum: %.4f of the SNPs below %g, stated %g" % (q, bound, stated))
        assert abs(q - stated) <= 4 * math.sqrt(stated * (1 - stated) / P)
    assert a.min() >= 0.001 * 65536 and a.max() < 0.5 * 65536 and a.min() <= 70 and a.max() >= 32000  # (and the range is used)
    assert b.min() >= 0.05 * 65536 and b.max() < 0.95 * 65536 and b.min() <= 3290 and b.max() >= 62240


@pytest.mark.parametrize("fst,maf_model", [(0.0, 0), (0.05, 0), (0.99, 0), (0.05, 1), (0.99, 1)])
def test_population_frequencies_stay_inside_the_clamps(fst, maf_model):
    """synth.hpp: p_jc is clamped to [0.01, 0.99] -- from 0.0001 where the ancestral frequency is below 0.05; without drift it is p_j."""
    t = thr(n_pop=4, fst=fst, maf_model=maf_model)
    lo = np.where(t.pj < 3277, 7, 655)[:, None]
    assert np.all(t.pop >= lo) and np.all(t.pop <= 64880)
    if fst == 0.0:
        assert np.array_equal(t.pop, np.repeat(t.pj[:, None], 4, axis=1))
    if fst == 0.99:  # both clamps are reached
        assert (t.pop == lo).any() and (t.pop == 64880).any()
        assert maf_model == 0 or ((t.pop == 7).any() and (t.pop == 655).any())


def test_population_boundaries():
    """synth.hpp: contiguous populations of weight c + 1: boundaries monotone from 0 to N, sizes N (c + 1) / (n_pop (n_pop + 1) / 2)
    to within one sample; the replica's population of a sample is the one whose range holds it."""
    for n_pop in (1, 2, 3, 7, 12, 40, 63, 64):
        for N in (1, 2, 5, 63, 64, 100, 2079, 2080, 2081, 4097, 20000, (1 << 40) - 1):
            b = Y.boundaries(N, n_pop)
            assert len(b) == n_pop + 1 and b[0] == 0 and b[-1] == N and all(x <= y for x, y in zip(b, b[1:]))
            tot = n_pop * (n_pop + 1) // 2
            assert all(abs((b[c + 1] - b[c]) * tot - N * (c + 1)) < tot for c in range(n_pop))
            if N <= 20000:
                pop = Y.population_of(N, n_pop)
                assert np.array_equal(np.bincount(pop, minlength=n_pop), np.diff(b)) and np.all(np.diff(pop) >= 0)


@pytest.mark.parametrize("model", range(len(Y.MODELS)))
def test_cells_follow_their_thresholds(model, fp):
    """One 20,000-sample record of the host generator per model: the allele count of every population over its called samples is
    binomial(2 called, p_jc), the missing count binomial(N, missing threshold) -- each within 6 sd of its own threshold's expectation
    (and exactly there where the sd is zero)."""
    N, n_pop, snp = 20000, 6, 11
    kw = dict(Y.MODELS[model], n_pop=n_pop)
    got, _ = fp.debug_synth_host(N, 1, snp, Y.DEFAULT_SEED, **kw)
    codes = Y.unpack(got, N)[0]
    t = Y.thresholds(1, snp, **kw)
    q = t.miss[0] / 65536.0
    nmiss = int((codes == 1).sum())
    print("model %d: missing %d of %d, expected %.1f +- %.1f" % (model, nmiss, N, N * q, math.sqrt(N * q * (1 - q))))
    assert abs(nmiss - N * q) <= 6 * math.sqrt(N * q * (1 - q))
    dosage = np.array([2, 0, 1, 0])[codes]
    b = Y.boundaries(N, n_pop)
    for c in range(n_pop):
        called = codes[b[c]:b[c + 1]] != 1
        m, a, p = int(called.sum()), int(dosage[b[c]:b[c + 1]][called].sum()), t.pop[0, c] / 65536.0
        print("  population %d: %d alleles over %d called samples, expected %.1f +- %.1f" % (c, a, m, 2 * m * p, math.sqrt(2 * m * p * (1 - p))))
        assert abs(a - 2 * m * p) <= 6 * math.sqrt(2 * m * p * (1 - p))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
REFUSED = [dict(n_pop=0), dict(n_pop=65), dict(fst=1.0), dict(fst=-0.1), dict(missing_rate=1.0), dict(maf_model=2), dict(missing_model=3),
           dict(conc_frac=1.5), dict(missing_model=2, lognormal_sigma=4.5), dict(missing_model=2, lognormal_sigma=float("nan"))]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_both_entries_refuse_a_bad_model(kw, fp):
    """The checks are one function (cabi.cpp synth_reduce) that runs before the device entry allocates anything: FPCA_EINVAL with
    or without a device, from both entries."""
    with pytest.raises(fp.FpcaError) as e:
        fp.debug_synth_host(17, 2, **kw)
    assert e.value.code == EINVAL
    with pytest.raises(fp.FpcaError) as e:
        fp.Context.synthetic(17, 2, **kw)
    assert e.value.code == EINVAL


def test_both_entries_refuse_a_null_model_and_the_host_entry_a_bad_buffer(fp):
    L = fp.lib()
    h = C.c_void_p()
    assert L.fpca_create_synthetic_model(C.byref(h), 17, 0, 2, 1, None, 3, 0, 64) == EINVAL and not h.value
    out = np.zeros(10, dtype=np.uint8)
    assert L.fpca_debug_synth_host(17, 0, 2, 1, None, out.ctypes.data_as(C.c_void_p), None) == EINVAL
    from flashpca_amd._lib import SynthModel

    m = SynthModel(3, 0.05, 0.001, 0, 0, 0.0, 0.0)
    assert L.fpca_debug_synth_host(17, 0, 2, 1, C.byref(m), None, None) == EINVAL
    assert L.fpca_debug_synth_host(0, 0, 2, 1, C.byref(m), out.ctypes.data_as(C.c_void_p), None) == EINVAL
    assert L.fpca_debug_synth_host(17, 0, 2, 1, C.byref(m), out.ctypes.data_as(C.c_void_p), None) == 0  # (fixed may be NULL)
    assert np.array_equal(out.reshape(2, 5), Y.generate(17, 2, 0, 1, n_pop=3))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import flashpca_amd

    open(FIGURES, "w").write(figures(flashpca_amd))
    print(open(FIGURES).read(), end="")
