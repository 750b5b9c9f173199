"""fpca_ucca on the GPU against the reference's own arithmetic restated in numpy (RandomPCA::ucca, randompca.cpp:530-625: SVD of the
standardised Y, cov, var, wilks) on the CPU oracle's standardised matrices: every --standy, chunked phenotype blocks, the missing-call
routes and edge rules, the three arithmetics, SNP shards, the full-size problem, the CLI end to end, and the finishing kernels at their
edges: fewer SNPs than a row group, the ones column alone in and at column 1 of the third chunk, dense columns without variance."""
import os
import subprocess

import numpy as np
import pytest
from scipy import special

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
CHR1 = os.path.join(GOLD, "data_chr1")
CLI = os.path.join(ROOT, "flashpca_amd", "_build", "flashpca")
STANDS = ("sd", "binom2", "binom", "center", "none")


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def reference_r2(X, Ys):
    """The reference's loop, all SNPs at once: s = cov(x_j, Y) V sqrt(n - 1); r2_j = |sum (s / d)^2| / var(x_j)."""
    n = X.shape[0]
    _, d, Vt = np.linalg.svd(Ys, full_matrices=False)
    Xc = X - X.mean(axis=0)
    cov = Xc.T @ (Ys - Ys.mean(axis=0)) / (n - 1)
    s = cov @ Vt.T * np.sqrt(n - 1)
    varx = np.sum(Xc * Xc, axis=0) / (n - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(np.sum((s / d) ** 2, axis=1)) / varx


def wilks(r2, n, k):
    """wilks() (randompca.cpp:103-119) with the tail exact in r2."""
    with np.errstate(invalid="ignore", divide="ignore"):
        F = r2 / (1 - r2) * (n - k - 1) / k
    return np.sqrt(r2), F, special.betaincc(k / 2.0, (n - k - 1) / 2.0, r2)


def compare(res, X, Ys, k, rtol_r=1e-10, rtol_p=1e-8, label=""):
    n = X.shape[0]
    r2 = reference_r2(X, Ys)
    R, F, P = wilks(r2, n, k)
    zero_var = ~(np.sum((X - X.mean(axis=0)) ** 2, axis=0) > 0)
    assert np.all(np.isnan(res[zero_var])), label
    ok = ~zero_var
    assert not np.isnan(res[ok]).any(), label
    assert np.max(np.abs(res[ok, 0] - R[ok]) / R[ok]) < rtol_r, (label, np.max(np.abs(res[ok, 0] - R[ok]) / R[ok]))
    assert np.max(np.abs(res[ok, 1] - F[ok]) / F[ok]) < 4 * rtol_r, label
    good = ok & (P >= 1e-290)
    if good.any():
        assert np.max(np.abs(res[good, 2] - P[good]) / P[good]) < rtol_p, label
    assert np.all(res[ok & ~good, 2] < 1e-280), label  # (below the smallest normal numbers P may underflow to 0)
    return zero_var


def phenotypes(rng, n, k, stand, nan_frac=0.02):
    if stand in ("binom", "binom2"):
        Y = rng.integers(0, 3, size=(n, k)).astype(float)
    else:
        Y = rng.standard_normal((n, k)) * rng.uniform(0.5, 3, k) + (rng.uniform(-5, 5, k) if stand == "none" else 0)
    Y[rng.random((n, k)) < nan_frac] = np.nan
    return Y


@pytest.fixture(scope="module")
def hm3(fp, O):
    n = fp.count_fam_rows(HM3 + ".fam")
    X = O.OracleData(HM3 + ".bed", n, "binom2").dense()
    ctx = fp.Context.from_bed(HM3 + ".bed", n, accum="auto")
    yield ctx, X
    ctx.close()


@pytest.mark.parametrize("stand", STANDS)
def test_every_standy_against_the_reference_loop(fp, O, hm3, stand):
    """hapmap3_data (957 x 14,389): NaN phenotypes mean-imputed by the standardisation; "none" on uncentred phenotypes (the
    reference's formula there, not lm's R^2)."""
    ctx, X = hm3
    rng = np.random.default_rng(STANDS.index(stand) + 11)
    k = 6
    Y = phenotypes(rng, X.shape[0], k, stand)
    Ys, _ = O.standardise(Y, stand)
    res = ctx.ucca(Y, standy=stand)
    assert res.shape == (X.shape[1], 3)
    compare(res, X, Ys, k, label=stand)


@pytest.mark.parametrize("k", [1, 63, 64, 150])
def test_chunked_phenotype_blocks(fp, O, hm3, k):
    """k + 1 columns go through K2 in chunks of at most 64: one pass (k = 1, 63), the ones column alone in a second (k = 64),
    three (k = 150)."""
    ctx, X = hm3
    rng = np.random.default_rng(k)
    Y = rng.standard_normal((X.shape[0], k))
    Ys, _ = O.standardise(Y, "sd")
    compare(ctx.ucca(Y), X, Ys, k, label=str(k))


def test_missing_calls_and_edge_rules(fp, O):
    """The realistic profile (rare variants, concentrated missing calls) on the hybrid missing-call route; a monomorphic SNP gives a
    NaN row and leaves the others as they were; a phenotype equal to a SNP's dosage gives R = 1."""
    N, P, k = 3000, 2000, 8
    with fp.Context.synthetic(N, P, n_pop=3, realistic=True, accum="auto") as ctx:
        assert ctx.missing_mode(16) == 4
        packed = ctx.download_packed()
        X = O.OracleData(packed=packed, N=N, P=P, stand="binom2").dense()
        rng = np.random.default_rng(3)
        Y = rng.standard_normal((N, k))
        Ys, _ = O.standardise(Y, "sd")
        res = ctx.ucca(Y)
        zero_var = compare(res, X, Ys, k, label="realistic")
        ms, _ = ctx.stats()
        assert zero_var.sum() == np.sum(ms[:, 1] <= 1e-9)
        # a phenotype that IS a SNP's dosage (missing calls -> NaN, imputed like the SNP's own missing calls)
        sd = X.std(axis=0)
        j = int(np.argmax(sd))
        m, s = ms[j]
        Yd = Y.copy()
        Yd[:, 0] = np.where(X[:, j] == 0, np.nan, X[:, j] * s + m)
        rd = ctx.ucca(Yd)
        assert abs(rd[j, 0] - 1.0) < 1e-12 and (rd[j, 2] == 0 or rd[j, 2] < 1e-290)
        assert rd[j, 1] > 1e12
    # SNP `j0` made monomorphic: its row becomes NaN, every other row keeps its value
    np_ = (N + 3) // 4
    j0 = int(np.flatnonzero(~zero_var)[5])
    pk = packed.reshape(P, np_).copy()
    pk[j0, :] = 0  # every call homozygous A1
    with fp.Context.from_packed(pk, N, P, accum="auto") as ctx2:
        res2 = ctx2.ucca(Y)
    assert np.all(np.isnan(res2[j0]))
    keep = np.ones(P, bool)
    keep[j0] = False
    a, b = res[keep], res2[keep]
    fin = np.isfinite(a[:, 0])
    assert np.array_equal(fin, np.isfinite(b[:, 0]))
    assert np.max(np.abs(a[fin] - b[fin]) / np.abs(a[fin])) < 1e-13


def test_arithmetics_and_shards(fp, O):
    """Exact int8 (default), fp64 and fp32 K2 agree; two SNP shards reproduce the single context bit for bit."""
    N, P, k = 4000, 3000, 12
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((N, k))
    out = {}
    for accum in ("auto", "fp64", "fp32"):
        with fp.Context.synthetic(N, P, n_pop=5, accum=accum) as ctx:
            out[accum] = ctx.ucca(Y)
    ok = np.isfinite(out["fp64"][:, 0])
    rel = lambda a, b: np.max(np.abs(a[ok, 0] - b[ok, 0]) / b[ok, 0])  # noqa: E731
    assert rel(out["auto"], out["fp64"]) < 1e-12
    assert rel(out["fp32"], out["fp64"]) < 1e-6
    P1 = 1234
    with fp.Context.synthetic(N, P1, n_pop=5, accum="auto") as c1, fp.Context.synthetic(N, P - P1, snp_begin=P1, n_pop=5, accum="auto") as c2:
        sh = np.vstack([c1.ucca(Y), c2.ucca(Y)])
    # the default exact mode: a SNP's row depends on its own column and on [W | 1] only -- bit for bit
    assert np.array_equal(sh, out["auto"], equal_nan=True)


def test_full_size(fp, O):
    """500,000 x 100,000, realistic profile, k = 10 phenotypes from 20 causal SNPs plus noise: 2,000 SNPs (the causal ones and ten
    random runs) against the reference loop on their decoded columns; every other row finite and in range, except the zero-variance
    SNPs, whose rows are NaN."""
    N, P, k, seed = 500_000, 100_000, 10, 20261016
    rng = np.random.default_rng(1)
    causal = np.sort(rng.choice(P, 20, replace=False))
    runs = [(int(s), 198) for s in rng.choice(P - 198, 10, replace=False)]

    def decode(start, count):
        with fp.Context.synthetic(N, count, snp_begin=start, seed=seed, realistic=True, accum="fp64") as sub:
            return O.OracleData(packed=sub.download_packed(), N=N, P=count, stand="binom2").dense()

    Xc = np.column_stack([decode(int(j), 1) for j in causal])
    Y = Xc @ rng.standard_normal((20, k)) * 0.3 + rng.standard_normal((N, k))
    Ys, _ = O.standardise(Y, "sd")
    with fp.Context.synthetic(N, P, seed=seed, realistic=True, accum="auto") as ctx:
        res = ctx.ucca(Y)
        ms, _ = ctx.stats()
    compare(res[causal], Xc, Ys, k, label="causal")
    assert np.nanmin(res[causal, 2]) < 1e-100  # the causal SNPs are found
    for start, count in runs:
        compare(res[start:start + count], decode(start, count), Ys, k, label="run %d" % start)
    nan_rows = np.isnan(res).any(axis=1)
    assert np.array_equal(nan_rows, np.isnan(res).all(axis=1))
    assert nan_rows.sum() == np.sum(ms[:, 1] <= 1e-9)
    f = res[~nan_rows]
    assert np.all((f[:, 0] >= 0) & (f[:, 0] <= 1) & (f[:, 1] >= 0) & (f[:, 2] >= 0) & (f[:, 2] <= 1))


def test_cli_end_to_end(fp, O, tmp_path):
    """flashpca --ucca on data_chr1 with a generated phenotype file: header, SNP ids in .bim order, the Python API's values at the
    written precision, --suffix, --precision, --standy, --outmeansd, the milestones."""
    fam = [l.split() for l in open(CHR1 + ".fam").read().splitlines()]
    bim = [l.split() for l in open(CHR1 + ".bim").read().splitlines()]
    n, k = len(fam), 4
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((n, k)) + 1.5
    with open(tmp_path / "ph.txt", "w") as f:
        for r, y in zip(fam, Y):
            f.write("%s %s %s\n" % (r[0], r[1], " ".join(repr(float(v)) for v in y)))
    for extra, suffix, prec, standy in (([], ".txt", 7, "sd"), (["--suffix", ".u", "--precision", "12", "--standy", "center"], ".u", 12, "center")):
        r = subprocess.run([CLI, "--bfile", CHR1, "--ucca", "--pheno", "ph.txt", "--outmeansd", "ms" + suffix, "-v"] + extra, capture_output=True,
                           text=True, cwd=tmp_path, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "UCCA begin" in r.stdout and "UCCA done" in r.stdout and "UCCA online mode, N=%d p=%d" % (n, len(bim)) in r.stdout
        lines = open(tmp_path / ("ucca" + suffix)).read().splitlines()
        assert lines[0] == "SNP\tR\tFstat\tP"
        rows = [l.split("\t") for l in lines[1:]]
        assert [x[0] for x in rows] == [b[1] for b in bim]
        api = fp.ucca(CHR1, Y, standx="binom2", standy=standy)["result"]
        for row, ref in zip(rows, api):
            assert row[1:] == [O.format_number(v, prec) for v in ref], (row, ref)
        with fp.Context.from_bed(CHR1 + ".bed", n, accum="auto") as ctx:
            ms, _ = ctx.stats()
        ml = [l.split("\t") for l in open(tmp_path / ("ms" + suffix)).read().splitlines()]
        assert ml[0] == ["SNP", "RefAllele", "Mean", "SD"]
        assert [x[2:] for x in ml[1:]] == [[O.format_number(v, prec) for v in m] for m in ms]


def small_fileset(O, N, P, seed):
    """Binomial dosages (MAF in [0.1, 0.5], 1 % missing calls, no monomorphic SNP) as packed records, and the oracle's dense matrix."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.1, 0.5, P)
    u = rng.random((P, N))
    codes = np.where(u < (maf * maf)[:, None], 0, np.where(u < (maf * (2 - maf))[:, None], 2, 3)).astype(np.uint8)  # hom A1, het, hom A2
    codes[rng.random((P, N)) < 0.01] = 1  # missing
    c = np.zeros((P, (N + 3) // 4 * 4), dtype=np.uint8)
    c[:, :N] = codes
    packed = (c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)).astype(np.uint8)
    X = O.OracleData(packed=packed, N=N, P=P, stand="binom2").dense()
    assert np.all(X.std(axis=0) > 0)
    return packed, X, rng


@pytest.mark.parametrize("k", [1, 38])
@pytest.mark.parametrize("P", [1, 15, 17])
def test_fewer_snps_than_a_row_group(fp, O, P, k):
    """k_ucca_accum takes 16 SNPs per workgroup and k_ucca_finish 64: one SNP, one short of a workgroup of the first, one over it.
    N = 60 leaves n - k - 1 >= 21, so F stays well conditioned."""
    N = 60
    packed, X, rng = small_fileset(O, N, P, 100 * P + k)
    Y = rng.standard_normal((N, k))
    Ys, _ = O.standardise(Y, "sd")
    with fp.Context.from_packed(packed, N, P, accum="auto") as ctx:
        res = ctx.ucca(Y)
    assert res.shape == (P, 3)
    assert not compare(res, X, Ys, k, label="P=%d k=%d" % (P, k)).any()


@pytest.mark.parametrize("k", [128, 129])
def test_ones_column_in_the_third_chunk(fp, O, k):
    """k + 1 columns in chunks of 64: the ones column alone in the third chunk (k = 128: no W column there, ncw = 0), then at column 1
    of it behind the last W column (k = 129)."""
    N, P = 200, 33
    packed, X, rng = small_fileset(O, N, P, k)
    Y = rng.standard_normal((N, k))
    Ys, _ = O.standardise(Y, "sd")
    with fp.Context.from_packed(packed, N, P, accum="auto") as ctx:
        res = ctx.ucca(Y)
    assert not compare(res, X, Ys, k, label="k=%d" % k).any()


@pytest.mark.parametrize("stand", ["sd", "none"])
def test_dense_columns_without_variance(fp, O, stand):
    """The DEN_TOL rule of k_ucca_finish: a dense column whose sd is <= 1e-9 keeps its non-zero mean through the standardisation
    (util.cpp:104-107), so its den = sum x^2 - (sum x)^2 / N is rounding noise of either sign, not 0: the row is NaN, NaN, NaN.
    Two such columns: a constant one (3.7), and one that is NaN except for two equal values (0.1).  Under "none" the missing values
    take the mean and both columns are constant: both rows NaN.  Under "sd" the missing values become 0 (util.cpp:102-103) and the two
    observed ones do not: they keep the mean or, as here, the shifted-data variance of two equal values is rounding noise, sd = 3.9e-9
    passes the 1e-9 test and they become (x - mean) / sd = -4e-9.  Either way the standardised column HAS variance, the reference's
    loop on the standardised matrix gives it a finite row (R = 0.3104), and so must fpca_ucca: that row is held to the reference like
    every other (a NaN there would be a departure from the reference, not an edge rule).  Every row not NaN by the rule is within compare()'s
    bounds of the reference loop on the oracle's standardised matrix."""
    N, P, k = 50, 20, 3
    rng = np.random.default_rng(77)
    Xr = rng.standard_normal((N, P)) * rng.uniform(0.5, 2, P) + rng.uniform(-1, 1, P)
    Xr[rng.random((N, P)) < 0.02] = np.nan
    const, two = 4, 11
    Xr[:, const] = 3.7
    Xr[:, two] = np.nan
    Xr[[7, 31], two] = 0.1
    Y = rng.standard_normal((N, k))
    Ys, _ = O.standardise(Y, "sd")
    Xs, _ = O.standardise(Xr, stand)
    assert np.all(Xs[:, const] == Xs[0, const]) and Xs[0, const] != 0  # constant, non-zero mean kept
    flat = [const, two] if stand == "none" else [const]
    assert np.all(Xs[:, two] == 0.1) if stand == "none" else (len(set(Xs[:, two])) == 2 and np.sum(Xs[:, two] == 0) == N - 2)
    with fp.Context.from_dense(Xr, stand=stand) as ctx:
        res = ctx.ucca(Y)
    assert res.shape == (P, 3)
    assert np.all(np.isnan(res[flat])), res[flat]
    others = np.setdiff1d(np.arange(P), flat)
    assert not compare(res[others], Xs[:, others], Ys, k, label="dense " + stand).any()
