"""PC-Relate (fpca_pcrelate_beta / fpca_pcrelate_block / fpca_pcrelate_tri; Context.pcrelate_beta / pcrelate_block / pcrelate_tri,
pcrelate()) on the GPU against a numpy yardstick that never calls the feature.  The yardstick unpacks the raw 2-bit codes, takes mean / sd
from Context.stats() and restates include/fpca.h:
   x in {2, -, 1, 0} for the codes {0, 1, 2, 3}; a SNP is live when sd > 1e-9 and neither mean nor sd is NaN; V = [1 | pcs];
   beta_s = argmin over the training samples of (g_is - V_i beta)^2, g = x at a call and mean_s at a missing call, 0 for a SNP not live;
   mu = V beta / 2; usable: live, called, eps < mu < 1 - eps; r = x - 2 mu, w = sqrt(mu (1 - mu)) where usable, 0 elsewhere;
   S = r r', D = w w', kin = S / (4 D), NaN where D == 0.
1. Bit for bit (stage 2).  beta_s = [1, b_s, 0, 0] with b_s in {0, 2} and a first pc column in {0, 1} make mu 0.5 (usable, r in {-1, 0, 1},
   w = 0.5 exactly) or 1.5 (not usable) at every entry of any genotypes: S is an integer and D a quarter-integer under any order of the
   sums, so kin and den must be array_equal (NaN = NaN) to int64 numpy divided once -- kin = S / n, den = n / 4, n the SNPs usable in both.
2. beta (stage 1) against the longdouble normal equations: per SNP s and component k the residual |A beta_s - rhs_s|_k, A = V_t' V_t and
   rhs_s = V_t' g_s in longdouble, is held to
      (N_pad + 3 d + 8) 2^-53 (sum_{i in train} |V_ik| |g_is| + sum_l (|L| |L'|)_kl |beta_sl|),        L = chol(A).
   Derivation: rhs_sk reaches the device as mean_s c_k + sd_s T_sk, T_sk a sum of N_pad products in some order -- the forward bound of
   such a sum is N_pad 2^-53 sum |V_ik| |g_is| to first order (sd z = x - mean is one rounding of each term, the 8 pays for those, for the
   rounding of mean_s c_k and of A's entries, which are summed in long double and rounded once); the computed solution of L L' beta = rhs
   solves (A + dA) beta = rhs with |dA| <= (3 d + 1) 2^-53 |L| |L'| (Higham, Accuracy and Stability, theorem 10.4), which moves the
   residual by at most |dA| |beta|.  SNPs that are not live give exactly 0.
3. Kinship on ordinary genotypes against longdouble sums, the device's own beta fed back (stage 1's error is not counted twice).  Per
   entry, with M_is = sum_k |V_ik| |beta_sk|, d = npc + 1 and u = 2^-53: mu carries d roundings of a dot product of size M (the halving is
   exact), so r = x - 2 mu has e_r = u (|r| + (d + 1) M); w = sqrt(mu (1 - mu)) has three roundings of its own and the slope (1 - 2 mu) /
   (2 w) <= 1 / (2 w) on mu's error: e_w = u (3 w + (d + 1) M / (2 w)).  A sum of P_pad products in any order, each with one rounding:
      dS_ij <= sum_s (|r_i| e_r,j + |r_j| e_r,i) + (P_pad + 8) u sum_s |r_i| |r_j|,      dD likewise with w,
      |kin - kin_ld| <= 1.01 (dS / (4 D) + |kin| dD / D + u |kin|)
   (the quotient's first-order error and the divide's rounding; 1.01 covers the second order).  The condition under which the usable
   sets agree is asserted: no called entry of a live SNP has mu within 1e-9 of eps or of 1 - eps, in longdouble from the beta used.
4. Composite: beta=None equals the two calls bit for bit; pcrelate() on tests/golden/hapmap3_data with the PCs of flashpca(unrelated=0.0884)
   and maf=0.05 against the yardstick on the re-packed SNPs, float64 sums at twice the bound.
5. Refusals; every exit gives the scratch back.
Data: two populations (every third sample in the second; pa ~ U(0.02, 0.98), pb = clip(pa + N(0, 0.15), 0.005, 0.995)) with
tests/test_gpu_grm.py's trio and full sibs, duplicates (one across the whole range), missing rates 0 / 1 % / 20 % by 32-sample block, one
sample without any call, two monomorphic SNPs and one SNP without a call.  pcs: the centred population indicator, linspace(-1, 1, N), a
standard normal draw; train drops a random 30 % and the sample without calls.  Shapes (tests/test_gpu_king.py's): 70 x 300 one chunk, mostly
pad slots, a ragged second tile; 130 x 1000 two chunks; 257 x 2100 five chunks and five tiles.
Every test prints what it measured (pytest -s).
Measured on the MI355X (profiles/pcrelate_test_figures.txt): the hand-made model equals int64 numpy bit for bit -- the square, six
rectangles, the triangle and the denominators on each shape -- and slabs of 64 / 128 rows with panels of 512 SNPs change no bit; beta: the
largest residual is 0.002 - 0.008 of the bound under the int8 context, 0.006 - 0.051 under fp64; kinship: the largest error is 0.006 -
0.014 of the bound over 3 shapes x npc {0, 3, 31} x eps {0.01, 0}, the nearest mu to a threshold 2.4e-8; hapmap3_data within 0.006 of the
bound (2 allowed), 459 pairs above 0.0442 where half the relationship matrix puts 4,474; 2 / 9 / 9 / 8 scratch acquisitions per entry
point, all given back on every injected failure.  The 23 tests take 9 s together."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ENOMEM = -4
U = 2.0 ** -53
LD = np.longdouble


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


NOCALL = 44           # the sample without any call
SPECIAL = (3, 7, 11)  # SNPs: monomorphic (all dosage 0), monomorphic (all dosage 2), without any call
SHAPES = {"70x300": (70, 300, 1), "130x1000": (130, 1000, 2), "257x2100": (257, 2100, 3)}
DOSAGE = np.array([2.0, 0.0, 1.0, 0.0])  # by raw code (code 1, missing, is masked wherever this is used)


def missing_rate(N):
    """Sample s of an even 32-sample block has no missing call; in the odd blocks every fourth sample has 1 % and every eighth 20 %."""
    s = np.arange(N)
    odd = (s // 32) % 2 == 1
    rate = np.where(odd & (s % 4 == 0), 0.01, 0.0)
    return np.where(odd & (s % 8 == 4), 0.20, rate)


def structured_codes(N, P, seed):
    """((P, N) codes, pop): two populations, the relatives and the missing pattern of the module's header."""
    rng = np.random.default_rng(seed)
    pop = (np.arange(N) % 3 == 2)
    pa = rng.uniform(0.02, 0.98, P)
    pb = np.clip(pa + rng.normal(0.0, 0.15, P), 0.005, 0.995)
    d = rng.binomial(2, np.where(pop[:, None], pb[None, :], pa[None, :]), (N, P))

    def child(a, b):
        return rng.binomial(1, d[a] / 2.0) + rng.binomial(1, d[b] / 2.0)

    d[2], d[3] = child(0, 1), child(0, 1)
    d[40], d[41] = child(33, 36), child(33, 36)
    d[5] = d[4]
    d[N - 1] = d[6]
    d[48] = d[7]
    codes = np.array([3, 2, 0], dtype=np.uint8)[d]  # (N, P)
    codes[rng.random((N, P)) < missing_rate(N)[:, None]] = 1
    codes[NOCALL] = 1
    codes[:, SPECIAL[0]] = np.where(codes[:, SPECIAL[0]] == 1, 1, 3)
    codes[:, SPECIAL[1]] = np.where(codes[:, SPECIAL[1]] == 1, 1, 0)
    codes[:, SPECIAL[2]] = 1
    return np.ascontiguousarray(codes.T), pop


def make_pcs(N, pop, seed, npc):
    """The three columns of the header, then standard normal columns up to npc."""
    rng = np.random.default_rng(seed + 100)
    base = np.stack([pop - pop.mean(), np.linspace(-1.0, 1.0, N), rng.standard_normal(N)], axis=1)
    extra = rng.standard_normal((N, max(npc - 3, 0)))
    return np.ascontiguousarray(np.concatenate([base, extra], axis=1)[:, :npc])


def make_train(N, seed):
    train = np.random.default_rng(seed + 200).random(N) >= 0.3
    train[NOCALL] = False
    return train


def n_pad(N):
    return ((N + 3) // 4 + 127) // 128 * 128 * 4


def p_pad(P):
    return (P + 255) // 256 * 256


_CASE = {}


def case(fp, name):
    """One generated shape: codes, the context's own mean / sd -- computed once and left unchanged."""
    if name not in _CASE:
        N, P, seed = SHAPES[name]
        codes, pop = structured_codes(N, P, seed)
        packed = pack_codes(codes)
        with fp.Context.from_packed(packed, N, P) as ctx:
            ms = ctx.stats()[0].copy()
        live = live_snps(ms)
        assert not live[list(SPECIAL)].any() and live.sum() == P - 3
        _CASE[name] = dict(N=N, P=P, seed=seed, codes=codes, pop=pop, packed=packed, ms=ms, live=live, train=make_train(N, seed))
    return _CASE[name]


# ---- the yardstick -------------------------------------------------------------------------------------------------
def live_snps(ms):
    with np.errstate(invalid="ignore"):
        return (ms[:, 1] > 1e-9) & ~np.isnan(ms[:, 0])


def design(pcs):
    return np.concatenate([np.ones((pcs.shape[0], 1)), pcs], axis=1)


def operands(codes, live, V, beta, eps, dtype):
    """(r, w, usable, mu, margin) as (N, P) arrays of `dtype`; margin: the smallest distance of mu from a threshold over the called entries
    of the live SNPs."""
    x = DOSAGE[codes].T.astype(dtype)
    called = (codes != 1).T & live[None, :]
    mu = (V.astype(dtype) @ beta.T.astype(dtype)) / dtype(2)
    lo, hi = dtype(eps), dtype(1) - dtype(eps)
    usable = called & (mu > lo) & (mu < hi)
    margin = float(np.minimum(np.abs(mu - lo), np.abs(mu - hi))[called].min()) if called.any() else np.inf
    with np.errstate(invalid="ignore"):
        r = np.where(usable, x - 2 * mu, dtype(0))
        w = np.where(usable, np.sqrt(np.where(usable, mu * (1 - mu), dtype(0))), dtype(0))
    return r, w, usable, mu, margin


def kin_reference(codes, live, V, beta, eps, dtype, P):
    """kin, D in `dtype` and the per-pair bound of the header (float64)."""
    r, w, usable, mu, margin = operands(codes, live, V, beta, eps, dtype)
    d = V.shape[1]
    S, D = r @ r.T, w @ w.T
    r64, w64 = np.abs(r).astype(np.float64), w.astype(np.float64)
    M = np.abs(V) @ np.abs(beta).T
    e_r = np.where(usable, U * (r64 + (d + 1) * M), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_w = np.where(usable, U * (3 * w64 + (d + 1) * M / (2 * w64)), 0.0)
    cross = r64 @ e_r.T
    dS = cross + cross.T + (p_pad(P) + 8) * U * (r64 @ r64.T)
    cross = w64 @ e_w.T
    dD = cross + cross.T + (p_pad(P) + 8) * U * (w64 @ w64.T)
    D64 = D.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        kin = np.where(D == 0, np.nan, S / (4 * D))
        band = 1.01 * (dS / (4 * D64) + np.abs(kin).astype(np.float64) * dD / D64 + U * np.abs(kin).astype(np.float64)) * (1.0 + 1e-9)
    band = np.where(D64 == 0, 0.0, band)
    return dict(kin=kin, D=D, band=band, margin=margin, usable=usable, mu=mu)


def within(got, G, band, factor=1.0):
    """Every entry of got within factor x band of G, NaN exactly where G is; returns (ok, the largest error / band)."""
    nan_ok = np.array_equal(np.isnan(got), np.isnan(G.astype(np.float64)))
    err = np.abs(got.astype(G.dtype) - G).astype(np.float64)
    f = np.isfinite(err)
    ok = nan_ok and bool(np.all(err[f] <= factor * band[f]))
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(band > 0, err / band, 0.0))) if f.any() else 0.0
    return ok, worst


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def rectangles(N):
    """Six rectangles off the 64-sample tiles and the 32-sample blocks; three reach below the diagonal, one is a single pair."""
    return [(5, 40, 3, N - 10), (33, N - 33, 0, 31), (N - 7, 7, N - 10, 10), (0, 1, N - 1, 1), (N - 1, 1, 0, N), (31, 34, 31, 34)]


def pack_tri(M):
    return np.ascontiguousarray(M[np.tril_indices(M.shape[0])])


# ---- 1. bit for bit (stage 2) ----------------------------------------------------------------------------------------
def exact_model(c):
    """(pcs, beta, kin, den) of the hand-made model on the case's genotypes: int64 numpy divided once."""
    N, P = c["N"], c["P"]
    pcs = make_pcs(N, c["pop"], c["seed"], 3)
    pcs[:, 0] = (np.arange(N) % 5 < 2)
    beta = np.zeros((P, 4))
    beta[:, 0] = 1.0
    beta[:, 1] = np.where(np.arange(P) % 3 == 1, 2.0, 0.0)
    mu2 = 1 + np.outer(pcs[:, 0], beta[:, 1]).astype(np.int64)  # 2 mu: 1 or 3
    usable = (c["codes"] != 1).T & c["live"][None, :] & (mu2 == 1)
    R = np.where(usable, DOSAGE[c["codes"]].T.astype(np.int64) - 1, 0)
    Uu = usable.astype(np.int64)
    S, n = R @ R.T, Uu @ Uu.T
    assert usable.any() and not usable.all() and (mu2 == 3).any() and n[NOCALL].max() == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        kin = S.astype(np.float64) / n.astype(np.float64)
    kin[n == 0] = np.nan
    return pcs, beta, kin, n.astype(np.float64) / 4.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_model_bit_for_bit(fp, name):
    c = case(fp, name)
    N, P = c["N"], c["P"]
    pcs, beta, kin, den = exact_model(c)
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        got, gden = ctx.pcrelate_block(pcs, 0, N, 0, N, beta=beta, den=True)
        eq, eqd, sym = same(got, kin), same(gden, den), np.array_equal(got, got.T, equal_nan=True)
        print("%s exact model pcrelate_block(0, %d, 0, %d): %d finite, %d NaN; kin equal to int64 numpy bit for bit: %s, den equal: %s, equal "
              "to its transpose: %s" % (name, N, N, np.isfinite(got).sum(), np.isnan(got).sum(), eq, eqd, sym))
        assert eq and eqd and sym, (name, np.argwhere(~((got == kin) | (np.isnan(got) & np.isnan(kin))))[:5])
        assert same(ctx.pcrelate_block(pcs, 0, N, 0, N, beta=beta), got), "two calls differ"
        tri, tden = ctx.pcrelate_tri(pcs, beta=beta, den=True)
        assert same(tri, pack_tri(kin)) and same(tden, pack_tri(den)), (name, "pcrelate_tri")
        assert same(ctx.pcrelate_tri(pcs, beta=beta), tri)
        for i0, ni, j0, nj in rectangles(N):
            got, gden = ctx.pcrelate_block(pcs, i0, ni, j0, nj, beta=beta, den=True)
            eq = same(got, np.ascontiguousarray(kin[i0:i0 + ni, j0:j0 + nj])) and same(gden, np.ascontiguousarray(den[i0:i0 + ni, j0:j0 + nj]))
            print("%s exact model pcrelate_block(%d, %d, %d, %d): equal to numpy bit for bit: %s" % (name, i0, ni, j0, nj, eq))
            assert eq, (name, i0, ni, j0, nj)
        assert np.isnan(ctx.pcrelate_block(pcs, NOCALL, 1, 0, N, beta=beta)).all()


_SLAB_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import flashpca_amd as fp
d = np.load(sys.argv[2])
N, P = int(d["N"]), int(d["P"])
out = {}
with fp.test_hooks():
    with fp.Context.from_packed(d["packed"], N, P) as ctx:
        for rows in json.loads(sys.argv[3]):
            os.environ["FPCA_PCR_SLAB_ROWS"] = str(rows)
            os.environ["FPCA_PCR_PANEL_SNPS"] = "512"
            for key in ("exact", "ord"):
                tri, den = ctx.pcrelate_tri(d[key + "_pcs"], beta=d[key + "_beta"], den=True)
                blk, bden = ctx.pcrelate_block(d[key + "_pcs"], 0, N, 0, N, beta=d[key + "_beta"], den=True)
                rect = ctx.pcrelate_block(d[key + "_pcs"], 5, 200, 130, 100, beta=d[key + "_beta"])
                for k, v in (("tri", tri), ("den", den), ("blk", blk), ("bden", bden), ("rect", rect)):
                    out["%d.%s.%s" % (rows, key, k)] = v
np.savez(sys.argv[4], **out)
print("CHILD ok")
"""


def test_slabs_and_panels_change_no_bit(fp):
    """FPCA_PCR_SLAB_ROWS (test build) = 64 and 128 with FPCA_PCR_PANEL_SNPS = 512 in a child process: slabs of one and two row tiles and
    five panels where the default is one slab and one panel give the triangle, the square and a rectangle of the default bit for bit, on
    the exact model and on ordinary coefficients (panel edges are multiples of the matrix instruction's K = 4)."""
    c = case(fp, "257x2100")
    N, P = c["N"], c["P"]
    pcs_e, beta_e, kin_e, den_e = exact_model(c)
    pcs_o = make_pcs(N, c["pop"], c["seed"], 3)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        beta_o = ctx.pcrelate_beta(pcs_o, train=c["train"])
        ref = {}
        for key, pcs, beta in (("exact", pcs_e, beta_e), ("ord", pcs_o, beta_o)):
            tri, den = ctx.pcrelate_tri(pcs, beta=beta, den=True)
            blk, bden = ctx.pcrelate_block(pcs, 0, N, 0, N, beta=beta, den=True)
            ref[key] = dict(tri=tri, den=den, blk=blk, bden=bden, rect=ctx.pcrelate_block(pcs, 5, 200, 130, 100, beta=beta))
    assert same(ref["exact"]["blk"], kin_e) and same(ref["ord"]["tri"], pack_tri(ref["ord"]["blk"]))
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(src, packed=c["packed"], N=N, P=P, exact_pcs=pcs_e, exact_beta=beta_e, ord_pcs=pcs_o, ord_beta=beta_o)
        r = subprocess.run([sys.executable, "-c", _SLAB_CHILD, ROOT, src, json.dumps([64, 128]), out], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0 and "CHILD ok" in r.stdout, r.stderr[-2000:]
        res = dict(np.load(out))
    for rows in (64, 128):
        for key in ("exact", "ord"):
            eq = all(same(res["%d.%s.%s" % (rows, key, k)], v) for k, v in ref[key].items())
            print("slabs of %d rows, panels of 512 SNPs, %s coefficients: triangle, square, rectangle and denominators equal to the default's bit "
                  "for bit: %s" % (rows, "hand-made" if key == "exact" else "ordinary", eq))
            assert eq, (rows, key)


# ---- 2. beta (stage 1) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accum", ["auto", "fp64"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_beta_against_the_normal_equations(fp, name, accum):
    c = case(fp, name)
    N, P, train, live = c["N"], c["P"], c["train"], c["live"]
    for npc in (0, 3, 31):
        pcs = make_pcs(N, c["pop"], c["seed"], npc)
        d = npc + 1
        with fp.Context.from_packed(c["packed"], N, P, accum=accum) as ctx:
            assert np.array_equal(ctx.stats()[0], c["ms"], equal_nan=True)
            beta = ctx.pcrelate_beta(pcs, train=train)
            if npc == 3:
                full = ctx.pcrelate_beta(pcs)
                assert same(full, ctx.pcrelate_beta(pcs, train=np.ones(N, dtype=bool))), "train=None differs from an all-ones mask"
        assert beta.shape == (P, d) and np.all(beta[~live] == 0.0) and np.isfinite(beta).all()
        Vt = design(pcs)[train].astype(LD)
        g = np.where(c["codes"] != 1, DOSAGE[c["codes"]], np.nan_to_num(c["ms"][:, 0])[:, None]).T[train].astype(LD)  # (n_train, P)
        A = Vt.T @ Vt
        rhs = Vt.T @ g  # (d, P)
        L = np.linalg.cholesky(A.astype(np.float64))
        res = np.abs(A @ beta.T.astype(LD) - rhs).astype(np.float64)
        bound = (n_pad(N) + 3 * d + 8) * U * ((np.abs(Vt).T @ np.abs(g)).astype(np.float64) + (np.abs(L) @ np.abs(L).T) @ np.abs(beta).T)
        worst = float((res[:, live] / bound[:, live]).max())
        print("%s accum=%s npc=%d: %d training samples, cond(A) %.3g; largest residual |A beta - rhs| / bound %.4f over %d live SNPs x %d "
              "components" % (name, accum, npc, train.sum(), np.linalg.cond(A.astype(np.float64)), worst, live.sum(), d))
        assert np.all(res[:, live] <= bound[:, live]), (name, accum, npc, worst)


# ---- 3. kinship on ordinary genotypes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("npc", [0, 3, 31])
@pytest.mark.parametrize("name", list(SHAPES))
def test_kinship_within_the_bound(fp, name, npc):
    c = case(fp, name)
    N, P, live = c["N"], c["P"], c["live"]
    pcs = make_pcs(N, c["pop"], c["seed"], npc)
    V = design(pcs)
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        beta = ctx.pcrelate_beta(pcs, train=c["train"])
        for eps in (0.01, 0.0):
            ref = kin_reference(c["codes"], live, V, beta, eps, LD, P)
            called = ((c["codes"] != 1).T & live[None, :])
            masked = called & ~ref["usable"]
            assert ref["margin"] > 1e-9, (name, npc, eps, ref["margin"])  # the premise: both sides agree on the usable entries
            got, den = ctx.pcrelate_block(pcs, 0, N, 0, N, eps=eps, beta=beta, den=True)
            ok, worst = within(got, ref["kin"], ref["band"])
            D64 = ref["D"].astype(np.float64)
            derr = float(np.max(np.abs(den - D64) / np.maximum(D64, 1e-300) * (D64 > 0)))
            fin = np.isfinite(got)
            off = got[np.tril(fin, -1)]
            print("%s npc=%d eps=%g: %.2f %% of the called entries outside (eps, 1 - eps), nearest mu to a threshold %.2e, min D %.1f; largest "
                  "|kin - kin_longdouble| / bound %.4f; den relative error %.1e; diagonal mean %.4f, off-diagonal mean %.4f; symmetric bit for "
                  "bit: %s" % (name, npc, eps, 100.0 * masked.sum() / called.sum(), ref["margin"], D64[D64 > 0].min(), worst, derr,
                               np.nanmean(np.diag(got)), off.mean(), np.array_equal(got, got.T, equal_nan=True)))
            print("%s npc=%d eps=%g: duplicates kin[4][5] %.4f kin[6][N-1] %.4f kin[7][48] %.4f, parent-offspring kin[0][2] %.4f kin[1][3] %.4f, "
                  "full sibs kin[2][3] %.4f, founders kin[0][1] %.4f" % (name, npc, eps, got[4, 5], got[6, N - 1], got[7, 48], got[0, 2], got[1, 3],
                                                                     got[2, 3], got[0, 1]))
            assert ok, (name, npc, eps, worst)
            assert np.array_equal(got, got.T, equal_nan=True)
            assert np.isnan(got[NOCALL]).all() and np.isnan(got[:, NOCALL]).all() and np.all(den[NOCALL] == 0.0)
            assert same(ctx.pcrelate_tri(pcs, eps=eps, beta=beta), pack_tri(got))  # the triangle is the square, bit for bit
            if npc == 3:
                for i0, ni, j0, nj in rectangles(N):
                    assert same(ctx.pcrelate_block(pcs, i0, ni, j0, nj, eps=eps, beta=beta), np.ascontiguousarray(got[i0:i0 + ni, j0:j0 + nj])), (name, eps, i0, ni, j0, nj)


# ---- 4. composite ----------------------------------------------------------------------------------------------------
def test_estimating_beta_inside_the_call_changes_no_bit(fp):
    for name in SHAPES:
        c = case(fp, name)
        N, P, train = c["N"], c["P"], c["train"]
        pcs = make_pcs(N, c["pop"], c["seed"], 3)
        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            beta = ctx.pcrelate_beta(pcs, train=train)
            tri2, den2 = ctx.pcrelate_tri(pcs, beta=beta, den=True)
            tri1, den1 = ctx.pcrelate_tri(pcs, train=train, den=True)
            blk2 = ctx.pcrelate_block(pcs, 5, 40, 3, N - 10, beta=beta)
            blk1 = ctx.pcrelate_block(pcs, 5, 40, 3, N - 10, train=train)
            other = ctx.pcrelate_tri(pcs)  # (all samples train: another beta, another matrix)
        eq = same(tri1, tri2) and same(den1, den2) and same(blk1, blk2)
        print("%s: beta=None against pcrelate_beta followed by beta=: triangle, denominators and a rectangle equal bit for bit: %s" % (name, eq))
        assert eq and not same(other, tri1), name


def test_golden_hapmap3(fp):
    name = "hapmap3_data"
    prefix = os.path.join(GOLD, name)
    codes, N, P = read_bed_codes(prefix)
    with fp.Context.from_bed(prefix + ".bed", N) as ctx:
        ms = ctx.stats()[0].copy()
    r = fp.flashpca(prefix, ndim=3, unrelated=0.0884)
    pcs, train = np.ascontiguousarray(r["projection_all"][:, :3]), r["unrelated_kept"]
    res = fp.pcrelate(prefix, pcs, train=train, maf=0.05)
    maf = np.minimum(ms[:, 0] / 2.0, 1.0 - ms[:, 0] / 2.0)
    snps = ~(np.nan_to_num(maf, nan=0.0) < 0.05)
    sub, subms = codes[snps], ms[snps]
    assert res["beta"].shape == (snps.sum(), 4) and len(res["ids"]) == N and 0 < snps.sum() < P
    ref = kin_reference(sub, live_snps(subms), design(pcs), res["beta"], 0.01, np.float64, int(snps.sum()))
    assert ref["margin"] > 1e-9, ref["margin"]
    ok, worst = within(res["tri"], pack_tri(ref["kin"]), pack_tri(ref["band"]), factor=2.0)
    dg = res["tri"][np.arange(N) * (np.arange(N) + 3) // 2]
    offd = np.ones(res["tri"].size, dtype=bool)
    offd[np.arange(N) * (np.arange(N) + 3) // 2] = False
    g = fp.grm(prefix, maf=0.05)["tri"]
    print("%s: %d x %d of %d SNPs (maf 0.05), %d training samples; triangle against float64 BLAS sums: largest error / bound %.4f (allowed 2); "
          "nearest mu to a threshold %.2e; diagonal mean %.4f, off-diagonal mean %.2e; pairs with kinship above 0.0442: PC-Relate %d, the "
          "relationship matrix on the same SNPs (G / 2) %d" % (name, N, snps.sum(), P, train.sum(), worst, ref["margin"], dg.mean(), res["tri"][offd].mean(),
                                                                (res["tri"][offd] > 0.0442).sum(), (g[offd] / 2.0 > 0.0442).sum()))
    assert ok, worst
    assert np.allclose(res["den"], pack_tri(ref["D"]), rtol=1e-12, atol=0.0) and same(res["inbreeding"], 2.0 * dg - 1.0)
    assert 0.4 < dg.mean() < 0.6


# ---- 5. refusals and scratch -------------------------------------------------------------------------------------------
def test_refusals(fp):
    c = case(fp, "70x300")
    N, P, train = c["N"], c["P"], c["train"]
    pcs = make_pcs(N, c["pop"], c["seed"], 3)

    def refused(call, msg, code=-1):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == code
        print("refused: %s" % str(e.value)[:140])

    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        beta = ctx.pcrelate_beta(pcs, train=train)
        ref = ctx.pcrelate_block(pcs, 0, N, 0, N, beta=beta)
        calls = ((lambda p=pcs, **kw: ctx.pcrelate_beta(p, **kw), "fpca_pcrelate_beta"),
                 (lambda p=pcs, **kw: ctx.pcrelate_block(p, 0, N, 0, N, **kw), "fpca_pcrelate_block"),
                 (lambda p=pcs, **kw: ctx.pcrelate_tri(p, **kw), "fpca_pcrelate_tri"))
        bad = pcs.copy()
        bad[9, 1] = np.nan
        dep = pcs.copy()
        dep[:, 2] = 2.0 * dep[:, 1] - 0.5
        few = np.zeros(N, dtype=bool)
        few[:4] = True
        for call, fn in calls:
            refused(lambda: call(np.zeros((N, 32))), fn + ": npc = 32 is outside 0 .. 31")
            refused(lambda: call(bad), fn + r": pcs\[9\]\[1\] is not finite")
            refused(lambda: call(dep), fn + r": \[1 \| pcs\] is rank deficient over the training samples")
            refused(lambda: call(train=few), fn + ": 4 training samples; a regression on 4 columns needs at least 5")
        for eps in (0.5, -0.01, float("nan")):
            refused(lambda: ctx.pcrelate_block(pcs, 0, N, 0, N, eps=eps), "fpca_pcrelate_block: eps = .* is outside 0 <= eps < 0.5")
            refused(lambda: ctx.pcrelate_tri(pcs, eps=eps, beta=beta), "fpca_pcrelate_tri: eps = .* is outside 0 <= eps < 0.5")
        binf = beta.copy()
        binf[17, 2] = np.inf
        refused(lambda: ctx.pcrelate_tri(pcs, beta=binf), r"fpca_pcrelate_tri: beta\[17\]\[2\] is not finite")
        refused(lambda: ctx.pcrelate_block(pcs, 0, N, 0, N, beta=binf), r"fpca_pcrelate_block: beta\[17\]\[2\] is not finite")
        refused(lambda: ctx.pcrelate_block(pcs, 0, N + 1, 0, N, beta=beta), "are not a non-empty rectangle")
        refused(lambda: ctx.pcrelate_block(pcs, 0, N, N, 1, beta=beta), "are not a non-empty rectangle")
        refused(lambda: ctx.pcrelate_block(pcs, 3, 0, 0, N, beta=beta), "are not a non-empty rectangle")
        with pytest.raises(ValueError):
            ctx.pcrelate_tri(pcs[:-1])
        with pytest.raises(ValueError):
            ctx.pcrelate_tri(pcs, beta=beta[:, :3])
        with pytest.raises(ValueError):
            ctx.pcrelate_beta(pcs, train=np.ones(N + 1, dtype=bool))
        L = fp.lib()
        assert L.fpca_pcrelate_beta(ctx.h, pcs.ctypes.data, 3, None, None) == -1 and L.fpca_pcrelate_tri(ctx.h, pcs.ctypes.data, 3, None, None, 0.01, None, None) == -1
        assert L.fpca_pcrelate_block(ctx.h, None, 3, None, None, 0.01, 0, N, 0, N, ref.ctypes.data, None) == -1
        ctx.set_sample_mask(np.arange(N) % 3 != 0)
        for call, fn in calls:
            refused(call, fn + ": a sample mask is set")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        for call, fn in calls:
            refused(call, fn + ": this context is one shard of several")
        refused(lambda: ctx.bench_pcrelate(3, 1), "fpca_bench_pcrelate: this context is one shard of several")
        ctx.set_rank(1, 0)
        assert same(ctx.pcrelate_block(pcs, 0, N, 0, N, beta=beta), ref) and same(ctx.pcrelate_beta(pcs, train=train), beta)  # the context is intact
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        p50 = np.zeros((50, 1))
        refused(lambda: dense.pcrelate_beta(p50), "fpca_pcrelate_beta: this context holds a dense matrix")
        refused(lambda: dense.pcrelate_block(p50, 0, 50, 0, 50), "fpca_pcrelate_block: this context holds a dense matrix")
        refused(lambda: dense.pcrelate_tri(p50), "fpca_pcrelate_tri: this context holds a dense matrix")
    # a block over 1 GiB, met through a wide context of few SNPs
    big_n = 2 ** 14 + 1
    with fp.Context.from_packed(np.full(((big_n + 3) // 4) * 2, 0xFF, dtype=np.uint8), big_n, 2) as wide:
        buf = np.zeros(1)
        assert fp.lib().fpca_pcrelate_block(wide.h, None, 0, None, None, 0.01, 0, big_n, 0, big_n, buf.ctypes.data, None) == -1
        msg = fp.lib().fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "16385 x 16385 doubles is over the limit of 1073741824 bytes" in msg


def test_scratch_is_freed_on_every_exit(fp):
    """The pattern of tests/test_gpu_grm.py on the test build: the n-th acquisition of a call is made to fail (FPCA_ENOMEM before the runtime
    is asked for anything) for every n until the call succeeds; after each failure the counts of live device allocations and events are
    what they were, the message names the entry point, and the result after the failures is the result before them."""
    c = case(fp, "257x2100")
    N, P, train = c["N"], c["P"], c["train"]
    pcs = make_pcs(N, c["pop"], c["seed"], 3)
    with fp.test_hooks() as L:
        def live():
            out = (C.c_uint64 * 3)()
            assert L.fpca_debug_scratch_live(out) == 0
            return tuple(int(v) for v in out)

        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            ctx.stats()
            ctx.pcrelate_beta(pcs, train=train)  # (the context's own workspaces of the K2 pass are grown once, outside the counts)

            def bench():
                ms, flops = ctx.bench_pcrelate(3, 2)
                return np.all(ms > 0), flops

            for entry, call, least in (("fpca_pcrelate_beta", lambda: (ctx.pcrelate_beta(pcs, train=train),), 2),
                                       ("fpca_pcrelate_block", lambda: ctx.pcrelate_block(pcs, 3, 130, 60, 190, train=train, den=True), 5),
                                       ("fpca_pcrelate_tri", lambda: ctx.pcrelate_tri(pcs, train=train, den=True), 5),
                                       ("fpca_bench_pcrelate", bench, 5)):
                L.fpca_debug_scratch_fail_at(0)
                base = live()
                ref = call()
                assert live() == base, "%s leaks on the success path" % entry
                first_ok, out = None, None
                for n in range(1, 40):
                    assert L.fpca_debug_scratch_fail_at(n) == 0
                    try:
                        out = call()
                    except fp.FpcaError as e:
                        assert e.code == ENOMEM and entry in str(e), (entry, n, str(e))
                        assert live() == base, "%s leaks when acquisition %d fails" % (entry, n)
                        continue
                    finally:
                        L.fpca_debug_scratch_fail_at(0)
                    first_ok = n
                    break
                print("%s: %d acquisitions, all given back on every injected failure" % (entry, (first_ok or 0) - 1))
                assert first_ok is not None and first_ok - 1 >= least and live() == base
                assert all(np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True) for a, b in zip(out, ref)), entry
