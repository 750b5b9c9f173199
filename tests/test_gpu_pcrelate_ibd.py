"""PC-Relate IBD sharing (fpca_pcrelate_ibd_block / fpca_pcrelate_ibd_tri / fpca_pcrelate_classify; Context.pcrelate_ibd_block /
pcrelate_ibd_tri, pcrelate_ibd(), pcrelate_related()) on the GPU against a numpy yardstick that never calls the feature.  The yardstick
unpacks the raw 2-bit codes, takes mean / sd from Context.stats() and restates include/fpca.h:
   x in {2, -, 1, 0} for the codes {0, 1, 2, 3}; a SNP is live when sd > 1e-9 and neither mean nor sd is NaN; V = [1 | pcs]; mu = V beta / 2;
   usable (m = 1): live, called, eps < mu < 1 - eps; where usable v = mu (1 - mu), gD = mu / 0 / 1 - mu for x = 0 / 1 / 2, q = gD - v,
   u = mu^2, t = (1 - mu)^2, a = [x = 0], c = [x = 2]; 0 elsewhere;
   Q = q q', E = v v', H = u t' + t u', I0 = a c' + c a', n = m m';  k2 = Q / E - f_i f_j (NaN where E == 0), k0 = I0 / H (NaN where H == 0).
1. Bit for bit.  npc = 1 with a pc column in {0, 1} and beta_s from {(1, 0), (0.5, 1), (1.5, -1), (1, 2)} make mu 0.25, 0.5, 0.75 (usable) or
   1.5 (not usable) at every entry of any genotypes: every q, v, u, t is a multiple of 2^-4 below 1, every product a multiple of 2^-8 and
   every sum exact in fp64 under any order, so k2 (with a dyadic f, and with f=None), k0 and nsnp must be array_equal (NaN = NaN) to
   float64 numpy -- one divide, one rounded product, one subtract -- on the square, six rectangles off the tiles and the triangle; the
   square equals its transpose; slabs of 64 / 128 rows with 512-SNP panels change no bit, on these and on ordinary coefficients; the
   sample without calls has NaN / 0 rows.
2. Exact structure on the relatives, same model: a child never holds the opposite homozygote of its parent and a duplicate never that
   of its copy, so I0 = 0 and k0 == 0.0 exactly wherever H > 0; the full sibs have the yardstick's I0 > 0 (asserted first).
3. Ordinary genotypes against longdouble sums, the device's own beta fed back, f from the device's own kinship diagonal.  Per entry, with
   M_is = sum_k |V_ik| |beta_sk|, d = npc + 1 and u = 2^-53 (first order; o = 1 - mu; 0 < mu, o < 1 at a usable entry):
      e_mu = (d + 1) u M / 2          d roundings of a dot product of size M, the halving exact (item 3 of test_gpu_pcrelate.py)
      e_o  = e_mu + u o                one subtract
      e_v  = o e_mu + mu e_o + u v = e_mu + 2 u v                         (mu + o = 1)
      e_u  = 2 mu e_mu + u mu^2        e_t = 2 o e_o + u o^2 = 2 o e_mu + 3 u o^2
      e_q  = e_gD + e_v + u |q|,       e_gD = e_mu (x = 0), e_o (x = 2), 0 (x = 1)
   A sum of P_pad products in any order, each with one rounding:
      dQ  <= sum_s (|q_i| e_q,j + |q_j| e_q,i) + (P_pad + 8) u sum_s |q_i| |q_j|,          dE likewise with v
      dH  <= sum_s (u_i e_t,j + t_j e_u,i + t_i e_u,j + u_j e_t,i) + (P_pad + 8) u H + u H   (the two halves, then their one add)
      |k2 - k2_ld| <= 1.01 (dQ / E + |Q / E| dE / E + u |Q / E| + u |f_i f_j| + u |k2|)       (the divide, the product, the subtract)
      |k0 - k0_ld| <= 1.01 (k0 dH / H + u k0)                                               (I0 is an exact integer)
   (1.01 covers the second order.)  nsnp is exact.  The condition under which the usable sets agree is asserted: no called entry of a live
   SNP has mu within 1e-9 of eps or of 1 - eps, in longdouble from the beta used.  The bound is not tuned to what was observed.
4. Composite: beta=None equals the two calls bit for bit; pcrelate_ibd() and pcrelate_related() on tests/golden/hapmap3_data with the PCs of
   flashpca(unrelated=0.0884) and maf=0.05 against the yardstick on the re-packed SNPs (float64 sums, twice the bound) on every listed pair
   and a fixed random sample of 500 other pairs; k0 + k1 + k2 == 1 within 4 ulp; the kinship triangle is pcrelate()'s bit for bit; the
   cross-table of the type against king_related()'s for KING's first-degree pairs is printed, not asserted.
5. Refusals; every exit gives the scratch back.
Data: tests/test_gpu_pcrelate.py's recipe, copied -- two populations, a trio with two children (0, 1 -> 2, 3) and a second one (33, 36 ->
40, 41), duplicates (4, 5), (6, N - 1), (7, 48), missing rates 0 / 1 % / 20 % by 32-sample block, one sample without any call, two
monomorphic SNPs and one SNP without a call.  Shapes: 70 x 300, 130 x 1000, 257 x 2100.
Every test prints what it measured (pytest -s); the figures of the MI355X run are in profiles/pcrelate_ibd_test_figures.txt."""
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


# ---- data (the recipe of tests/test_gpu_pcrelate.py) -------------------------------------------------------------------
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
PARENT_CHILD = ((0, 2), (1, 2), (0, 3), (1, 3), (33, 40), (36, 40), (33, 41), (36, 41))
FULL_SIBS = (2, 3)


def duplicates(N):
    return ((4, 5), (6, N - 1), (7, 48))


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
    """The centred population indicator, linspace(-1, 1, N), a standard normal draw, then standard normal columns up to npc."""
    rng = np.random.default_rng(seed + 100)
    base = np.stack([pop - pop.mean(), np.linspace(-1.0, 1.0, N), rng.standard_normal(N)], axis=1)
    extra = rng.standard_normal((N, max(npc - 3, 0)))
    return np.ascontiguousarray(np.concatenate([base, extra], axis=1)[:, :npc])


def make_train(N, seed):
    train = np.random.default_rng(seed + 200).random(N) >= 0.3
    train[NOCALL] = False
    return train


def p_pad(P):
    return (P + 255) // 256 * 256


def live_snps(ms):
    with np.errstate(invalid="ignore"):
        return (ms[:, 1] > 1e-9) & ~np.isnan(ms[:, 0])


def design(pcs):
    return np.concatenate([np.ones((pcs.shape[0], 1)), pcs], axis=1)


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
def operands(codes, live, V, beta, eps, dtype):
    """The operands of the header as (N, P) arrays of `dtype`, the usable mask, and margin: the smallest distance of mu from a threshold
    over the called entries of the live SNPs."""
    x = DOSAGE[codes].T
    called = (codes != 1).T & live[None, :]
    mu = (V.astype(dtype) @ beta.T.astype(dtype)) / dtype(2)
    lo, hi = dtype(eps), dtype(1) - dtype(eps)
    usable = called & (mu > lo) & (mu < hi)
    margin = float(np.minimum(np.abs(mu - lo), np.abs(mu - hi))[called].min()) if called.any() else np.inf
    zero = dtype(0)
    mu = np.where(usable, mu, zero)
    om = np.where(usable, dtype(1) - mu, zero)
    v = mu * om
    gd = np.where(x == 0, mu, np.where(x == 2, om, zero))
    q = np.where(usable, gd - v, zero)
    return dict(x=x, usable=usable, mu=mu, om=om, v=v, q=q, u=mu * mu, t=om * om, a=(usable & (x == 0)).astype(np.float64),
                c=(usable & (x == 2)).astype(np.float64), m=usable.astype(np.float64), margin=margin)


def sums(o):
    H1 = o["u"] @ o["t"].T
    I0 = o["a"] @ o["c"].T
    return dict(Q=o["q"] @ o["q"].T, E=o["v"] @ o["v"].T, H=H1 + H1.T, I0=I0 + I0.T, n=o["m"] @ o["m"].T)


def outputs(s, f):
    """k2, k0, nsnp from the sums in their own dtype: one divide, one rounded product, one subtract."""
    ff = np.multiply.outer(f, f).astype(s["Q"].dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        k2 = np.where(s["E"] == 0, np.nan, s["Q"] / s["E"] - ff)
        k0 = np.where(s["H"] == 0, np.nan, s["I0"].astype(s["H"].dtype) / s["H"])
    return k2, k0, s["n"].astype(np.uint32)


def reference(codes, live, V, beta, eps, f, dtype, P):
    """k2, k0 in `dtype`, nsnp, and the per-pair bounds of the header (float64)."""
    o = operands(codes, live, V, beta, eps, dtype)
    s = sums(o)
    k2, k0, n = outputs(s, f.astype(dtype))
    d = V.shape[1]
    us = o["usable"]
    g = {k: np.abs(o[k]).astype(np.float64) for k in ("mu", "om", "v", "q", "u", "t")}
    M = np.abs(V) @ np.abs(beta).T
    e_mu = np.where(us, (d + 1) * U * M / 2.0, 0.0)
    e_o = np.where(us, e_mu + U * g["om"], 0.0)
    e_v = np.where(us, e_mu + 2.0 * U * g["v"], 0.0)
    e_u = np.where(us, 2.0 * g["mu"] * e_mu + U * g["u"], 0.0)
    e_t = np.where(us, 2.0 * g["om"] * e_mu + 3.0 * U * g["t"], 0.0)
    e_gd = np.where(o["x"] == 0, e_mu, np.where(o["x"] == 2, e_o, 0.0))
    e_q = np.where(us, e_gd + e_v + U * g["q"], 0.0)
    n_u = (p_pad(P) + 8) * U
    cross = g["q"] @ e_q.T
    dQ = cross + cross.T + n_u * (g["q"] @ g["q"].T)
    cross = g["v"] @ e_v.T
    dE = cross + cross.T + n_u * (g["v"] @ g["v"].T)
    cross = g["u"] @ e_t.T + e_u @ g["t"].T
    H64 = s["H"].astype(np.float64)
    dH = cross + cross.T + n_u * H64 + U * H64
    E64, QE = s["E"].astype(np.float64), np.abs(s["Q"] / np.where(s["E"] == 0, 1, s["E"])).astype(np.float64)
    ff = np.abs(np.multiply.outer(f, f))
    with np.errstate(invalid="ignore", divide="ignore"):
        b2 = 1.01 * (dQ / E64 + QE * dE / E64 + U * QE + U * ff + U * np.abs(k2).astype(np.float64)) * (1.0 + 1e-9)
        a0 = np.abs(k0).astype(np.float64)
        b0 = 1.01 * (a0 * dH / H64 + U * a0) * (1.0 + 1e-9)
    return dict(k2=k2, k0=k0, nsnp=n, band2=np.where(E64 == 0, 0.0, b2), band0=np.where(H64 == 0, 0.0, b0), margin=o["margin"], usable=us,
                E=s["E"], H=s["H"], I0=s["I0"])


def within(got, G, band, factor=1.0):
    """Every entry of got within factor x band of G, NaN exactly where G is; returns (ok, the largest error / band)."""
    nan_ok = np.array_equal(np.isnan(got), np.isnan(G.astype(np.float64)))
    err = np.abs(got.astype(G.dtype) - G).astype(np.float64)
    f = np.isfinite(err)
    ok = nan_ok and bool(np.all(err[f] <= factor * band[f]))
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0)))) if f.any() else 0.0
    return ok, worst


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same3(got, k2, k0, n):
    return same(got["k2"], k2) and same(got["k0"], k0) and same(got["nsnp"], n)


def rectangles(N):
    """Six rectangles off the 64-sample tiles and the 32-sample blocks; three reach below the diagonal, one is a single pair."""
    return [(5, 40, 3, N - 10), (33, N - 33, 0, 31), (N - 7, 7, N - 10, 10), (0, 1, N - 1, 1), (N - 1, 1, 0, N), (31, 34, 31, 34)]


def pack_tri(M):
    return np.ascontiguousarray(M[np.tril_indices(M.shape[0])])


def sub(M, r):
    i0, ni, j0, nj = r
    return np.ascontiguousarray(M[i0:i0 + ni, j0:j0 + nj])


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------
BETAS = np.array([[1.0, 0.0], [0.5, 1.0], [1.5, -1.0], [1.0, 2.0]])

_EXACT = {}


def exact_model(c):
    """(pcs, beta, f, the float64 yardstick with f, the float64 yardstick without) of the hand-made model on the case's genotypes."""
    key = (c["N"], c["P"])
    if key not in _EXACT:
        N, P = c["N"], c["P"]
        pcs = (np.arange(N) % 5 < 2).astype(np.float64).reshape(N, 1)
        beta = BETAS[np.random.default_rng(c["seed"] + 300).integers(0, 4, P)]
        f = ((np.arange(N) % 9) - 4) / 16.0
        o = operands(c["codes"], c["live"], design(pcs), beta, 0.01, np.float64)
        called = (c["codes"] != 1).T & c["live"][None, :]
        mus = set(np.unique((design(pcs) @ beta.T / 2.0)[called]))
        assert mus == {0.25, 0.5, 0.75, 1.5} and o["usable"].any() and not o["usable"][called].all()
        for k in ("q", "v", "u", "t"):  # multiples of 2^-4 below 1: every sum is exact in any order
            assert np.all(o[k] * 16 == np.round(o[k] * 16)) and np.abs(o[k]).max() < 1
        s = sums(o)
        assert s["n"][NOCALL].max() == 0
        _EXACT[key] = (pcs, beta, f, outputs(s, f), outputs(s, np.zeros(N)), s)
    return _EXACT[key]


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_model_bit_for_bit(fp, name):
    c = case(fp, name)
    N, P = c["N"], c["P"]
    pcs, beta, f, (k2, k0, n), (k2z, _, _), _ = exact_model(c)
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        got = ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta)
        eq = [same(got["k2"], k2), same(got["k0"], k0), same(got["nsnp"], n)]
        sym = all(np.array_equal(got[k], got[k].T, equal_nan=True) for k in got)
        print("%s exact model pcrelate_ibd_block(0, %d, 0, %d): k2 %d finite, %d NaN, k0 %d finite, %d NaN, nsnp up to %d; k2 / k0 / nsnp equal "
              "to float64 numpy bit for bit: %s; equal to their transposes: %s" % (name, N, N, np.isfinite(got["k2"]).sum(), np.isnan(got["k2"]).sum(),
                                                                                 np.isfinite(got["k0"]).sum(), np.isnan(got["k0"]).sum(),
                                                                                 got["nsnp"].max(), eq, sym))
        assert all(eq) and sym, (name, eq, sym)
        assert same3(ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta), got["k2"], got["k0"], got["nsnp"]), "two calls differ"
        nof = ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, beta=beta)
        assert same3(nof, k2z, k0, n) and not same(k2z, k2), (name, "f=None")
        tri = ctx.pcrelate_ibd_tri(pcs, f=f, beta=beta)
        assert same3(tri, pack_tri(k2), pack_tri(k0), pack_tri(n)), (name, "pcrelate_ibd_tri")
        assert same3(ctx.pcrelate_ibd_tri(pcs, beta=beta), pack_tri(k2z), pack_tri(k0), pack_tri(n)), (name, "pcrelate_ibd_tri, f=None")
        for r in rectangles(N):
            g = ctx.pcrelate_ibd_block(pcs, *r, f=f, beta=beta)
            eq = same3(g, sub(k2, r), sub(k0, r), sub(n, r))
            print("%s exact model pcrelate_ibd_block(%d, %d, %d, %d): equal to numpy bit for bit: %s" % ((name,) + r + (eq,)))
            assert eq, (name, r)
        row = ctx.pcrelate_ibd_block(pcs, NOCALL, 1, 0, N, f=f, beta=beta)
        assert np.isnan(row["k2"]).all() and np.isnan(row["k0"]).all() and np.all(row["nsnp"] == 0)


def test_relatives_have_the_exact_structure(fp):
    for name in SHAPES:
        c = case(fp, name)
        N, P = c["N"], c["P"]
        pcs, beta, f, (k2, k0, n), _, s = exact_model(c)
        assert s["I0"][FULL_SIBS] > 0 and s["H"][FULL_SIBS] > 0, name  # first: the yardstick's own full sibs hold opposite homozygotes
        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            got = ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta)["k0"]
        for i, j in PARENT_CHILD + duplicates(N):
            assert s["H"][i, j] > 0 and s["I0"][i, j] == 0, (name, i, j)
            assert got[i, j] == 0.0 and got[j, i] == 0.0 and not np.signbit(got[i, j]), (name, i, j, got[i, j])
        i, j = FULL_SIBS
        assert got[i, j] == s["I0"][i, j] / s["H"][i, j] and got[i, j] > 0, (name, got[i, j])
        print("%s: k0 == 0.0 exactly on %d parent-offspring pairs and %d duplicates; full sibs I0 %d, H %.4f, k0 %.6f (the yardstick's, bit for "
              "bit)" % (name, len(PARENT_CHILD), len(duplicates(N)), s["I0"][i, j], s["H"][i, j], got[i, j]))


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
                pcs, beta, f = d[key + "_pcs"], d[key + "_beta"], d[key + "_f"]
                for tag, r in (("tri", ctx.pcrelate_ibd_tri(pcs, f=f, beta=beta)), ("blk", ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta)),
                               ("rect", ctx.pcrelate_ibd_block(pcs, 5, 200, 130, 100, f=f, beta=beta))):
                    for k, v in r.items():
                        out["%d.%s.%s.%s" % (rows, key, tag, k)] = v
np.savez(sys.argv[4], **out)
print("CHILD ok")
"""


def test_slabs_and_panels_change_no_bit(fp):
    """FPCA_PCR_SLAB_ROWS (test build) = 64 and 128 with FPCA_PCR_PANEL_SNPS = 512 in a child process: slabs of one and two row tiles and
    five panels where the default is one slab and one panel give the triangle, the square and a rectangle of the default bit for bit, on
    the exact model and on ordinary coefficients."""
    c = case(fp, "257x2100")
    N, P = c["N"], c["P"]
    pcs_e, beta_e, f_e, (k2, k0, n), _, _ = exact_model(c)
    pcs_o = make_pcs(N, c["pop"], c["seed"], 3)
    f_o = np.random.default_rng(5).uniform(-0.1, 0.1, N)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FPCA_")}
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        beta_o = ctx.pcrelate_beta(pcs_o, train=c["train"])
        ref = {}
        for key, pcs, beta, f in (("exact", pcs_e, beta_e, f_e), ("ord", pcs_o, beta_o, f_o)):
            ref[key] = dict(tri=ctx.pcrelate_ibd_tri(pcs, f=f, beta=beta), blk=ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta),
                            rect=ctx.pcrelate_ibd_block(pcs, 5, 200, 130, 100, f=f, beta=beta))
    assert same3(ref["exact"]["blk"], k2, k0, n)
    o = ref["ord"]
    assert same3(o["tri"], pack_tri(o["blk"]["k2"]), pack_tri(o["blk"]["k0"]), pack_tri(o["blk"]["nsnp"]))
    assert all(np.array_equal(o["blk"][k], o["blk"][k].T, equal_nan=True) for k in o["blk"])  # (ordinary sums: (i, j) and (j, i) the same bits)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "in.npz"), os.path.join(tmp, "out.npz")
        np.savez(src, packed=c["packed"], N=N, P=P, exact_pcs=pcs_e, exact_beta=beta_e, exact_f=f_e, ord_pcs=pcs_o, ord_beta=beta_o, ord_f=f_o)
        r = subprocess.run([sys.executable, "-c", _SLAB_CHILD, ROOT, src, json.dumps([64, 128]), out], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0 and "CHILD ok" in r.stdout, r.stderr[-2000:]
        res = dict(np.load(out))
    for rows in (64, 128):
        for key in ("exact", "ord"):
            eq = all(same(res["%d.%s.%s.%s" % (rows, key, tag, k)], v) for tag, d in ref[key].items() for k, v in d.items())
            print("slabs of %d rows, panels of 512 SNPs, %s coefficients: triangle, square and rectangle of k2, k0 and nsnp equal to the default's "
                  "bit for bit: %s" % (rows, "hand-made" if key == "exact" else "ordinary", eq))
            assert eq, (rows, key)


# ---- 3. ordinary genotypes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npc", [0, 3, 31])
@pytest.mark.parametrize("name", list(SHAPES))
def test_ibd_within_the_bound(fp, name, npc):
    c = case(fp, name)
    N, P, live = c["N"], c["P"], c["live"]
    pcs = make_pcs(N, c["pop"], c["seed"], npc)
    V = design(pcs)
    with fp.Context.from_packed(c["packed"], N, P) as ctx:
        beta = ctx.pcrelate_beta(pcs, train=c["train"])
        for eps in (0.01, 0.0):
            kin = ctx.pcrelate_tri(pcs, eps=eps, beta=beta)
            f = np.nan_to_num(2.0 * kin[np.arange(N) * (np.arange(N) + 3) // 2] - 1.0)
            ref = reference(c["codes"], live, V, beta, eps, f, LD, P)
            assert ref["margin"] > 1e-9, (name, npc, eps, ref["margin"])  # the premise: both sides agree on the usable entries
            got = ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, eps=eps, beta=beta)
            ok2, worst2 = within(got["k2"], ref["k2"], ref["band2"])
            ok0, worst0 = within(got["k0"], ref["k0"], ref["band0"])
            sym = all(np.array_equal(got[k], got[k].T, equal_nan=True) for k in got)
            print("%s npc=%d eps=%g: nearest mu to a threshold %.2e, min E %.2f, min H %.2f; largest |k2 - k2_longdouble| / bound %.4f, largest "
                  "|k0 - k0_longdouble| / bound %.4f; nsnp equal: %s; symmetric bit for bit: %s" % (
                      name, npc, eps, ref["margin"], float(ref["E"][ref["E"] > 0].min()), float(ref["H"][ref["H"] > 0].min()), worst2, worst0,
                      same(got["nsnp"], ref["nsnp"]), sym))
            print("%s npc=%d eps=%g: (k0, k2) of duplicates [4][5] (%.4f, %.4f), parent-offspring [0][2] (%.4f, %.4f) [1][3] (%.4f, %.4f), full "
                  "sibs [2][3] (%.4f, %.4f), founders [0][1] (%.4f, %.4f)" % (name, npc, eps, got["k0"][4, 5], got["k2"][4, 5], got["k0"][0, 2],
                                                                             got["k2"][0, 2], got["k0"][1, 3], got["k2"][1, 3], got["k0"][2, 3],
                                                                             got["k2"][2, 3], got["k0"][0, 1], got["k2"][0, 1]))
            assert ok2 and ok0, (name, npc, eps, worst2, worst0)
            assert same(got["nsnp"], ref["nsnp"]) and sym
            assert np.isnan(got["k2"][NOCALL]).all() and np.isnan(got["k0"][:, NOCALL]).all() and np.all(got["nsnp"][NOCALL] == 0)
            tri = ctx.pcrelate_ibd_tri(pcs, f=f, eps=eps, beta=beta)  # the triangle is the square, bit for bit
            assert same3(tri, pack_tri(got["k2"]), pack_tri(got["k0"]), pack_tri(got["nsnp"]))
            if npc == 3:
                for r in rectangles(N):
                    g = ctx.pcrelate_ibd_block(pcs, *r, f=f, eps=eps, beta=beta)
                    assert same3(g, sub(got["k2"], r), sub(got["k0"], r), sub(got["nsnp"], r)), (name, eps, r)


# ---- 4. composite ----------------------------------------------------------------------------------------------------
def test_estimating_beta_inside_the_call_changes_no_bit(fp):
    for name in SHAPES:
        c = case(fp, name)
        N, P, train = c["N"], c["P"], c["train"]
        pcs = make_pcs(N, c["pop"], c["seed"], 3)
        f = np.random.default_rng(6).uniform(-0.1, 0.1, N)
        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            beta = ctx.pcrelate_beta(pcs, train=train)
            t2 = ctx.pcrelate_ibd_tri(pcs, f=f, beta=beta)
            t1 = ctx.pcrelate_ibd_tri(pcs, f=f, train=train)
            b2 = ctx.pcrelate_ibd_block(pcs, 5, 40, 3, N - 10, f=f, beta=beta)
            b1 = ctx.pcrelate_ibd_block(pcs, 5, 40, 3, N - 10, f=f, train=train)
            other = ctx.pcrelate_ibd_tri(pcs, f=f)  # (all samples train: another beta, other sums)
        eq = same3(t1, t2["k2"], t2["k0"], t2["nsnp"]) and same3(b1, b2["k2"], b2["k0"], b2["nsnp"])
        print("%s: beta=None against pcrelate_beta followed by beta=: triangle and a rectangle of k2, k0, nsnp equal bit for bit: %s" % (name, eq))
        assert eq and not same(other["k2"], t1["k2"]), name


def test_golden_hapmap3(fp):
    name = "hapmap3_data"
    prefix = os.path.join(GOLD, name)
    codes, N, P = read_bed_codes(prefix)
    with fp.Context.from_bed(prefix + ".bed", N) as ctx:
        ms = ctx.stats()[0].copy()
    r = fp.flashpca(prefix, ndim=3, unrelated=0.0884)
    pcs, train = np.ascontiguousarray(r["projection_all"][:, :3]), r["unrelated_kept"]
    res = fp.pcrelate_ibd(prefix, pcs, train=train, maf=0.05)
    tab = fp.pcrelate_related(prefix, pcs, train=train, maf=0.05)
    base = fp.pcrelate(prefix, pcs, train=train, maf=0.05)
    assert all(same(res[k], base[k]) for k in ("tri", "den", "inbreeding", "beta")) and res["ids"] == base["ids"]  # the kinship triangle, bit for bit
    maf = np.minimum(ms[:, 0] / 2.0, 1.0 - ms[:, 0] / 2.0)
    snps = ~(np.nan_to_num(maf, nan=0.0) < 0.05)
    subc, subms = codes[snps], ms[snps]
    f = np.nan_to_num(res["inbreeding"])
    ref = reference(subc, live_snps(subms), design(pcs), res["beta"], 0.01, f, np.float64, int(snps.sum()))
    assert ref["margin"] > 1e-9, ref["margin"]
    size = N * (N + 1) // 2
    assert all(res[k].shape == (size,) for k in ("k0", "k1", "k2", "nsnp")) and res["nsnp"].dtype == np.uint32
    assert same(res["nsnp"], pack_tri(ref["nsnp"]))
    # the table: the pairs i < j above 2^-5.5, sorted by (i, j), rows of the triangles
    ii, jj = np.tril_indices(N, -1)
    at = ii * (ii + 1) // 2 + jj
    sel = res["tri"][at] > 2 ** -5.5
    order = np.lexsort((ii[sel], jj[sel]))
    li, lj, lat = jj[sel][order], ii[sel][order], at[sel][order]
    assert list(tab) == ["i", "j", "kin", "k0", "k1", "k2", "nsnp", "type"] and tab["type"].dtype == np.uint8
    assert np.array_equal(tab["i"], li) and np.array_equal(tab["j"], lj) and np.all(tab["i"] < tab["j"]) and len(li) > 0
    for k, src in (("kin", "tri"), ("k0", "k0"), ("k1", "k1"), ("k2", "k2"), ("nsnp", "nsnp")):
        assert same(tab[k], res[src][lat]), k
    assert same(tab["type"], fp.pcrelate_classify(tab["kin"], tab["k0"], tab["k2"], tab["nsnp"], k0_switch=-1.0)[2])
    few = fp.pcrelate_related(prefix, pcs, train=train, maf=0.05, thr=0.2, min_snps=int(tab["nsnp"].max()) + 1)
    assert few["i"].size == 0
    # every listed pair and a fixed random sample of 500 others, at twice the bound
    rest = at[~sel]
    pick = np.concatenate([lat, np.random.default_rng(7).choice(rest, 500, replace=False)])
    kin = res["tri"][pick]
    rk2, rk0, b2, b0 = (pack_tri(ref[k])[pick] for k in ("k2", "k0", "band2", "band0"))
    ok2, worst2 = within(res["k2"][pick], rk2, b2, factor=2.0)
    close = kin > 2 ** -5.5
    ok0, worst0 = within(res["k0"][pick][close], rk0[close], b0[close], factor=2.0)
    assert np.array_equal(close[:lat.size], np.ones(lat.size, dtype=bool)) and not close[lat.size:].any()
    far = ~close
    rule = same(res["k0"][pick][far], (1.0 - 4.0 * kin[far]) + res["k2"][pick][far])  # below the switch: 1 - 4 kin + k2, restated
    tot = res["k0"] + res["k1"] + res["k2"]
    fin = np.isfinite(tot)
    ulp = float(np.max(np.abs(tot[fin] - 1.0)) / 2.0 ** -52)
    print("%s: %d x %d of %d SNPs (maf 0.05), %d training samples; %d pairs above 2^-5.5 and 500 others against float64 BLAS sums: largest k2 "
          "error / bound %.4f, largest k0 error / bound %.4f over the listed pairs (allowed 2); nearest mu to a threshold %.2e; k0 = 1 - 4 kin + k2 "
          "below the switch bit for bit: %s; largest |k0 + k1 + k2 - 1| %.2f ulp over %d finite entries" % (
              name, N, snps.sum(), P, train.sum(), lat.size, worst2, worst0, ref["margin"], rule, ulp, fin.sum()))
    print("%s: types of the table: %s" % (name, dict(zip(*[a.tolist() for a in np.unique(tab["type"], return_counts=True)]))))
    assert ok2 and ok0 and rule, (worst2, worst0, rule)
    assert ulp <= 4.0, ulp
    # KING's first-degree pairs against the type here: printed and recorded, not asserted (nobody has measured it)
    king = fp.king_related(prefix)
    first = np.isin(king["type"], (1, 2))
    mine = {(int(a), int(b)): int(t) for a, b, t in zip(tab["i"], tab["j"], tab["type"])}
    cross = {}
    for a, b, t in zip(king["i"][first], king["j"][first], king["type"][first]):
        key = (int(t), mine.get((int(a), int(b)), -1))
        cross[key] = cross.get(key, 0) + 1
    print("%s: king_related()'s %d first-degree pairs, (KING type, type here; -1: not listed) -> pairs: %s" % (name, first.sum(), sorted(cross.items())))


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
        f = np.linspace(-0.1, 0.1, N)
        ref = ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta)
        calls = ((lambda p=pcs, **kw: ctx.pcrelate_ibd_block(p, 0, N, 0, N, **kw), "fpca_pcrelate_ibd_block"),
                 (lambda p=pcs, **kw: ctx.pcrelate_ibd_tri(p, **kw), "fpca_pcrelate_ibd_tri"))
        bad = pcs.copy()
        bad[9, 1] = np.nan
        dep = pcs.copy()
        dep[:, 2] = 2.0 * dep[:, 1] - 0.5
        few = np.zeros(N, dtype=bool)
        few[:4] = True
        binf = beta.copy()
        binf[17, 2] = np.inf
        fbad = f.copy()
        fbad[12] = np.nan
        for call, fn in calls:
            refused(lambda: call(np.zeros((N, 32))), fn + ": npc = 32 is outside 0 .. 31")
            refused(lambda: call(bad), fn + r": pcs\[9\]\[1\] is not finite")
            refused(lambda: call(dep), fn + r": \[1 \| pcs\] is rank deficient over the training samples")
            refused(lambda: call(train=few), fn + ": 4 training samples; a regression on 4 columns needs at least 5")
            refused(lambda: call(beta=binf), fn + r": beta\[17\]\[2\] is not finite")
            refused(lambda: call(beta=beta, f=fbad), fn + r": f\[12\] is not finite")
            for eps in (0.5, -0.01, float("nan")):
                refused(lambda: call(beta=beta, eps=eps), fn + ": eps = .* is outside 0 <= eps < 0.5")
        refused(lambda: ctx.pcrelate_ibd_block(pcs, 0, N + 1, 0, N, beta=beta), "are not a non-empty rectangle")
        refused(lambda: ctx.pcrelate_ibd_block(pcs, 0, N, N, 1, beta=beta), "are not a non-empty rectangle")
        refused(lambda: ctx.pcrelate_ibd_block(pcs, 3, 0, 0, N, beta=beta), "are not a non-empty rectangle")
        with pytest.raises(ValueError):
            ctx.pcrelate_ibd_tri(pcs[:-1])
        with pytest.raises(ValueError):
            ctx.pcrelate_ibd_tri(pcs, beta=beta[:, :3])
        with pytest.raises(ValueError):
            ctx.pcrelate_ibd_tri(pcs, f=f[:-1])
        L = fp.lib()
        buf = np.zeros(N * N)
        # all three outputs NULL; pcs NULL with npc > 0; one output alone is enough
        assert L.fpca_pcrelate_ibd_tri(ctx.h, pcs.ctypes.data, 3, None, None, 0.01, None, None, None, None) == -1
        assert b"k2, k0 and nsnp are all NULL" in L.fpca_last_error()
        assert L.fpca_pcrelate_ibd_block(ctx.h, pcs.ctypes.data, 3, None, None, 0.01, None, 0, N, 0, N, None, None, None) == -1
        assert L.fpca_pcrelate_ibd_block(ctx.h, None, 3, None, None, 0.01, None, 0, N, 0, N, buf.ctypes.data, None, None) == -1
        for slot, key in ((0, "k2"), (1, "k0")):
            outs = [None, None, None]
            outs[slot] = buf.ctypes.data
            assert L.fpca_pcrelate_ibd_block(ctx.h, pcs.ctypes.data, 3, beta.ctypes.data, None, 0.01, f.ctypes.data, 0, N, 0, N, *outs) == 0
            assert same(buf.reshape(N, N), ref[key]), key
        n32 = np.zeros((N, N), dtype=np.uint32)
        assert L.fpca_pcrelate_ibd_block(ctx.h, pcs.ctypes.data, 3, beta.ctypes.data, None, 0.01, None, 0, N, 0, N, None, None, n32.ctypes.data) == 0
        assert same(n32, ref["nsnp"])
        ctx.set_sample_mask(np.arange(N) % 3 != 0)
        for call, fn in calls:
            refused(call, fn + ": a sample mask is set")
        ctx.set_sample_mask(None)
        ctx.set_rank(2, 0)
        for call, fn in calls:
            refused(call, fn + ": this context is one shard of several")
        refused(lambda: ctx.bench_pcrelate_ibd(3, 1), "fpca_bench_pcrelate_ibd: this context is one shard of several")
        ctx.set_rank(1, 0)
        again = ctx.pcrelate_ibd_block(pcs, 0, N, 0, N, f=f, beta=beta)
        assert same3(again, ref["k2"], ref["k0"], ref["nsnp"]) and same(ctx.pcrelate_beta(pcs, train=train), beta)  # the context is intact
    with fp.Context.from_dense(np.random.default_rng(2).integers(0, 3, size=(50, 30)).astype(float)) as dense:
        p50 = np.zeros((50, 1))
        refused(lambda: dense.pcrelate_ibd_block(p50, 0, 50, 0, 50), "fpca_pcrelate_ibd_block: this context holds a dense matrix")
        refused(lambda: dense.pcrelate_ibd_tri(p50), "fpca_pcrelate_ibd_tri: this context holds a dense matrix")
    # a block over 1 GiB, met through a wide context of few SNPs
    big_n = 2 ** 14 + 1
    with fp.Context.from_packed(np.full(((big_n + 3) // 4) * 2, 0xFF, dtype=np.uint8), big_n, 2) as wide:
        buf = np.zeros(1)
        assert fp.lib().fpca_pcrelate_ibd_block(wide.h, None, 0, None, None, 0.01, None, 0, big_n, 0, big_n, buf.ctypes.data, None, None) == -1
        msg = fp.lib().fpca_last_error().decode()
        print("refused: %s" % msg)
        assert "16385 x 16385 doubles is over the limit of 1073741824 bytes" in msg


def test_scratch_is_freed_on_every_exit(fp):
    """The pattern of tests/test_gpu_pcrelate.py on the test build: the n-th acquisition of a call is made to fail (FPCA_ENOMEM before the
    runtime is asked for anything) for every n until the call succeeds; after each failure the counts of live device allocations and
    events are what they were, the message names the entry point, and the result after the failures is the result before them.  A call
    acquires the sample-major copy, V, beta, (the factor,) f, three panels, six sums and up to three outputs."""
    c = case(fp, "257x2100")
    N, P, train = c["N"], c["P"], c["train"]
    pcs = make_pcs(N, c["pop"], c["seed"], 3)
    f = np.linspace(-0.1, 0.1, N)
    with fp.test_hooks() as L:
        def live():
            out = (C.c_uint64 * 3)()
            assert L.fpca_debug_scratch_live(out) == 0
            return tuple(int(v) for v in out)

        with fp.Context.from_packed(c["packed"], N, P) as ctx:
            ctx.stats()
            ctx.pcrelate_beta(pcs, train=train)  # (the context's own workspaces of the K2 pass are grown once, outside the counts)

            def tri():
                r = ctx.pcrelate_ibd_tri(pcs, f=f, train=train)
                return r["k2"], r["k0"], r["nsnp"]

            def block():
                r = ctx.pcrelate_ibd_block(pcs, 3, 130, 60, 190, f=f, train=train)
                return r["k2"], r["k0"], r["nsnp"]

            def bench():
                ms, flops = ctx.bench_pcrelate_ibd(3, 2)
                return np.all(ms > 0), flops

            for entry, call, least in (("fpca_pcrelate_ibd_block", block, 16), ("fpca_pcrelate_ibd_tri", tri, 16), ("fpca_bench_pcrelate_ibd", bench, 14)):
                L.fpca_debug_scratch_fail_at(0)
                base = live()
                ref = call()
                assert live() == base, "%s leaks on the success path" % entry
                first_ok, out = None, None
                for n in range(1, 60):
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
