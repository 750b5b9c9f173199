"""Sample subsets (fpca_set_sample_mask, flashpca --keep / --remove / --outpcall) on the GPU against the CPU oracle, which never sees
the feature: the kept columns of the raw 2-bit codes are RE-PACKED with numpy and given to OracleData (dense matrix, mean / sd), and
the held-out rows go through a second OracleData with the training mean / sd preloaded -- the scheme of tests/test_gpu_scca_cv.py.

Every tolerance is one this project already holds the same quantity to (tests/test_gpu_pca.py, tests/test_gpu_kernels.py,
tests/test_gpu_scca_cv.py): statistics array_equal, trace 1e-12 relative, operator 1e-11 of the largest entry (fp32: 2e-6), eigenvalues
1e-9 relative against dense eigh, |u'u_ref| within 1e-8 of 1, U'U within 1e-10 of I, pve 1e-11, the three-step route 1e-5
(test_project.R).  Every test prints what it measured (pytest -s).
Measured on the MI355X (profiles/subset_test_figures.txt): mean / sd array_equal everywhere, trace <= 2.9e-15; operator 1.1e-15 /
5.4e-16 / 7.8e-16 (fp64), 1.0e-15 / 4.5e-16 / 8.3e-16 (exact-integer), 8.5e-7 / 9.6e-8 / 2.9e-7 (fp32), hybrid route 1.0e-15 / 9.6e-16 /
1.7e-15; PCA eigenvalues <= 2.2e-15, |u'u_ref| - 1 <= 1.8e-15, U'U - I <= 2.4e-15 (4.0e-15 at ndim 24), pve <= 8.7e-17, held-out Px
<= 9.5e-16, V <= 1.4e-15; three-step route 1.1e-15 / 1.6e-9 / 3.5e-9; --outpcall against --project 3.2e-14."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HM3 = os.path.join(GOLD, "hapmap3_data")
CHR1 = os.path.join(GOLD, "data_chr1")


@pytest.fixture(scope="module")
def fp(built_lib):
    import flashpca_amd

    return flashpca_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


# ---- the yardstick -----------------------------------------------------------------------------------------
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


def subset_oracle(O, codes, keep, stand="binom2"):
    """The oracle's view of a subset: X of the re-packed kept samples, their mean / sd, X of the other samples under that mean / sd,
    and the trace sum X_kept^2."""
    P = codes.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        od = O.OracleData(packed=pack_codes(codes[:, keep]), N=int(keep.sum()), P=P, stand=stand)
        Xs, ms = od.dense(), od.meansd()
        Xh = np.zeros((0, P))
        if (~keep).any():
            oh = O.OracleData(packed=pack_codes(codes[:, ~keep]), N=int((~keep).sum()), P=P, stand=stand)
            oh.set_preloaded_meansd(ms)
            Xh = oh.dense()
    return Xs, ms, Xh, float(np.sum(Xs * Xs))


def masks_for(N):
    rng = np.random.default_rng(20261017)
    m = {"random70": rng.random(N) < 0.7, "first600": np.arange(N) < 600, "every4th_out": np.arange(N) % 4 != 3}
    odd = np.zeros(N, dtype=bool)
    odd[rng.choice(N, 501, replace=False)] = True  # 501 kept samples: not a multiple of 4
    m["count_not_multiple_of_4"] = odd
    assert int(odd.sum()) % 4 != 0 and int(m["first600"].sum()) == 600
    return m


def subset_classes(codes, keep):
    """SNPs monomorphic among the kept samples but not overall, and SNPs all-missing among the kept samples (numpy, on the raw codes)."""
    def mono(c):
        good = c != 1
        n = good.sum(axis=1)
        return (n > 0) & ((((c == 0) & good).sum(axis=1) == n) | (((c == 2) & good).sum(axis=1) == n) | (((c == 3) & good).sum(axis=1) == n))

    sub = codes[:, keep]
    return mono(sub) & ~mono(codes), (sub != 1).sum(axis=1) == 0


@pytest.fixture(scope="module")
def hm3():
    codes, N, P = read_bed_codes(HM3)
    return dict(codes=codes, N=N, P=P, masks=masks_for(N))


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---- 1. statistics bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hapmap3_data", "data_chr1"])
@pytest.mark.parametrize("stand", ["binom2", "binom"])
def test_masked_statistics_bit_for_bit(fp, O, name, stand):
    codes, N, P = read_bed_codes(os.path.join(GOLD, name))
    with fp.Context.from_bed(os.path.join(GOLD, name + ".bed"), N, stand=stand, accum="auto") as ctx:
        assert ctx.nkept == N
        for mname, keep in masks_for(N).items():
            Xs, ms_ref, _, tr_ref = subset_oracle(O, codes, keep, stand)
            ctx.set_sample_mask(keep)
            assert ctx.nkept == int(keep.sum())
            ms, tr = ctx.stats()
            print("%s %s %s: kept %d, trace rel err %.2e" % (name, stand, mname, keep.sum(), abs(tr - tr_ref) / tr_ref))
            assert np.array_equal(ms, ms_ref, equal_nan=True), (name, stand, mname)
            assert abs(tr - tr_ref) <= 1e-12 * tr_ref
            if name == "hapmap3_data" and mname == "first600":
                # checked with numpy: exactly one SNP is monomorphic among the first 600 samples and not overall, none is all-missing --
                # the zero-column rule is really exercised
                mono_new, allmiss = subset_classes(codes, keep)
                assert int(mono_new.sum()) == 1 and int(allmiss.sum()) == 0
                j = int(np.argmax(mono_new))
                assert ms[j, 1] == 0.0 and np.all(Xs[:, j] == 0.0)
                B = np.random.default_rng(3).standard_normal((N, 16))
                T = ctx.apply_xt(B)
                assert np.all(T[j] == 0.0) and np.abs(T).max() > 0
        ctx.set_sample_mask(None)
        assert ctx.nkept == N
        with np.errstate(invalid="ignore", divide="ignore"):
            od = O.OracleData(os.path.join(GOLD, name + ".bed"), N, stand)
            od.dense()  # (the oracle takes its statistics while it reads the blocks)
            assert np.array_equal(ctx.stats()[0], od.meansd(), equal_nan=True)


def test_masked_statistics_small_matrix_with_an_all_missing_snp(fp, O):
    """A numpy-made 203 x 64 matrix, 2 % missing calls, one SNP all-missing among the kept samples (it has calls among the others) and
    one monomorphic among them: mean / sd as K1 makes them of such SNPs (NaN / 0: zero columns), the operator stays finite."""
    rng = np.random.default_rng(11)
    N, P = 203, 64
    codes = rng.choice(np.array([3, 2, 0], dtype=np.uint8), size=(P, N), p=[0.5, 0.35, 0.15])
    codes[rng.random((P, N)) < 0.02] = 1
    keep = rng.random(N) < 0.6
    codes[7, keep] = 1    # all-missing among the kept samples
    codes[7, ~keep] = 2
    codes[9, keep] = 3    # monomorphic among the kept samples
    mono_new, allmiss = subset_classes(codes, keep)
    assert allmiss[7] and int(allmiss.sum()) == 1 and mono_new[9]
    Xs, ms_ref, Xh, tr_ref = subset_oracle(O, codes, keep)
    assert np.isnan(ms_ref[7, 0]) and np.all(Xs[:, 7] == 0) and np.all(Xh[:, 7] == 0) and np.all(Xs[:, 9] == 0)
    B = rng.standard_normal((N, 16))
    T = rng.standard_normal((P, 16))
    for accum in ("auto", "fp64"):
        with fp.Context.from_packed(pack_codes(codes), N, P, accum=accum) as ctx:
            ctx.set_sample_mask(keep)  # (on a fresh context: this is the context's first pass over the matrix)
            ms, tr = ctx.stats()
            assert np.array_equal(ms, ms_ref, equal_nan=True) and abs(tr - tr_ref) <= 1e-12 * tr_ref
            Y = ctx.apply_xxt(B)
            ref = Xs @ (Xs.T @ B[keep])
            assert np.isfinite(Y).all() and relmax(Y[keep], ref) <= 1e-11 and np.all(Y[~keep] == 0.0)
            Z = ctx.apply_x(T)
            assert relmax(Z[keep], Xs @ T) <= 1e-11 and relmax(Z[~keep], Xh @ T) <= 1e-11


# ---- 2. operator -------------------------------------------------------------------------------------------
def check_operator(ctx, keep, Xs, Xh, tol, rng, label, b=20):
    N, P = keep.size, Xs.shape[1]
    B, T = rng.standard_normal((N, b)), rng.standard_normal((P, b))
    B[~keep] *= 7.0  # (the held-out rows of B count as zero, however large)
    t_ref = Xs.T @ B[keep]
    e_t = relmax(ctx.apply_xt(B), t_ref)
    Y = ctx.apply_xxt(B)
    e_y = relmax(Y[keep], Xs @ t_ref)
    full = np.zeros((N, b))
    full[keep], full[~keep] = Xs @ T, Xh @ T
    e_x = relmax(ctx.apply_x(T), full)
    print("%s: apply_xt %.2e, apply_xxt (kept rows) %.2e, apply_x (all rows) %.2e" % (label, e_t, e_y, e_x))
    assert e_t <= tol and e_y <= tol and e_x <= tol, (label, e_t, e_y, e_x)
    assert np.all(Y[~keep] == 0.0), label
    return e_t, e_y, e_x


class DeviceBlocks:
    """Row-major host blocks copied to device memory through the HIP runtime the library itself runs on."""
    hip = None

    def __init__(self, *arrays):
        self.arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
        if DeviceBlocks.hip is None:
            for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
                try:
                    DeviceBlocks.hip = C.CDLL(name)
                    break
                except OSError:
                    pass
        assert DeviceBlocks.hip is not None

    def __enter__(self):
        self.ptrs = []
        for a in self.arrays:
            p = C.c_void_p()
            assert DeviceBlocks.hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
            assert DeviceBlocks.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
            self.ptrs.append(p)
        return self.ptrs

    def __exit__(self, *a):
        for p in self.ptrs:
            DeviceBlocks.hip.hipFree(p)

    @staticmethod
    def to_host(p, shape):
        out = np.empty(shape)
        assert DeviceBlocks.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        return out


@pytest.mark.parametrize("accum,tol", [("fp64", 1e-11), ("auto", 1e-11), ("fp32", 2e-6)])
def test_masked_operator(fp, O, hm3, accum, tol):
    keep = hm3["masks"]["random70"]
    Xs, _, Xh, _ = subset_oracle(O, hm3["codes"], keep)
    rng = np.random.default_rng(5)
    with fp.Context.from_bed(HM3 + ".bed", hm3["N"], accum=accum) as ctx:
        ctx.set_sample_mask(keep)
        e = check_operator(ctx, keep, Xs, Xh, tol, rng, "hapmap3_data %s" % accum)
        if accum == "fp32":
            assert max(e) > 1e-12  # (really fp32)
        # the device-resident entry point: the caller's block is not modified, the held-out rows of the result are exactly zero
        rows, b = ctx.block_rows(), 16
        B = rng.standard_normal((hm3["N"], b))
        Bh = np.zeros((rows, b))
        Bh[: hm3["N"]] = B
        Y = np.full((rows, b), 3.0)
        with DeviceBlocks(Bh, Y) as (dB, dY):
            ctx.apply_xxt_dev(dB.value, b, dY.value)
            ctx.synchronize()
            B_after = DeviceBlocks.to_host(dB, Bh.shape)
            Y = DeviceBlocks.to_host(dY, Y.shape)
        assert np.array_equal(B_after, Bh)
        assert relmax(Y[: hm3["N"]][keep], Xs @ (Xs.T @ B[keep])) <= tol
        assert np.all(Y[: hm3["N"]][~keep] == 0.0) and np.all(Y[hm3["N"]:] == 0.0)
        assert np.array_equal(Y[: hm3["N"]], ctx.apply_xxt(B))  # (the host entry point runs the same kernels)


def test_masked_operator_on_the_hybrid_missing_call_route(fp, O):
    """The realistic profile (missing calls concentrated in few SNPs) takes the hybrid route; the route is the packed matrix's, so it is
    the same with and without a mask."""
    N, P = 3000, 2000
    rng = np.random.default_rng(6)
    keep = rng.random(N) < 0.7
    with fp.Context.synthetic(N, P, n_pop=3, realistic=True, accum="auto") as ctx:
        codes = unpack_codes(ctx.download_packed(), N, P)
        assert ctx.missing_mode(16) == 4
        ctx.set_sample_mask(keep)
        mode = ctx.missing_mode(16)
        print("missing-call route under the mask: %d" % mode)
        assert mode == 4
        Xs, ms_ref, Xh, tr_ref = subset_oracle(O, codes, keep)
        ms, tr = ctx.stats()
        assert np.array_equal(ms, ms_ref, equal_nan=True) and abs(tr - tr_ref) <= 1e-12 * tr_ref
        check_operator(ctx, keep, Xs, Xh, 1e-11, rng, "realistic profile, hybrid route", b=16)
        check_operator(ctx, keep, Xs, Xh, 1e-11, rng, "realistic profile, hybrid route", b=20)
        assert ctx.missing_mode(16) == 4
        r = ctx.pca(ndim=5, tol=1e-8)
        w = np.linalg.eigvalsh(Xs @ Xs.T)[::-1][:5] / P
        assert np.max(np.abs(r["d"] - w) / w) <= 1e-9
        ctx.set_sample_mask(None)
        assert ctx.missing_mode(16) == 4


# ---- 3. PCA ------------------------------------------------------------------------------------------------
def check_pca(r, keep, Xs, Xh, tr_ref, ms_ref, P, k, div, label, vectors=True):
    nk = int(keep.sum())
    divv = {"p": float(P), "n1": nk - 1.0, "none": 1.0}[div]
    w, Q = np.linalg.eigh(Xs @ Xs.T)
    w, Q = w[::-1][:k] / divv, Q[:, ::-1][:, :k]
    gaps = np.min(np.abs(np.diff(np.r_[w, np.linalg.eigvalsh(Xs @ Xs.T)[::-1][k] / divv])) / w)
    U, d, Px, V = r["U"], r["d"], r["Px"], r["V"]
    e_d = float(np.max(np.abs(d - w) / w))
    e_u = float(np.max(np.abs(np.abs(np.sum(U[keep] * Q, axis=0)) - 1.0)))
    e_o = float(np.max(np.abs(U.T @ U - np.eye(k))))
    e_pve = float(np.max(np.abs(r["pve"] - w / (tr_ref / divv))))
    proj_ref = Xh @ V / np.sqrt(divv)
    e_px = relmax(Px[~keep], proj_ref)
    v_ref = Xs.T @ U[keep] / np.sqrt(d) / np.sqrt(divv)
    e_v = float(np.max(np.abs(V - v_ref)) / np.max(np.abs(v_ref)))
    print("%s: smallest relative gap %.3f, eigenvalues %.2e, |u'u_ref| - 1 %.2e, U'U - I %.2e, pve %.2e, held-out Px %.2e, V %.2e, "
          "%d block applies" % (label, gaps, e_d, e_u, e_o, e_pve, e_px, e_v, r["info"]["block_applies"]))
    assert e_d <= 1e-9 and (e_u <= 1e-8 or not vectors) and e_o <= 1e-10 and e_pve <= 1e-11, label
    assert np.all(U[~keep] == 0.0), label
    assert np.allclose(Px[keep], U[keep] * np.sqrt(d), rtol=1e-14, atol=0), label
    assert e_px <= 1e-11 and e_v <= 1e-11, label
    assert np.array_equal(r["meansd"], ms_ref, equal_nan=True), label
    assert abs(r["info"]["trace"] - tr_ref / divv) <= 1e-12 * tr_ref / divv
    assert r["info"]["converged"] == 1


@pytest.mark.parametrize("mname", ["random70", "first600", "every4th_out"])
def test_masked_pca(fp, O, hm3, mname):
    """(measured with numpy: the smallest relative gap among the top ten eigenvalues is 2.0 %, 1.1 % and 2.8 % for the three masks, so
    the comparison up to sign is well posed)"""
    keep = hm3["masks"][mname]
    Xs, ms_ref, Xh, tr_ref = subset_oracle(O, hm3["codes"], keep)
    with fp.Context.from_bed(HM3 + ".bed", hm3["N"], accum="auto") as ctx:
        ctx.set_sample_mask(keep)
        r = ctx.pca(ndim=10, tol=1e-8, do_loadings=True)
        check_pca(r, keep, Xs, Xh, tr_ref, ms_ref, hm3["P"], 10, "p", "hapmap3_data %s" % mname)
        if mname == "random70":
            r = ctx.pca(ndim=10, tol=1e-8, do_loadings=True, div="n1")  # divisor n_kept - 1
            check_pca(r, keep, Xs, Xh, tr_ref, ms_ref, hm3["P"], 10, "n1", "hapmap3_data %s, div n1" % mname)
            # more components than one block holds: two Ritz blocks of loadings (the gaps further down the spectrum were not measured,
            # so the eigenvectors are not compared with eigh's one by one; everything else is)
            r = ctx.pca(ndim=24, tol=1e-8, do_loadings=True)
            check_pca(r, keep, Xs, Xh, tr_ref, ms_ref, hm3["P"], 24, "p", "hapmap3_data %s, ndim 24" % mname, vectors=False)
            r2 = ctx.pca(ndim=10, tol=1e-8)  # no loadings asked for: the K2 + K3 pass after the solve runs all the same
            assert r2["V"] is None
            r1 = ctx.pca(ndim=10, tol=1e-8, do_loadings=True)
            assert np.array_equal(r2["Px"], r1["Px"]) and np.array_equal(r2["U"], r1["U"])


@pytest.mark.parametrize("accum", ["auto", "fp64"])
def test_masked_pca_dimension_limit_and_direct_route(fp, O, hm3, accum):
    """41 kept samples: ndim may be (min(41, P) - 1) / 2 = 20 and not 21 (957 samples would allow 478), and 41 < 3 x 16 takes the
    small-N direct route: ceil(41 / 16) = 3 applies on the identity of the KEPT samples, a dense eigendecomposition on the host."""
    N, P = hm3["N"], hm3["P"]
    keep = np.zeros(N, dtype=bool)
    keep[np.random.default_rng(8).choice(N, 41, replace=False)] = True
    Xs, ms_ref, Xh, tr_ref = subset_oracle(O, hm3["codes"], keep)
    with fp.Context.from_bed(HM3 + ".bed", N, accum=accum) as ctx:
        ctx.set_sample_mask(keep)
        with pytest.raises(fp.FpcaError, match="You asked for 21 dimensions, but only 20 allowed") as e:
            ctx.pca(ndim=21)
        assert e.value.code == -1
        for k in (5, 20):
            r = ctx.pca(ndim=k, tol=1e-8, do_loadings=True)
            assert r["info"]["block_applies"] == 3, r["info"]
            check_pca(r, keep, Xs, Xh, tr_ref, ms_ref, P, k, "p", "41 kept samples, ndim %d, %s" % (k, accum))
        ctx.set_sample_mask(None)
        with pytest.raises(fp.FpcaError, match="You asked for 479 dimensions, but only 478 allowed"):
            ctx.pca(ndim=479)
        assert ctx.pca(ndim=21, tol=1e-6)["info"]["block_applies"] > 3


# ---- 4. equivalence with the three-step route ---------------------------------------------------------------
def test_equivalence_with_the_three_step_route(fp, O, hm3):
    """A second .bed of the subset -> PCA with loadings and mean/sd -> projection of the other samples (what flashpca_amd.project() does
    with a PLINK input: mean/sd preloaded, apply_x on the loadings, / sqrt(div)), through the existing public interface, against ONE
    masked run."""
    keep = hm3["masks"]["random70"]
    codes, N, P = hm3["codes"], hm3["N"], hm3["P"]
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        ctx.set_sample_mask(keep)
        m = ctx.pca(ndim=10, tol=1e-8, do_loadings=True)
    with fp.Context.from_packed(pack_codes(codes[:, keep]), int(keep.sum()), P, accum="auto") as sub:
        s = sub.pca(ndim=10, tol=1e-8, do_loadings=True)
    with fp.Context.from_packed(pack_codes(codes[:, ~keep]), int((~keep).sum()), P, accum="auto") as held:
        held.set_meansd(s["meansd"])
        proj = held.apply_x(s["V"]) / np.sqrt(P)
    sg = np.sign(np.sum(m["U"][keep] * s["U"], axis=0))
    e_d = float(np.max(np.abs(m["d"] - s["d"]) / s["d"]))
    e_p = relmax(m["Px"][~keep] * sg, proj)
    e_k = relmax(m["Px"][keep] * sg, s["Px"])
    print("masked run against the three-step route: eigenvalues %.2e, held-out projections %.2e, kept PCs %.2e" % (e_d, e_p, e_k))
    assert e_d <= 1e-9 and e_p <= 1e-5 and e_k <= 1e-5
    assert np.array_equal(m["meansd"], s["meansd"], equal_nan=True)
    # the scripting entry point: what a run on the subset fileset returns, plus projection_all
    f = fp.flashpca(HM3, ndim=10, tol=1e-8, do_loadings=True, keep=keep)
    nk = int(keep.sum())
    assert f["vectors"].shape == (nk, 10) and f["projection"].shape == (nk, 10) and f["projection_all"].shape == (N, 10)
    assert np.array_equal(f["vectors"], m["U"][keep]) and np.array_equal(f["projection"], m["Px"][keep]) and np.array_equal(f["projection_all"], m["Px"])
    assert np.array_equal(f["center"], s["meansd"][:, 0], equal_nan=True) and np.array_equal(f["scale"], s["meansd"][:, 1], equal_nan=True)
    assert np.array_equal(f["values"], m["d"]) and np.array_equal(f["loadings"], m["V"])
    g = fp.flashpca(HM3, ndim=10, tol=1e-8)
    assert "projection_all" not in g and g["vectors"].shape == (N, 10)


# ---- 5. the context is left as it was ------------------------------------------------------------------------
def context_fingerprint(ctx, Y, B):
    ms, tr = ctx.stats()
    p = ctx.pca(ndim=3)
    return dict(ms=ms, tr=np.array(tr), xxt=ctx.apply_xxt(B), ucca=ctx.ucca(Y, standy="sd"), pca=p["d"], pcaU=p["U"], pcaPx=p["Px"],
                mode=np.array(ctx.missing_mode(16)), nkept=np.array(ctx.nkept))


@pytest.mark.parametrize("accum", ["auto", "fp64"])
def test_context_is_left_as_it_was(fp, hm3, accum):
    N = hm3["N"]
    rng = np.random.default_rng(4)
    Y, B = rng.standard_normal((N, 4)), rng.standard_normal((N, 16))
    keep = hm3["masks"]["random70"]
    with fp.Context.from_bed(HM3 + ".bed", N, accum=accum) as ctx:
        before = context_fingerprint(ctx, Y, B)
        ctx.set_sample_mask(keep)
        a = ctx.pca(ndim=5, tol=1e-8, do_loadings=True)
        b = ctx.pca(ndim=5, tol=1e-8, do_loadings=True)
        for kk in ("U", "d", "Px", "pve", "V", "meansd"):
            assert np.array_equal(a[kk], b[kk], equal_nan=True), kk  # a repeat call is bit-identical
        assert np.array_equal(ctx.apply_xxt(B), ctx.apply_xxt(B))
        ctx.set_sample_mask(hm3["masks"]["first600"])  # one mask replaces another
        ctx.set_sample_mask(keep)
        c = ctx.pca(ndim=5, tol=1e-8, do_loadings=True)
        for kk in ("U", "d", "Px", "pve", "V", "meansd"):
            assert np.array_equal(a[kk], c[kk], equal_nan=True), kk
        ctx.set_sample_mask(None)
        after = context_fingerprint(ctx, Y, B)
        for kk in before:
            assert np.array_equal(before[kk], after[kk], equal_nan=True), kk
        # calls that fail leave everything where it was: with a mask set ...
        ctx.set_sample_mask(keep)
        masked_ref = (ctx.stats()[0], ctx.apply_xxt(B))
        one = np.zeros(N, dtype=bool)
        one[5] = True
        for call in (lambda: ctx.set_sample_mask(one), lambda: ctx.check(a["U"], a["d"]), lambda: ctx.ucca(Y), lambda: ctx.set_meansd(before["ms"]),
                     lambda: ctx.pca(ndim=400), lambda: ctx.set_rank(2, 0)):
            with pytest.raises(fp.FpcaError) as e:
                call()
            assert e.value.code == -1
        assert ctx.nkept == int(keep.sum())
        assert np.array_equal(ctx.stats()[0], masked_ref[0], equal_nan=True) and np.array_equal(ctx.apply_xxt(B), masked_ref[1])
        ctx.set_sample_mask(None)
        # ... and without one
        with pytest.raises(fp.FpcaError):
            ctx.set_sample_mask(one)
        with pytest.raises(ValueError):
            ctx.set_sample_mask(keep[:-1])
        after = context_fingerprint(ctx, Y, B)
        for kk in before:
            assert np.array_equal(before[kk], after[kk], equal_nan=True), kk
    # a mask set on a FRESH context (its first pass over the matrix) and cleared: indistinguishable from a fresh context
    with fp.Context.from_bed(HM3 + ".bed", N, accum=accum) as ctx:
        ctx.set_sample_mask(keep)
        ctx.set_sample_mask(None)
        after = context_fingerprint(ctx, Y, B)
        for kk in before:
            assert np.array_equal(before[kk], after[kk], equal_nan=True), kk


# ---- 6. refusals ---------------------------------------------------------------------------------------------
def test_refusals(fp, hm3):
    N = hm3["N"]
    keep = hm3["masks"]["random70"]
    rng = np.random.default_rng(9)
    Y = rng.standard_normal((N, 3))

    def refused(call, msg):
        with pytest.raises(fp.FpcaError, match=msg) as e:
            call()
        assert e.value.code == -1

    with fp.Context.from_dense(rng.integers(0, 3, size=(50, 30)).astype(float)) as dense:
        refused(lambda: dense.set_sample_mask(np.arange(50) < 30), "dense matrix, of which only the standardised copy is kept")
        dense.set_sample_mask(None)  # (clearing what is not set is no error)
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        for n in (0, 1):
            few = np.zeros(N, dtype=bool)
            few[:n] = True
            refused(lambda: ctx.set_sample_mask(few), "the mask keeps %d of %d samples; at least 2 are needed" % (n, N))
        two = np.zeros(N, dtype=bool)
        two[[3, 900]] = True
        ctx.set_sample_mask(two)
        assert ctx.nkept == 2
        ctx.set_sample_mask(keep)
        # follow-ups: these do not run under a mask
        refused(lambda: ctx.check(np.zeros((N, 2)), np.ones(2)), "fpca_check: a sample mask is set")
        refused(lambda: ctx.ucca(Y), "fpca_ucca: a sample mask is set")
        refused(lambda: ctx.scca_prepare(Y), "fpca_scca_prepare: a sample mask is set")
        refused(lambda: ctx.scca_fit(1e-3, 1e-3, 1, np.ones((3, 1))), "fpca_scca_fit: a sample mask is set")
        refused(lambda: ctx.scca_cv(Y, np.arange(N) % 3, [1e-3], [1e-3], 1, np.ones((3, 1))), "fpca_scca_cv: a sample mask is set")
        # a preloaded mean/sd and a mask exclude each other, in either order
        refused(lambda: ctx.set_meansd(ctx.stats()[0]), "fpca_set_meansd: a sample mask is set")
        # a masked context does not become one shard of several
        refused(lambda: ctx.set_rank(2, 0), "fpca_set_rank: a sample mask is set .* single context only")
        refused(lambda: ctx.set_allreduce(lambda ptr, count, stream: 0), "fpca_set_allreduce: a sample mask is set")
        refused(lambda: ctx.set_collectives(lambda *a: 0, lambda *a: 0), "fpca_set_collectives: a sample mask is set")
        refused(lambda: ctx.comm_init_rank(2, 0, bytes(128)), "fpca_comm_init_rank: a sample mask is set")
        ctx.set_rank(1, 0)  # (one rank is no sharding)
        assert ctx.nkept == int(keep.sum()) and ctx.pca(ndim=3)["info"]["converged"] == 1
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        ctx.set_meansd(ctx.stats()[0])
        refused(lambda: ctx.set_sample_mask(keep), "preloaded mean/sd")
    msg = "the context is one shard of several"
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        ctx.set_rank(2, 0)
        refused(lambda: ctx.set_sample_mask(keep), msg)
    with fp.Context.from_bed(HM3 + ".bed", N, accum="auto") as ctx:
        ctx.set_allreduce(lambda ptr, count, stream: 0)
        refused(lambda: ctx.set_sample_mask(keep), msg)
        assert ctx.nkept == N


# ---- 7. command line -----------------------------------------------------------------------------------------
def _tab(path, skip=2):
    return np.array([l.split("\t")[skip:] for l in open(path).read().splitlines()[1:]], dtype=float)


def _labels(path):
    return [tuple(l.split("\t")[:2]) for l in open(path).read().splitlines()[1:]]


def write_fileset(prefix, codes, fam_lines, bim_text):
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(pack_codes(codes).tobytes())
    open(prefix + ".fam", "w").write("".join(fam_lines))
    open(prefix + ".bim", "w").write(bim_text)


def test_cli_keep_remove_outpcall(fp, tmp_path):
    codes, N, P = read_bed_codes(CHR1)
    fam = open(CHR1 + ".fam").read().splitlines(keepends=True)
    bim = open(CHR1 + ".bim").read()
    keep = np.random.default_rng(12).random(N) < 0.7
    kept, held = np.flatnonzero(keep), np.flatnonzero(~keep)
    write_fileset(str(tmp_path / "sub"), codes[:, keep], [fam[i] for i in kept], bim)
    write_fileset(str(tmp_path / "held"), codes[:, ~keep], [fam[i] for i in held], bim)
    # the keep list carries duplicates and further columns; the remove list is the complement
    lines = [" ".join(fam[i].split()[:2]) + " x\n" for i in list(kept) + list(kept[:7])]
    (tmp_path / "keep.txt").write_text("".join(lines))
    (tmp_path / "remove.txt").write_text("".join("\t".join(fam[i].split()[:2]) + "\n" for i in held))
    common = ["--ndim", "5", "--tol", "1e-9", "--precision", "14", "--notime", "--outload", "load.txt", "--outmeansd", "ms.txt"]

    def cli(name, args):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run([fp.CLI_PATH] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return d

    d_sub = cli("run_sub", ["--bfile", str(tmp_path / "sub")] + common)
    d_keep = cli("run_keep", ["--bfile", CHR1, "--keep", str(tmp_path / "keep.txt"), "--outpcall", "pcall.txt"] + common)
    d_rem = cli("run_remove", ["--bfile", CHR1, "--remove", str(tmp_path / "remove.txt"), "--outpcall", "pcall.txt"] + common)
    assert not (d_sub / "pcall.txt").exists()  # (written only when asked for)
    e_sub, e_keep = np.loadtxt(d_sub / "eigenvalues.txt"), np.loadtxt(d_keep / "eigenvalues.txt")
    assert np.max(np.abs(e_keep - e_sub) / e_sub) <= 1e-9
    assert np.max(np.abs(np.loadtxt(d_keep / "pve.txt") - np.loadtxt(d_sub / "pve.txt"))) <= 1e-9
    U_sub, U_keep = _tab(d_sub / "eigenvectors.txt"), _tab(d_keep / "eigenvectors.txt")
    assert U_keep.shape == (kept.size, 5)
    sg = np.sign(np.sum(U_sub * U_keep, axis=0))
    for f in ("eigenvectors.txt", "pcs.txt", "load.txt"):
        a, b = _tab(d_sub / f), _tab(d_keep / f)
        assert a.shape == b.shape and np.max(np.abs(b * sg - a)) <= 1e-6 * max(1.0, np.max(np.abs(a))), f
        assert _labels(d_sub / f) == _labels(d_keep / f), f
    m_sub, m_keep = _tab(d_sub / "ms.txt"), _tab(d_keep / "ms.txt")
    assert _labels(d_sub / "ms.txt") == _labels(d_keep / "ms.txt")
    assert np.allclose(m_keep, m_sub, rtol=1e-9, atol=0, equal_nan=True)
    # --remove with the complementary list: the same files
    for f in ("eigenvalues.txt", "eigenvectors.txt", "pcs.txt", "pve.txt", "load.txt", "ms.txt", "pcall.txt"):
        assert open(d_keep / f, "rb").read() == open(d_rem / f, "rb").read(), f
    # --outpcall: all N samples in .fam order; the kept rows are the pcs file's, the others are --project of the held-out fileset with
    # this run's loadings and mean/sd (which the files carry to 14 digits)
    all_lines = open(d_keep / "pcall.txt").read().splitlines()
    pcs_lines = open(d_keep / "pcs.txt").read().splitlines()
    assert len(all_lines) == N + 1 and all_lines[0] == pcs_lines[0]
    assert [all_lines[1 + i] for i in kept] == pcs_lines[1:]
    assert _labels(d_keep / "pcall.txt") == [tuple(l.split()[:2]) for l in fam]
    d_proj = cli("run_project", ["--bfile", str(tmp_path / "held"), "--project", "--inload", str(d_keep / "load.txt"), "--inmeansd", str(d_keep / "ms.txt"),
                                 "--outproj", "proj.txt", "--precision", "14", "--notime"])
    proj, pall = _tab(d_proj / "proj.txt"), _tab(d_keep / "pcall.txt")
    assert proj.shape == (held.size, 5)
    e_p = relmax(pall[held], proj)
    print("--outpcall against --project of the held-out fileset: %.2e" % e_p)
    assert e_p <= 1e-11
    assert _labels(d_proj / "proj.txt") == [tuple(fam[i].split()[:2]) for i in held]
    # without a subset --outpcall is the pcs file
    d_all = cli("run_all", ["--bfile", CHR1, "--ndim", "5", "--notime", "--outpcall", "pcall.txt"])
    assert open(d_all / "pcall.txt", "rb").read() == open(d_all / "pcs.txt", "rb").read()
