"""Per-call device scratch is given back on every way out (csrc/dev_scratch.hpp): DevMem / PinnedMem / DevEvent.

The test build counts the live objects of the three kinds (fpca_debug_scratch_live) and can make the n-th acquisition from now throw
FPCA_ENOMEM before the runtime is asked for anything (fpca_debug_scratch_fail_at): a host-side exception, nothing fails on the device.
For every entry point that owns scratch, with one synthetic fp64 context of 600 samples x 520 SNPs at 1 % missing calls (N_pad = 1024,
three 256-SNP tiles, two 64-record LD / KING tiles per side and a non-zero N % 4 pad) and a .bed of the same matrix:

  1. the call once un-injected: outputs kept, and the live counts are what they were before it (no leak on the success path);
  2. n = 1, 2, ...: the n-th acquisition fails; while the call fails it returns exactly FPCA_ENOMEM, fpca_last_error names the entry
     point and the three live counts are back at the baseline.  The first n at which the call succeeds is at least 2 (the call does
     acquire through the owners) and at most 64 (a countdown that never fires cannot pass for success; the largest count of a call
     below is 16, fpca_scca_cv's: the last one is the first fit's workspace, taken while the folds' standardisation is installed);
  3. that call's outputs equal the kept ones, and fpca_stats and one 16-column apply_xxt give the bits they gave before the injections
     (for fpca_scca_cv: its guard put the standardisation back after every failure).

fpca_debug_k4_fused_bench alone runs on a second context, 7,700 x 260: its kernel exists from 8,192 block rows on.
The countdown counts events and pinned allocations beside device allocations: fpca_bench_stats owns two events and nothing else.
Times are not results: of the measurement hooks the byte / MAC counts are compared, and the times only checked to be positive.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P = 600, 520
ENOMEM = -4


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def env(built_lib, tmp_path_factory):
    import flashpca_amd as fp

    with fp.test_hooks() as L:
        with fp.Context.synthetic(N, P, n_pop=4, missing_rate=0.01, accum="fp64") as ctx:
            packed = ctx.download_packed()
            bed = str(tmp_path_factory.mktemp("scratch") / "s.bed")
            with open(bed, "wb") as f:
                f.write(bytes([0x6C, 0x1B, 0x01]))
                f.write(packed.tobytes())
            rng = np.random.default_rng(11)
            yield dict(fp=fp, L=L, ctx=ctx, packed=packed, bed=bed, Y=rng.standard_normal((N, 3)), B=rng.standard_normal((N, 16)),
                       folds=np.arange(N) % 2, keep=rng.random(N) < 0.7, snps=rng.random(P) < 0.5)
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


def _run(env, entry, call, ctx=None):
    """call() -> tuple of arrays; raises FpcaError on failure"""
    fp, L = env["fp"], env["L"]
    ctx = env["ctx"] if ctx is None else ctx
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


def test_product_build_has_no_counters(built_lib):
    import flashpca_amd as fp

    L = fp._lib._load(fp.LIB_PATH)  # (the product, whichever library lib() currently answers with)
    out = (C.c_uint64 * 3)()
    assert L.fpca_debug_scratch_live(out) == -1 and b"product build" in L.fpca_last_error()
    assert L.fpca_debug_scratch_fail_at(1) == -1 and b"product build" in L.fpca_last_error()


def test_ucca(env):
    _run(env, "fpca_ucca", lambda: (env["ctx"].ucca(env["Y"]),))


def test_scca_prepare_and_cv(env):
    ctx, Y = env["ctx"], env["Y"]
    V0 = np.ones((3, 1))

    def prepare():
        ctx.scca_prepare(Y)
        env["L"].fpca_debug_scratch_fail_at(0)  # (the fit only reads what the call under test left: C)
        r = ctx.scca_fit(0.01, 0.01, 1, V0)
        return r["U"], r["V"], r["d"]

    _run(env, "fpca_scca_prepare", prepare)

    def cv():
        r = ctx.scca_cv(Y, env["folds"], [0.005, 0.01], [0.005, 0.01], 1, V0, return_pred=True)
        return r["corr"], r["nzero_x"], r["nzero_y"], r["iters"], r["xpred"], r["ypred"]

    _run(env, "fpca_scca_cv", cv)


def test_king(env):
    ctx = env["ctx"]
    _run(env, "fpca_king_block", lambda: (ctx.king_block(3, 130, 60, 200),))
    _run(env, "fpca_king_pairs", lambda: ctx.king_pairs(-0.05, keep=env["keep"]))
    _run(env, "fpca_king_cutoff", lambda: (ctx.king_cutoff(-0.02, keep=env["keep"]),))

    def bench():
        ms, macs = ctx.bench_king(2)
        return np.all(ms > 0), macs

    _run(env, "fpca_bench_king", bench)


def test_ld(env):
    ctx = env["ctx"]
    _run(env, "fpca_ld_band", lambda: (ctx.ld_band(5, 500, 70),))
    _run(env, "fpca_ld_prune", lambda: (ctx.ld_prune(window=50, step=5, r2=0.02),))

    def bench():
        ms, macs = ctx.bench_ld(70, 2)
        return np.all(ms > 0), macs

    _run(env, "fpca_bench_ld", bench)


def test_sample_mask(env):
    ctx = env["ctx"]
    try:
        _run(env, "fpca_set_sample_mask", lambda: (ctx.set_sample_mask(env["keep"]), ctx.nkept)[1:])
    finally:
        ctx.set_sample_mask(None)


def test_snp_subset(env):
    ctx = env["ctx"]

    def subset():
        with ctx.snp_subset(env["snps"]) as sub:
            return (sub.download_packed(),)

    _run(env, "fpca_create_snp_subset", subset)

    def bench():
        ms, nbytes = ctx.snp_subset_bench(env["snps"], 2)
        return ms > 0, nbytes

    _run(env, "fpca_debug_snp_subset_bench", bench)


def test_create_from_bed(env):
    fp = env["fp"]

    def upload():
        with fp.Context.from_bed(env["bed"], N) as c:
            return (c.download_packed(),)  # (nothing here that takes scratch of its own: the countdown is for the upload)

    assert np.array_equal(upload()[0], env["packed"])
    _run(env, "fpca_create_from_bed", upload)


def test_debug_gather(env):
    from flashpca_amd.api import debug_gather

    rng = np.random.default_rng(5)
    nrec, v_rows, b = 70, 90, 16
    lens = rng.integers(0, 9, nrec)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    idx = rng.integers(0, v_rows, int(ptr[-1])).astype(np.uint32)
    V, rs = rng.standard_normal((v_rows, b)), rng.standard_normal(v_rows)
    _run(env, "fpca_debug_gather", lambda: (debug_gather(ptr, idx, V, b, rows_out=80, rowscale=rs, init=np.ones((80, b)))[0],))


def test_debug_i8_slices(env):
    from flashpca_amd.api import debug_i8_slices

    rng = np.random.default_rng(6)
    V, peers = rng.standard_normal((48, 16)), rng.uniform(0.0, 9.0, (2, 64))

    def both_routes():
        a, = debug_i8_slices(V, 16, 4, rows=45, route=0, rowscales=[np.full(45, 2.0)], peers=peers, copy=(32, None))
        b, = debug_i8_slices(V, 16, 4, rows=45, route=1, peers=peers, rows_valid=40, copy=(32, None), dequant=(32, 64))
        return a["Q"], a["colw"], a["colsum"], a["copy32"], b["Q"], b["Qrm"], b["colw"], b["colsum"], b["copy32"], b["dq32"], b["dq64"]

    _run(env, "fpca_debug_i8_slices", both_routes)


def test_bench_hooks(env):
    ctx, L = env["ctx"], env["L"]

    def apply():
        r = ctx.bench_apply(b=16, steps=1, warmup=0)
        return r["ms_total"] > 0, r["flops_per_step"], r["packed_bytes_per_step"]

    _run(env, "fpca_bench_apply", apply)

    def stats():
        ms, nbytes = ctx.bench_stats(2)
        return ms > 0, nbytes

    _run(env, "fpca_bench_stats", stats)

    def k4():
        g, m = C.c_double(0), C.c_double(0)
        env["fp"]._lib.check(L.fpca_debug_k4_bench(ctx.h, 16, 2, 2, C.byref(g), C.byref(m)))
        return g.value > 0, m.value > 0

    _run(env, "fpca_debug_k4_bench", k4)

    # the fused update + Gram kernel exists from 8,192 block rows on (kern::update_gram_planes): the 600-sample context is refused with
    # FPCA_EINVAL before anything is acquired, so this one call gets a context of its own, 7,700 samples (N_pad = 8,192) x 260 SNPs
    with env["fp"].Context.synthetic(7700, 260, n_pop=4, missing_rate=0.01, accum="fp64") as tall:
        assert tall.block_rows() == 8192

        def k4_fused():
            f = C.c_double(0)
            env["fp"]._lib.check(L.fpca_debug_k4_fused_bench(tall.h, 16, 2, 2, C.byref(f)))
            return (f.value > 0,)

        _run(dict(env, B=np.random.default_rng(12).standard_normal((7700, 16))), "fpca_debug_k4_fused_bench", k4_fused, ctx=tall)


def test_mfma_probes(env):
    L, check = env["L"], env["fp"]._lib.check
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((16, 4)), rng.standard_normal((4, 16))
    A8, B8 = rng.integers(-128, 128, (32, 32), dtype=np.int8), rng.integers(-128, 128, (32, 32), dtype=np.int8)

    def f64():
        D = np.zeros((16, 16))
        check(L.fpca_debug_mfma_probe(_p(A), _p(B), _p(D)))
        return (D,)

    def i8():
        D = np.zeros((32, 32), dtype=np.int32)
        check(L.fpca_debug_mfma_i8_probe(_p(A8), _p(B8), _p(D)))
        return (D,)

    assert np.array_equal(i8()[0], A8.astype(np.int32) @ B8.astype(np.int32).T)
    _run(env, "fpca_debug_mfma_probe", f64)
    _run(env, "fpca_debug_mfma_i8_probe", i8)
