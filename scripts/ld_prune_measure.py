"""LD pruning, the numbers of DESIGN 7f (profiles/ld_prune_figures.txt):

  python scripts/ld_prune_measure.py [OUT.json] [--parent-lib PATH] [--n N] [--p P] [--no-e2e]

at 500,000 x 100,000 synthetic of the realistic profile, on one MI355X:
  - the bitmap kernel alone (fpca_bench_ld: a pair of HIP events around each launch) at span 49, 199 and 999: ms, int8 MAC/s over the
    products actually issued (the hook replays the kernel's own x.x-only / six-product decisions), fraction of the int8 issue peak
    measured in the same session (fpca_debug_mfma_peak with random operands; the zero-operand rate is printed beside it) and, beside it, the K2 int8 GEMM of a 16-column apply on the same
    context (bench_apply's ms_gemm_xt) as the project's own yardstick;
  - fpca_ld_prune as a whole (1000, 50, 0.05), and its two halves from the test build's FPCA_LD_TIMING line: device part (totals, kernel,
    bitmap download) and host rule;
  - a 16-column apply of this build against the parent commit's library (--parent-lib), same process, alternating;
  - unless --no-e2e: flashpca(ld=) end to end against the same call without ld= on a fileset written under TMPDIR (--n / --p, default
    20,000 x 50,000: the wall of both calls is the .bed upload and the solve, the prune is the difference).
Every figure is the median of five with min and max beside it.
"""
import ctypes as C
import json
import os
import shutil
import statistics as st
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
import flashpca_amd as fp  # noqa: E402
from flashpca_amd import _lib  # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


N, P = 500_000, 100_000
parent = opt("--parent-lib", "")
out_path = args[0] if args and not args[0].startswith("--") else "ld_prune_measure.json"


def spread(ts):
    return dict(values=[round(float(t), 4) for t in ts], min=float(min(ts)), median=float(st.median(ts)), max=float(max(ts)))


out = dict(N=N, P=P)
os.environ["FPCA_LD_TIMING"] = "1"  # (read by the test build only)
with fp.test_hooks():
    t0 = time.time()
    ctx = fp.Context.synthetic(N, P, seed=20261017, n_pop=10, realistic=True, accum="auto")
    print("context %.1fs accum %s" % (time.time() - t0, ctx.accum), flush=True)
    tops, tops0 = C.c_double(0), C.c_double(0)
    _lib.check(fp.lib().fpca_debug_mfma_peak(2, 20000, 11, C.byref(tops)))
    _lib.check(fp.lib().fpca_debug_mfma_peak(2, 20000, 10, C.byref(tops0)))
    peak_macs = tops.value * 1e12 / 2.0
    out["int8_issue_peak_tops"] = dict(random_operands=tops.value, zero_operands=tops0.value)
    print("int8 MFMA issue peak, 2 waves/SIMD: %.0f TOP/s with random operands (the yardstick below), %.0f TOP/s with zero operands" % (
        tops.value, tops0.value), flush=True)

    # the project's own int8 GEMM on the same context: K2 of a 16-column apply
    ctx.bench_apply(b=16, steps=3, warmup=2)
    g = [ctx.bench_apply(b=16, steps=10, warmup=2) for _ in range(5)]
    out["apply_b16_ms"] = spread([r["ms_total"] / 10 for r in g])
    out["k2_gemm_ms"] = spread([r["ms_gemm_xt"] for r in g])
    print("apply b=16 %.3f ms; K2 GEMM launch alone %.3f ms" % (out["apply_b16_ms"]["median"], out["k2_gemm_ms"]["median"]), flush=True)

    for span in (49, 199, 999):
        ms, macs = ctx.bench_ld(span, reps=5)
        rate = macs / (st.median(ms) * 1e-3)
        out["kernel_span%d" % span] = dict(ms=spread(ms), macs=macs, mac_per_s=rate, fraction_of_issue_peak=rate / peak_macs)
        print("bitmap kernel span %d: %.2f ms (%.2f ... %.2f), %.3e int8 MACs issued, %.3e MAC/s = %.3f of the issue peak" % (
            span, st.median(ms), min(ms), max(ms), macs, rate, rate / peak_macs), flush=True)

    walls = []
    for _ in range(5):
        t = time.perf_counter()
        kept = ctx.ld_prune(1000, 50, 0.05)
        walls.append((time.perf_counter() - t) * 1e3)
    out["ld_prune_wall_ms"] = spread(walls)
    out["ld_prune_kept"] = int(kept.sum())
    print("fpca_ld_prune(1000, 50, 0.05): %.1f ms (%.1f ... %.1f), %d of %d kept (halves: the FPCA_LD_TIMING lines on stderr)" % (
        st.median(walls), min(walls), max(walls), kept.sum(), P), flush=True)

    if parent:
        Lp = C.CDLL(parent)
        for name in ("fpca_create_synthetic_model", "fpca_bench_apply", "fpca_destroy", "fpca_last_error"):
            res, argt = _lib.SIGNATURES[name]
            getattr(Lp, name).restype, getattr(Lp, name).argtypes = res, argt
        h = C.c_void_p()
        mdl = _lib.SynthModel(10, 0.05, 0.001, 1, 1, 0.05, 0.0)
        rc = Lp.fpca_create_synthetic_model(C.byref(h), N, 0, P, 20261017, C.byref(mdl), 3, 0, 0)
        assert rc == 0, Lp.fpca_last_error()

        def parent_apply(steps, warmup):
            r = _lib.BenchResult()
            assert Lp.fpca_bench_apply(h, 16, steps, warmup, C.byref(r)) == 0, Lp.fpca_last_error()
            return r.ms_total / steps

        parent_apply(3, 2)
        a, b = [], []
        for _ in range(5):
            a.append(ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"] / 10)
            b.append(parent_apply(10, 2))
        Lp.fpca_destroy(h)
        out["apply_b16_ms_ab"] = dict(this_build=spread(a), parent_build=spread(b), ratio=st.median(a) / st.median(b))
        print("apply b=16, alternating: this build %.3f ms, parent build %.3f ms (ratio %.4f)" % (st.median(a), st.median(b), st.median(a) / st.median(b)),
              flush=True)
    ctx.close()

if "--no-e2e" not in args:
    n, p = opt("--n", 20_000), opt("--p", 50_000)
    td = tempfile.mkdtemp(prefix="fpca_ld_")
    try:
        with fp.Context.synthetic(n, p, seed=7, n_pop=10, realistic=True, accum="fp64") as c:
            with open(os.path.join(td, "d.bed"), "wb") as f:
                f.write(bytes([0x6C, 0x1B, 0x01]))
                c.download_packed().tofile(f)
        with open(os.path.join(td, "d.fam"), "w") as f:
            f.writelines("f%d i%d 0 0 0 -9\n" % (i, i) for i in range(n))
        with open(os.path.join(td, "d.bim"), "w") as f:
            f.writelines("%d rs%d 0 %d A C\n" % (1 + j * 22 // p, j, j + 1) for j in range(p))
        prefix = os.path.join(td, "d")
        fp.flashpca(prefix, ndim=10)
        plain, pruned = [], []
        for _ in range(5):
            t = time.perf_counter()
            fp.flashpca(prefix, ndim=10)
            plain.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            r = fp.flashpca(prefix, ndim=10, ld=(1000, 50, 0.05))
            pruned.append((time.perf_counter() - t) * 1e3)
        out["flashpca_e2e"] = dict(N=n, P=p, kept=int(r["snps_kept"].sum()), without_ld_ms=spread(plain), with_ld_ms=spread(pruned))
        print("flashpca %d x %d end to end: without ld= %.0f ms, with ld=(1000, 50, 0.05) %.0f ms (%d kept)" % (
            n, p, st.median(plain), st.median(pruned), r["snps_kept"].sum()), flush=True)
    finally:
        shutil.rmtree(td, ignore_errors=True)
json.dump(out, open(out_path, "w"), indent=1)
