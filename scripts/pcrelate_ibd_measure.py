"""PC-Relate IBD sharing, the numbers of DESIGN 7l (profiles/pcrelate_ibd_figures.txt):

  python scripts/pcrelate_ibd_measure.py [OUT.txt] [--n N] [--p P] [--npc K] [--reps R]

at 20,000 x 100,000 synthetic genotypes of the realistic profile (fp64 mode, DESIGN 7k's context), npc = 4 (the context's own first four
PCs), on one MI355X, with the test build of the library:
  - the three instances of k_pcr_ibd alone over the whole lower triangle (fpca_bench_pcrelate_ibd: a pair of HIP events around each pass):
    ms, FLOP/s over the matrix instructions issued, seven products counted, and that rate as a fraction of the FP64 MFMA issue peak of the
    same session (fpca_debug_mfma_peak, pattern 1, 2 waves per SIMD: the occupancy of every instance);
  - k_pcr_gram on the same context in the same session (fpca_bench_pcrelate) and the ratio of the two rates;
  - k_pcr_ibd_operands alone, every launch of the triangle (the same hook under FPCA_PCR_BENCH_OPERANDS=1), and its share of the kernels;
  - fpca_pcrelate_ibd_tri as a whole with beta and f given (the sample-major copy, the upload of beta, every slab, the download of
    N (N + 1) / 2 entries of k2, k0 and nsnp).
Every figure is the median of --reps (5) after one untimed pass, with min and max beside it.
"""
import ctypes as C
import os
import statistics as st
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import flashpca_amd as fp  # noqa: E402
from flashpca_amd import _lib  # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


N, P, npc, reps = opt("--n", 20_000), opt("--p", 100_000), opt("--npc", 4), opt("--reps", 5)
out_path = args[0] if args and not args[0].startswith("--") else "profiles/pcrelate_ibd_figures.txt"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def med(ts):
    return "%.2f (%.2f ... %.2f)" % (st.median(ts), min(ts), max(ts))


def walls(call, n):
    call()  # one untimed pass
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        out = call()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts, out


with fp.test_hooks():
    t = C.c_double(0)
    _lib.check(fp.lib().fpca_debug_mfma_peak(2, 10000, 1, C.byref(t)))
    peak = t.value
    say("FP64 MFMA issue peak (fpca_debug_mfma_peak, pattern 1): %.1f TFLOP/s at 2 waves/SIMD" % peak)
    with fp.Context.synthetic(N, P, seed=20261020, n_pop=10, realistic=True, accum="fp64") as ctx:
        pcs = np.ascontiguousarray(ctx.pca(ndim=npc)["Px"][:, :npc])
        say("%d x %d synthetic, realistic profile, fp64 mode; pcs: the context's first %d PCs" % (N, P, npc))
        ms, flops = ctx.bench_pcrelate_ibd(npc=npc, reps=reps)
        rate = flops / (st.median(ms) * 1e-3) / 1e12
        say("k_pcr_ibd, three instances, whole triangle (fpca_bench_pcrelate_ibd): %s ms, %.4e flops issued (seven products), %.2f TFLOP/s = "
            "%.3f of the peak" % (med(ms), flops, rate, rate / peak))
        gms, gflops = ctx.bench_pcrelate(npc=npc, reps=reps)
        grate = gflops / (st.median(gms) * 1e-3) / 1e12
        say("k_pcr_gram on the same context (fpca_bench_pcrelate): %s ms, %.2f TFLOP/s = %.3f of the peak; k_pcr_ibd runs at %.3f of its rate"
            % (med(gms), grate, grate / peak, rate / grate))
        os.environ["FPCA_PCR_BENCH_OPERANDS"] = "1"
        oms, _ = ctx.bench_pcrelate_ibd(npc=npc, reps=reps)
        del os.environ["FPCA_PCR_BENCH_OPERANDS"]
        say("k_pcr_ibd_operands, every launch of the triangle: %s ms = %.3f of the kernels' time" % (med(oms), st.median(oms) / (st.median(oms) + st.median(ms))))
        beta = ctx.pcrelate_beta(pcs)
        f = np.zeros(N)
        tt, r = walls(lambda: ctx.pcrelate_ibd_tri(pcs, f=f, beta=beta), min(reps, 3))
        say("fpca_pcrelate_ibd_tri (beta and f given; 3 x %d entries downloaded): %s ms; k0 mean %.4f, k2 mean %.2e, %d NaN, nsnp "
            "%d ... %d" % (r["k2"].size, med(tt), np.nanmean(r["k0"]), np.nanmean(r["k2"]), int(np.isnan(r["k2"]).sum() + np.isnan(r["k0"]).sum()),
                           int(r["nsnp"].min()), int(r["nsnp"].max())))
