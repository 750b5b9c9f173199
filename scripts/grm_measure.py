"""The relationship matrix, the numbers of DESIGN 7j (profiles/grm_figures.txt):

  python scripts/grm_measure.py [OUT.txt] [--n N] [--p P] [--reps R]

at 20,000 x 100,000 synthetic genotypes of the realistic profile (fp64 mode), on one MI355X, with the test build of the library:
  - the FP64 Gram kernel alone over the whole lower triangle (fpca_bench_grm: a pair of HIP events around each pass): ms, FLOP/s over the
    matrix instructions issued, and that rate as a fraction of the FP64 MFMA issue peak of the same session (fpca_debug_mfma_peak,
    pattern 1) at 2 and at 4 waves per SIMD -- launch_bounds(256, 2) and the occupancy the compiler's remarks state;
  - the K2 GEMM launch of a 64-column apply on the same context (fpca_bench_apply, ms_gemm_xt) and its fraction of the same peak: the
    project's own FP64-MFMA kernel as the yardstick;
  - the shared-call count kernel alone (the same hook under FPCA_GRM_BENCH_SHARED=1) and its share of the two kernels' time;
  - fpca_grm_cutoff(0.025) as a whole (the sample-major copy, totals, both kernels slab by slab, the list, the host rule) and
    fpca_grm_tri (with its download of N (N + 1) / 2 doubles and counts).
Every figure is the median of --reps (5) with min and max beside it.
"""
import ctypes as C
import os
import statistics as st
import sys
import time

sys.path.insert(0, ".")
import flashpca_amd as fp  # noqa: E402
from flashpca_amd import _lib  # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


N, P, reps = opt("--n", 20_000), opt("--p", 100_000), opt("--reps", 5)
out_path = args[0] if args and not args[0].startswith("--") else "profiles/grm_figures.txt"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def med(ts):
    return "%.2f (%.2f ... %.2f)" % (st.median(ts), min(ts), max(ts))


def peak(waves):
    t = C.c_double(0)
    _lib.check(fp.lib().fpca_debug_mfma_peak(waves, 10000, 1, C.byref(t)))
    return t.value


with fp.test_hooks():
    peaks = {w: peak(w) for w in (2, 4)}
    say("FP64 MFMA issue peak (fpca_debug_mfma_peak, pattern 1): %.1f TFLOP/s at 2 waves/SIMD, %.1f at 4" % (peaks[2], peaks[4]))
    t0 = time.time()
    with fp.Context.synthetic(N, P, seed=20261020, n_pop=10, realistic=True, accum="fp64") as ctx:
        say("%d x %d synthetic, realistic profile, fp64 mode: context in %.1f s" % (N, P, time.time() - t0))
        ms, flops = ctx.bench_grm(reps=reps)
        rate = flops / (st.median(ms) * 1e-3) / 1e12
        say("k_grm_dot, whole triangle (fpca_bench_grm): %s ms, %.4e flops issued, %.2f TFLOP/s = %.3f of the peak at 2 waves/SIMD, %.3f at 4"
            % (med(ms), flops, rate, rate / peaks[2], rate / peaks[4]))
        g = [ctx.bench_apply(b=64, steps=10, warmup=2) for _ in range(reps)]
        k2 = [r["ms_gemm_xt"] for r in g]
        n_pad, p_pad = (N + 511) // 512 * 512, (P + 255) // 256 * 256
        k2rate = 2.0 * n_pad * p_pad * 64 / (st.median(k2) * 1e-3) / 1e12
        say("K2 GEMM launch of a 64-column apply on the same context: %s ms, %.2f TFLOP/s = %.3f of the peak at 2 waves/SIMD; k_grm_dot runs at "
            "%.3f of K2's rate" % (med(k2), k2rate, k2rate / peaks[2], rate / k2rate))
        os.environ["FPCA_GRM_BENCH_SHARED"] = "1"
        cms, _ = ctx.bench_grm(reps=reps)
        del os.environ["FPCA_GRM_BENCH_SHARED"]
        say("k_grm_shared, whole triangle: %s ms = %.3f of the two kernels' time" % (med(cms), st.median(cms) / (st.median(cms) + st.median(ms))))
        walls = []
        for _ in range(reps):
            t = time.perf_counter()
            kept = ctx.grm_cutoff(0.025)
            walls.append((time.perf_counter() - t) * 1e3)
        say("fpca_grm_cutoff(0.025, shared): %s ms, %d of %d kept" % (med(walls), kept.sum(), N))
        walls = []
        for _ in range(min(reps, 3)):
            t = time.perf_counter()
            tri, cnt = ctx.grm_tri(counts=True)
            walls.append((time.perf_counter() - t) * 1e3)
        dg = tri[[i * (i + 3) // 2 for i in range(N)]]
        say("fpca_grm_tri (shared, with counts; %d entries downloaded): %s ms; diagonal mean %.4f" % (tri.size, med(walls), dg.mean()))
