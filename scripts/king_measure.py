"""KING-robust kinship, the numbers of DESIGN 7g (profiles/king_figures.txt):

  python scripts/king_measure.py [OUT.json] [--parent-lib PATH] [--sizes 20000,100000] [--p P] [--big]

on synthetic genotypes of the realistic profile with P = 100,000 SNPs, on one MI355X, for each sample count of --sizes:
  - the pair kernel alone over the whole triangle (fpca_bench_king: a pair of HIP events around each pass): ms, int8 MAC/s over the
    products actually issued (the hook replays the kernel's own x.x-only / five-product decisions), and that rate as a fraction of
      * the int8 issue peak of the same session (fpca_debug_mfma_peak, random operands) at 2 waves per SIMD -- launch_bounds(256, 2) -- and
        at the occupancy the compiler's remarks state for k_king (3);
      * the band kernel's rate (fpca_bench_ld at span 999) on the same context: the same inner loop, so the yardstick;
  - fpca_king_cutoff(0.0884) as a whole (the sample-major copy, totals, the kernel, the host rule);
  - at the first size, a 16-column apply of this build against the parent commit's library (--parent-lib), same process, alternating.
--big: one pass at 500,000 samples, only when the last size's figure extrapolates (quadratically) below 120 s.
Every figure is the median of five with min and max beside it.
"""
import ctypes as C
import json
import statistics as st
import sys
import time

sys.path.insert(0, ".")
import flashpca_amd as fp  # noqa: E402
from flashpca_amd import _lib  # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


sizes = [int(s) for s in opt("--sizes", "20000,100000").split(",")]
P = opt("--p", 100_000)
parent = opt("--parent-lib", "")
out_path = args[0] if args and not args[0].startswith("--") else "king_measure.json"


def spread(ts):
    return dict(values=[round(float(t), 4) for t in ts], min=float(min(ts)), median=float(st.median(ts)), max=float(max(ts)))


def peak(waves):
    tops = C.c_double(0)
    _lib.check(fp.lib().fpca_debug_mfma_peak(waves, 20000, 11, C.byref(tops)))
    return tops.value


out = dict(P=P, sizes=sizes)
peaks = {w: peak(w) for w in (2, 3)}
out["int8_issue_peak_tops"] = peaks
print("int8 MFMA issue peak, random operands: %.0f TOP/s at 2 waves/SIMD, %.0f at 3" % (peaks[2], peaks[3]), flush=True)


def measure(N, reps=5, ab=False):
    r = dict(N=N)
    t0 = time.time()
    with fp.Context.synthetic(N, P, seed=20261019, n_pop=10, realistic=True, accum="auto") as ctx:
        print("%d x %d: context %.1fs accum %s" % (N, P, time.time() - t0, ctx.accum), flush=True)
        ms, macs = ctx.bench_king(reps=reps)
        rate = macs / (st.median(ms) * 1e-3)
        r["kernel"] = dict(ms=spread(ms), macs=macs, mac_per_s=rate, fraction_of_peak_2_waves=rate / (peaks[2] * 1e12 / 2),
                           fraction_of_peak_3_waves=rate / (peaks[3] * 1e12 / 2))
        print("%d x %d pair kernel, whole triangle: %.2f ms (%.2f ... %.2f), %.3e int8 MACs issued, %.3e MAC/s = %.3f of the issue peak at 2 "
              "waves/SIMD, %.3f at 3" % (N, P, st.median(ms), min(ms), max(ms), macs, rate, r["kernel"]["fraction_of_peak_2_waves"],
                                        r["kernel"]["fraction_of_peak_3_waves"]), flush=True)
        if reps > 1:
            lms, lmacs = ctx.bench_ld(999, reps=reps)
            lrate = lmacs / (st.median(lms) * 1e-3)
            r["ld_span999"] = dict(ms=spread(lms), macs=lmacs, mac_per_s=lrate)
            r["kernel"]["fraction_of_ld_rate"] = rate / lrate
            print("%d x %d band kernel span 999 on the same context: %.2f ms, %.3e MAC/s; the pair kernel runs at %.3f of that rate" % (
                N, P, st.median(lms), lrate, rate / lrate), flush=True)
            walls = []
            for _ in range(reps):
                t = time.perf_counter()
                kept = ctx.king_cutoff(0.0884)
                walls.append((time.perf_counter() - t) * 1e3)
            r["king_cutoff_wall_ms"] = spread(walls)
            r["king_cutoff_kept"] = int(kept.sum())
            print("%d x %d fpca_king_cutoff(0.0884): %.1f ms (%.1f ... %.1f), %d of %d kept" % (
                N, P, st.median(walls), min(walls), max(walls), kept.sum(), N), flush=True)
        if ab and parent:
            Lp = C.CDLL(parent)
            for name in ("fpca_create_synthetic_model", "fpca_bench_apply", "fpca_destroy", "fpca_last_error"):
                res, argt = _lib.SIGNATURES[name]
                getattr(Lp, name).restype, getattr(Lp, name).argtypes = res, argt
            h = C.c_void_p()
            mdl = _lib.SynthModel(10, 0.05, 0.001, 1, 1, 0.05, 0.0)
            rc = Lp.fpca_create_synthetic_model(C.byref(h), N, 0, P, 20261019, C.byref(mdl), 3, 0, 0)
            assert rc == 0, Lp.fpca_last_error()

            def parent_apply(steps, warmup):
                b = _lib.BenchResult()
                assert Lp.fpca_bench_apply(h, 16, steps, warmup, C.byref(b)) == 0, Lp.fpca_last_error()
                return b.ms_total / steps

            parent_apply(3, 2)
            ctx.bench_apply(b=16, steps=3, warmup=2)
            a, b = [], []
            for _ in range(5):
                a.append(ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"] / 10)
                b.append(parent_apply(10, 2))
            Lp.fpca_destroy(h)
            r["apply_b16_ms_ab"] = dict(this_build=spread(a), parent_build=spread(b), ratio=st.median(a) / st.median(b))
            print("%d x %d apply b=16, alternating: this build %.3f ms, parent build %.3f ms (ratio %.4f)" % (
                N, P, st.median(a), st.median(b), st.median(a) / st.median(b)), flush=True)
    return r


out["runs"] = []
for k, N in enumerate(sizes):
    out["runs"].append(measure(N, ab=(k == 0)))
    json.dump(out, open(out_path, "w"), indent=1)
if "--big" in args:
    last = out["runs"][-1]
    guess = last["kernel"]["ms"]["median"] * (500_000 / last["N"]) ** 2 / 1e3
    print("500,000 samples, extrapolated from %d: %.0f s" % (last["N"], guess), flush=True)
    out["big_extrapolated_s"] = guess
    if guess < 120:
        out["runs"].append(measure(500_000, reps=1))
    else:
        print("not run: over 120 s", flush=True)
json.dump(out, open(out_path, "w"), indent=1)
