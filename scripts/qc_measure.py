"""The genotype census and the HWE kernel, the numbers of DESIGN 7h (profiles/qc_figures.txt):

  python scripts/qc_measure.py [OUT.json] [--parent-lib PATH] [--n N] [--p P]

on synthetic genotypes of the realistic profile, 500,000 SNPs x 100,000 samples unless --p / --n say otherwise, on one MI355X:
  - K1 (fpca_bench_stats) and the two count kernels (fpca_bench_qc) on the same context: ms per launch and the rate over the packed
    bytes, which are the same for all three, so K1 is the yardstick;
  - the HWE kernel on the all-sample counts: ms per launch, the recurrence steps of one launch (the hook replays the walk lengths on the
    host) and steps per second;
  - the filters end to end on the resident context, as qc_filter() runs them after its upload: sample_qc(0.02), then
    snp_qc_samples(survivors, maf 0.01, geno 0.02, hwe 1e-6), wall clock;
  - a 16-column apply of this build against the parent commit's library (--parent-lib), same process, alternating.
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


N, P = opt("--n", 100_000), opt("--p", 500_000)
parent = opt("--parent-lib", "")
out_path = args[0] if args and not args[0].startswith("--") else "qc_measure.json"


def spread(ts):
    return dict(values=[round(float(t), 4) for t in ts], min=float(min(ts)), median=float(st.median(ts)), max=float(max(ts)))


out = dict(N=N, P=P)
t0 = time.time()
with fp.Context.synthetic(N, P, seed=20261019, n_pop=10, realistic=True, accum="auto") as ctx:
    print("%d samples x %d SNPs: context %.1fs accum %s" % (N, P, time.time() - t0, ctx.accum), flush=True)
    k1, snp, smp, hwe = [], [], [], []
    nbytes = steps = 0.0
    for _ in range(5):
        ms, nbytes = ctx.bench_stats(reps=5)
        k1.append(ms)
        q, steps = ctx.bench_qc(reps=5)
        snp.append(q[0])
        smp.append(q[1])
        hwe.append(q[2])
    out.update(packed_bytes=nbytes, k1_ms=spread(k1), snp_counts_ms=spread(snp), sample_counts_ms=spread(smp), hwe_ms=spread(hwe), hwe_steps=steps)
    for name, ts in (("K1 (k_bed_stats)", k1), ("k_snp_counts", snp), ("k_sample_counts", smp)):
        m = st.median(ts)
        print("%-18s %.3f ms (%.3f ... %.3f), %.0f GB/s over the packed bytes, %.2f x K1" % (
            name, m, min(ts), max(ts), nbytes / m / 1e6, m / st.median(k1)), flush=True)
    m = st.median(hwe)
    print("k_hwe_exact        %.3f ms (%.3f ... %.3f), at most %.3e recurrence steps, %.3e steps/s" % (m, min(hwe), max(hwe), steps, steps / (m * 1e-3)),
          flush=True)
    walls = []
    for _ in range(5):
        t = time.perf_counter()
        samples = ctx.sample_qc(0.02)
        snps = ctx.snp_qc_samples(samples, maf=0.01, geno=0.02, hwe=1e-6)
        walls.append((time.perf_counter() - t) * 1e3)
    out.update(filters_wall_ms=spread(walls), samples_kept=int(samples.sum()), snps_kept=int(snps.sum()))
    print("sample_qc(0.02) + snp_qc_samples(maf 0.01, geno 0.02, hwe 1e-6): %.1f ms (%.1f ... %.1f); %d of %d samples, %d of %d SNPs" % (
        st.median(walls), min(walls), max(walls), samples.sum(), N, snps.sum(), P), flush=True)
    if parent:
        Lp = C.CDLL(parent)
        for name in ("fpca_create_synthetic_model", "fpca_bench_apply", "fpca_destroy", "fpca_last_error"):
            res, argt = _lib.SIGNATURES[name]
            getattr(Lp, name).restype, getattr(Lp, name).argtypes = res, argt
        h = C.c_void_p()
        mdl = _lib.SynthModel(10, 0.05, 0.001, 1, 1, 0.05, 0.0)
        rc = Lp.fpca_create_synthetic_model(C.byref(h), N, 0, P, 20261019, C.byref(mdl), 3, 0, 0)
        assert rc == 0, Lp.fpca_last_error()

        def parent_apply(nsteps, warmup):
            b = _lib.BenchResult()
            assert Lp.fpca_bench_apply(h, 16, nsteps, warmup, C.byref(b)) == 0, Lp.fpca_last_error()
            return b.ms_total / nsteps

        parent_apply(3, 2)
        ctx.bench_apply(b=16, steps=3, warmup=2)
        a, b = [], []
        for _ in range(5):
            a.append(ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"] / 10)
            b.append(parent_apply(10, 2))
        Lp.fpca_destroy(h)
        out["apply_b16_ms_ab"] = dict(this_build=spread(a), parent_build=spread(b), ratio=st.median(a) / st.median(b))
        print("apply b=16, alternating: this build %.3f ms, parent build %.3f ms (ratio %.4f)" % (st.median(a), st.median(b), st.median(a) / st.median(b)),
              flush=True)
json.dump(out, open(out_path, "w"), indent=1)
