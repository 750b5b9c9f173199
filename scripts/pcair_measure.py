"""PC-AiR's census pass, the numbers of DESIGN 7m (profiles/pcair_figures.txt):

  python scripts/pcair_measure.py [OUT.txt] [--n N] [--p P] [--reps R] [--rounds K]

on one synthetic context of 10 populations, 20,000 samples x 100,000 SNPs unless told otherwise, on one MI355X:
  - the census kernel alone over the whole triangle (fpca_bench_king_census) and the pair kernel of fpca_king_pairs (fpca_bench_king),
    INTERLEAVED on the same context, K rounds of R passes each (a pair of HIP events around every pass): the median of each with its own
    min and max, and the ratio of the medians.  Both kernels issue the same products, so the pair pass is the yardstick and its own spread
    is the resolution of the comparison;
  - the whole fpca_pcair_king call (operand, fused pass, downloads, the rule on the host), wall clock;
  - a 16-column apply before and after, to show the hot path is untouched.
The lines go to standard output and, as they come, to OUT.txt (default profiles/pcair_figures.txt).
"""
import statistics as st
import sys
import time

sys.path.insert(0, ".")
import flashpca_amd as fp  # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


N, P, reps, rounds = opt("--n", 20_000), opt("--p", 100_000), opt("--reps", 5), opt("--rounds", 3)
out_path = args[0] if args and not args[0].startswith("--") else "profiles/pcair_figures.txt"
open(out_path, "w").close()


def say(s):
    print(s, flush=True)
    with open(out_path, "a") as f:
        f.write(s + "\n")


def apply_ms(ctx):
    ctx.bench_apply(b=16, steps=3, warmup=2)
    return [ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"] / 10 for _ in range(5)]


t0 = time.time()
with fp.Context.synthetic(N, P, seed=20261021, n_pop=10, accum="auto") as ctx:
    say("%d x %d synthetic, n_pop = 10: context in %.1f s, accum %s" % (N, P, time.time() - t0, ctx.accum))
    before = apply_ms(ctx)
    say("16-column apply before: %.3f ms (%.3f ... %.3f over 5 x 10 steps)" % (st.median(before), min(before), max(before)))
    census, pairs, macs = [], [], 0.0
    for _ in range(rounds):
        census += list(ctx.bench_king_census(reps=reps))
        ms, macs = ctx.bench_king(reps=reps)
        pairs += list(ms)
    mc, mp = st.median(census), st.median(pairs)
    say("k_king_census (fpca_bench_king_census) whole triangle: %.2f ms (%.2f ... %.2f over %d passes), %.4e MAC/s over %.4e int8 MACs" % (
        mc, min(census), max(census), len(census), macs / (mc * 1e-3), macs))
    say("k_king<PAIRS> (fpca_bench_king)        whole triangle: %.2f ms (%.2f ... %.2f over %d passes), %.4e MAC/s" % (
        mp, min(pairs), max(pairs), len(pairs), macs / (mp * 1e-3)))
    say("time ratio census / pairs: %.4f; the pair pass's own spread (max - min) / median: %.4f, the census pass's: %.4f" % (
        mc / mp, (max(pairs) - min(pairs)) / mp, (max(census) - min(census)) / mc))
    t = time.time()
    try:
        mask, n_rel, n_div = ctx.pcair_partition(counts=True)
        say("fpca_pcair_king whole call at +-2^-5.5: %.2f s; %d related and %d divergent pairs; %d of %d samples kept" % (
            time.time() - t, int(n_rel.sum()) // 2, int(n_div.sum()) // 2, int(mask.sum()), N))
    except fp.FpcaError as e:  # (more related pairs than the call keeps room for: the message names the count)
        say("fpca_pcair_king whole call at +-2^-5.5: refused after %.2f s: %s" % (time.time() - t, e))
        n_rel, n_div = ctx.king_census()
        say("fpca_king_census at +-2^-5.5: %d related and %d divergent pairs" % (int(n_rel.sum()) // 2, int(n_div.sum()) // 2))
    after = apply_ms(ctx)
    say("16-column apply after:  %.3f ms (%.3f ... %.3f over 5 x 10 steps)" % (st.median(after), min(after), max(after)))
    say("registers by the compiler's remarks (tests/test_pcair_cpu.py, tests/test_king_cpu.py): k_king_census 136 VGPRs, occupancy 3 waves "
        "per SIMD; k_king 136 VGPRs, occupancy 3")
