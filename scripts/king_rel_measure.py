"""The KING relationship table, the numbers of DESIGN 7i (profiles/king_rel_figures.txt):

  python scripts/king_rel_measure.py [OUT.txt] [--n N] [--p P] [--reps R]

on one synthetic context of the realistic profile, 20,000 samples x 100,000 SNPs unless told otherwise, on one MI355X:
  - the pair kernel of fpca_king_related alone over the whole triangle (fpca_bench_king_rel) and the pair kernel of fpca_king_pairs
    (fpca_bench_king) on the SAME context: ms of each pass (a pair of HIP events around it) and the int8 MAC rate over the products
    actually issued (each hook replays its kernel's own fast-path decisions);
  - the ratio of the two times, next to 7/5 -- what the product count of the general path alone predicts.
Every figure is the median of the passes with min and max beside it.  The lines go to standard output and to OUT.txt (default
profiles/king_rel_figures.txt).
"""
import statistics as st
import sys
import time

sys.path.insert(0, ".")
import flashpca_amd as fp  # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    return type(default)(args[args.index(name) + 1]) if name in args else default


N, P, reps = opt("--n", 20_000), opt("--p", 100_000), opt("--reps", 5)
out_path = args[0] if args and not args[0].startswith("--") else "profiles/king_rel_figures.txt"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


t0 = time.time()
with fp.Context.synthetic(N, P, seed=20261019, n_pop=10, realistic=True, accum="auto") as ctx:
    say("%d x %d synthetic, realistic profile: context in %.1f s, accum %s" % (N, P, time.time() - t0, ctx.accum))
    res = {}
    for name, bench in (("k_king_rel (fpca_bench_king_rel)", ctx.bench_king_rel), ("k_king (fpca_bench_king)", ctx.bench_king)):
        ms, macs = bench(reps=reps)
        med = st.median(ms)
        res[name] = (med, macs)
        say("%-34s whole triangle: %.2f ms (%.2f ... %.2f over %d passes), %.4e int8 MACs issued, %.4e MAC/s" % (
            name, med, min(ms), max(ms), reps, macs, macs / (med * 1e-3)))
    (t_rel, m_rel), (t_old, m_old) = res.values()
    say("time ratio k_king_rel / k_king: %.3f; MACs issued ratio %.3f; 7/5 = 1.400 is what the product count of the general path predicts"
        % (t_rel / t_old, m_rel / m_old))
    say("registers by the compiler's remarks (tests/test_king_rel_cpu.py, tests/test_king_cpu.py): k_king_rel 171 / 182 VGPRs, occupancy 2 "
        "waves per SIMD; k_king 136 VGPRs, occupancy 3")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
