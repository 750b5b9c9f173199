"""Sample subsets, the numbers of DESIGN 7d (profiles/subset_measure.json, profiles/subset_kernels.json):

  python scripts/subset_measure.py measure [OUT.json]    at 500,000 x 100,000 on the realistic profile, 80 % of the samples kept:
                                                         bench_apply(b = 16) with the mask set against without, same process,
                                                         alternating (the difference is the row-mask pass); the wall of a masked
                                                         fpca_pca (k = 20, tol 1e-6) against the unmasked solve on the same context,
                                                         with the pass counts; the wall of fpca_set_sample_mask itself
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o subset -- python scripts/subset_measure.py profile
                                                         k_bed_stats_masked and k_bed_stats on the same context, five launches each,
                                                         and five masked applies (k_mask_rows); no counters in that run
  python scripts/subset_measure.py summary DIR [OUT.json]  launch times of the kernels from that trace, bytes/s of the packed stream
"""
import csv, glob, json, statistics as st, sys, time

import numpy as np

sys.path.insert(0, ".")

N, P, k = 500_000, 100_000, 20


def summary():
    rows = []
    for f in glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = {}
    nbytes = ((N + 3) // 4 + 127) // 128 * 128 * P
    for name in ("k_bed_stats_masked", "k_bed_stats", "k_mask_rows"):
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows
                   if name in r["Kernel_Name"] and (name != "k_bed_stats" or "masked" not in r["Kernel_Name"]))
        if d:
            out[name] = dict(launches=len(d), ms=d, median_ms=st.median(d))
            if name != "k_mask_rows":
                out[name].update(packed_bytes=nbytes, tb_per_s=nbytes / (st.median(d) * 1e-3) / 1e12)
    if "k_bed_stats_masked" in out and "k_bed_stats" in out:
        out["ratio_masked_over_k1"] = out["k_bed_stats_masked"]["median_ms"] / out["k_bed_stats"]["median_ms"]
    print(json.dumps(out))
    json.dump(out, open(sys.argv[3] if len(sys.argv) > 3 else "subset_kernels.json", "w"), indent=1)


if len(sys.argv) > 1 and sys.argv[1] == "summary":
    summary()
    sys.exit(0)

import flashpca_amd as fp  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "measure"
rng = np.random.default_rng(1)


def spread(ts):
    return dict(values=ts, min=min(ts), median=st.median(ts), max=max(ts))


t0 = time.time()
ctx = fp.Context.synthetic(N, P, seed=20261017, n_pop=10, realistic=True, accum="auto")
print("context %.1fs accum %s" % (time.time() - t0, ctx.accum), flush=True)
keep = rng.random(N) < 0.8
if mode == "profile":
    for _ in range(5):
        ctx.set_sample_mask(keep)   # k_bed_stats_masked
        ctx.bench_apply(b=16, steps=1, warmup=0)
        ctx.set_sample_mask(None)
        ctx.bench_stats(reps=1)     # k_bed_stats
    ctx.set_sample_mask(keep)
    B = rng.standard_normal((N, 16))
    for _ in range(5):
        ctx.apply_xxt(B)            # k_mask_rows twice per apply (operand and result)
    sys.exit(0)

out = dict(N=N, P=P, kept=int(keep.sum()))
ctx.bench_apply(b=16, steps=3, warmup=2)  # (allocations, the sample-major copy, the route)
out["missing_mode"] = ctx.missing_mode(16)
ts = []
for _ in range(5):
    t = time.time(); ctx.set_sample_mask(keep); ts.append(time.time() - t)
    ctx.set_sample_mask(None)
    ctx.stats()
out["set_sample_mask_wall_s"] = spread(ts)
# the operator itself (apply_xxt_dev as bench_apply times it) does not depend on the mask; the masked entry points add the row-mask pass.
# Timed here through Context.apply_xxt_dev on device blocks: wall clock around 20 applies between two synchronisations.
import ctypes as C  # noqa: E402

hip = C.CDLL("libamdhip64.so")  # (the runtime the library is linked against)
rows, b = ctx.block_rows(), 16
Bh = np.zeros((rows, b))
Bh[:N] = rng.random((N, b)) - 0.5
dB, dY = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(dB), C.c_size_t(Bh.nbytes)) == 0 and hip.hipMalloc(C.byref(dY), C.c_size_t(Bh.nbytes)) == 0
assert hip.hipMemcpy(dB, Bh.ctypes.data_as(C.c_void_p), C.c_size_t(Bh.nbytes), 1) == 0


def timed_applies(n=20):
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        ctx.apply_xxt_dev(dB.value, b, dY.value)
    ctx.synchronize()
    return (time.perf_counter() - t) / n * 1e3


plain, masked, plain_hook, masked_hook = [], [], [], []
for _ in range(4):
    ctx.set_sample_mask(None)
    timed_applies(3)
    plain.append(timed_applies())
    plain_hook.append(ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"])
    ctx.set_sample_mask(keep)
    timed_applies(3)
    masked.append(timed_applies())
    masked_hook.append(ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"])  # (K2 + K3 alone: the kernels under the subset's statistics)
out["apply_b16_ms"] = dict(no_mask=spread(plain), mask_set=spread(masked), no_mask_bench_apply=spread(plain_hook), mask_set_bench_apply=spread(masked_hook),
                           difference_us=(st.median(masked) - st.median(plain)) * 1e3)
print(json.dumps(out["apply_b16_ms"]), flush=True)
# fpca_pca, k = 20, tol 1e-6: unmasked against masked (80 % kept) on the same context, alternating
walls = dict(no_mask=[], mask_set=[])
info = {}
for rep in range(3):
    for name, m in (("no_mask", None), ("mask_set", keep)):
        ctx.set_sample_mask(m)
        ctx.stats()
        t = time.time(); r = ctx.pca(ndim=k, tol=1e-6); walls[name].append(time.time() - t)
        info[name] = dict(block_applies=r["info"]["block_applies"], cheap_applies=r["info"]["cheap_applies"], seconds_total=r["info"]["seconds_total"],
                          seconds_apply=r["info"]["seconds_apply"], seconds_ortho=r["info"]["seconds_ortho"], seconds_post=r["info"]["seconds_post"],
                          seconds_download=r["info"]["seconds_download"], d1=float(r["d"][0]), d20=float(r["d"][-1]))
out["pca_k20"] = dict(walls_s={a: spread(v) for a, v in walls.items()}, info=info)
print(json.dumps(out["pca_k20"]), flush=True)
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "subset_measure.json", "w"), indent=1)
