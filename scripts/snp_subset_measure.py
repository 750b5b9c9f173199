"""SNP subsets, the numbers of DESIGN 7e (profiles/snp_subset_figures.txt):

  python scripts/snp_subset_measure.py [OUT.json] [--parent-lib PATH] [--no-bed]

at 500,000 x 100,000 synthetic, for three masks (90 % random, 50 % random, the first 90 % contiguous):
  - the record gather alone (fpca_debug_snp_subset_bench: HIP events around `reps` launches, the destination allocated before), next to
    K1's pass on the same context (fpca_bench_stats); achieved bandwidth of both (the gather moves 2 pitch P_kept bytes, K1 reads
    ceil(N / 4) P);
  - the wall of fpca_create_snp_subset as a whole (allocation, 0x55 memset, index upload, gather, synchronise);
  - the route a user has without the feature: fpca_create_from_bed of a subset fileset (11.3 GB written under TMPDIR through the feature itself, read
    back warm), for the 90 % random mask;
  - bench_apply(b = 16) on the unfiltered context and on the 90 % subset, and -- with --parent-lib, the parent commit's libfpca.so --
    the unfiltered apply of both builds in the same process, alternating.
Every figure is the median of five (the spread is kept beside it).
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

N, P = 500_000, 100_000
args = sys.argv[1:]
parent = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
no_bed = "--no-bed" in args
out_path = args[0] if args and not args[0].startswith("--") else "snp_subset_measure.json"


def spread(ts):
    return dict(values=[round(t, 4) for t in ts], min=min(ts), median=st.median(ts), max=max(ts))


rng = np.random.default_rng(20261018)
masks = {"random90": rng.random(P) < 0.9, "random50": rng.random(P) < 0.5, "first90": np.arange(P) < int(0.9 * P)}
t0 = time.time()
ctx = fp.Context.synthetic(N, P, seed=20261017, n_pop=10, realistic=True, accum="auto")
print("context %.1fs accum %s" % (time.time() - t0, ctx.accum), flush=True)
pitch = ((N + 3) // 4 + 127) // 128 * 128
out = dict(N=N, P=P, pitch=pitch)

# K1 on the same context
ctx.bench_stats(reps=2)
k1 = [ctx.bench_stats(reps=5) for _ in range(5)]
k1_ms, k1_bytes = st.median(m for m, _ in k1), k1[0][1]
out["k1"] = dict(ms=spread([m for m, _ in k1]), bytes=k1_bytes, tb_per_s=k1_bytes / (k1_ms * 1e-3) / 1e12)
print("K1: %.3f ms, %.2f TB/s" % (k1_ms, out["k1"]["tb_per_s"]), flush=True)

for name, m in masks.items():
    kept = int(m.sum())
    ctx.snp_subset_bench(m, reps=1)
    g = [ctx.snp_subset_bench(m, reps=5) for _ in range(5)]
    ms, nbytes = st.median(t for t, _ in g), g[0][1]
    assert nbytes == 2.0 * pitch * kept
    walls = []
    for _ in range(5):
        t = time.perf_counter()
        sub = ctx.snp_subset(m)
        walls.append((time.perf_counter() - t) * 1e3)
        sub.close()
    out[name] = dict(kept=kept, gather_ms=spread([t for t, _ in g]), bytes_moved=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                     fraction_of_k1_bandwidth=nbytes / ms / (k1_bytes / k1_ms), create_snp_subset_wall_ms=spread(walls))
    print("%s: %d SNPs, gather %.3f ms = %.2f TB/s (%.2f of K1's), fpca_create_snp_subset %.1f ms" % (
        name, kept, ms, out[name]["tb_per_s"], out[name]["fraction_of_k1_bandwidth"], st.median(walls)), flush=True)

# the operator: unfiltered, and on the 90 % subset
ctx.bench_apply(b=16, steps=3, warmup=2)
full = [ctx.bench_apply(b=16, steps=10, warmup=2)["ms_total"] / 10 for _ in range(5)]
out["apply_b16_ms_unfiltered"] = spread(full)
with ctx.snp_subset(masks["random90"]) as sub:
    sub.bench_apply(b=16, steps=3, warmup=2)
    out["apply_b16_ms_random90_subset"] = spread([sub.bench_apply(b=16, steps=10, warmup=2)["ms_total"] / 10 for _ in range(5)])
    out["missing_mode"] = dict(unfiltered=ctx.missing_mode(16), random90_subset=sub.missing_mode(16))
print("apply b=16: unfiltered %.3f ms, 90 %% subset %.3f ms" % (st.median(full), out["apply_b16_ms_random90_subset"]["median"]), flush=True)

# today's route: a second fileset of the subset, uploaded from the page cache
if not no_bed:
    td = tempfile.mkdtemp(prefix="fpca_snpsub_")  # (TMPDIR; needs room for the subset fileset, 11.3 GB)
    try:
        m = masks["random90"]
        idx = np.flatnonzero(m)
        t = time.perf_counter()
        with open(os.path.join(td, "sub.bed"), "wb") as f:
            f.write(bytes([0x6C, 0x1B, 0x01]))
            step = max(1, (1 << 30) // ((N + 3) // 4))
            for j0 in range(0, idx.size, step):
                with ctx.snp_subset(idx[j0:j0 + step], accum="fp64") as c:
                    c.download_packed().tofile(f)
        t_write = time.perf_counter() - t
        walls = []
        for _ in range(4):
            t = time.perf_counter()
            c = fp.Context.from_bed(os.path.join(td, "sub.bed"), N, accum="auto")
            walls.append((time.perf_counter() - t) * 1e3)
            c.close()
        out["from_bed_of_subset_fileset"] = dict(bed_bytes=os.path.getsize(os.path.join(td, "sub.bed")), write_s=t_write, first_ms=walls[0],
                                                  warm_ms=spread(walls[1:]))
        print("fpca_create_from_bed of the subset fileset: first %.0f ms, warm %.0f ms (fileset written in %.1f s)" % (
            walls[0], st.median(walls[1:]), t_write), flush=True)
    finally:
        shutil.rmtree(td, ignore_errors=True)

# the unfiltered apply of this build against the parent commit's, same process, alternating
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
    print("unfiltered apply b=16, alternating: this build %.3f ms, parent build %.3f ms (ratio %.4f)" % (st.median(a), st.median(b), st.median(a) / st.median(b)),
          flush=True)
ctx.close()
json.dump(out, open(out_path, "w"), indent=1)
