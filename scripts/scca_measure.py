"""SCCA at 500,000 x 100,000 (realistic profile), the numbers of DESIGN 7b (profiles/r07_scca_*):

  python scripts/scca_measure.py measure [OUT.json]   walls: fpca_ucca next to fpca_scca_prepare, one literal iteration
                                                       (bench_apply, 16 columns), the warm start, a lambda1 scan, one fit
                                                       (k = 10, ndim = 5, tol 1e-6), a 5 x 5 grid, k = 256
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o scca -- python scripts/scca_measure.py profile LAMBDA1
                                                       the launches of a warm start + one fit at k = 10, then one fit at k = 256
  python scripts/scca_measure.py summary DIR [OUT.txt] per-kernel launch statistics of that trace, the two phases apart, and the
                                                       time of one iteration (first kernel's start to last kernel's end)
"""
import csv, glob, json, statistics as st, sys, time

import numpy as np

sys.path.insert(0, ".")


def summary():
    rows = []
    for f in glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    ev = []
    for r in rows:
        n = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), n))
    ev.sort()
    stores = [s for s, e, n in ev if n == "k_scca_store_c"]
    split = stores[1] if len(stores) > 1 else 1 << 62
    with open(sys.argv[3] if len(sys.argv) > 3 else "scca_profile_summary.txt", "w") as o:
        for label, sel in (("k = 10 (warm start + one fit, ndim 5)", [x for x in ev if x[0] < split]), ("k = 256 (one fit, ndim 2)", [x for x in ev if x[0] >= split])):
            by = {}
            for s, e, n in sel:
                if n.startswith("k_scca"):
                    by.setdefault(n, []).append((e - s) / 1e3)
            o.write("== %s\nkernel  launches  total_ms  mean_us  median_us  p10_us  p90_us\n" % label)
            for n, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
                d.sort()
                o.write("%s  %d  %.3f  %.2f  %.2f  %.2f  %.2f\n" % (n, len(d), sum(d) / 1e3, sum(d) / len(d), st.median(d), d[len(d) // 10], d[9 * (len(d) - 1) // 10]))
            # (launches enqueued after a dimension has converged return at once: they pull the means and the p10 down, not the medians)
            it = [(s, e) for s, e, n in sel if n == "k_scca_cv"]
            v_end = [e for s, e, n in sel if n == "k_scca_v"]
            if len(it) > 2 and len(v_end) == len(it):
                per = sorted((ve - s) / 1e3 for (s, e), ve in zip(it, v_end))
                gaps = sorted((b[0] - a[0]) / 1e3 for a, b in zip(it, it[1:]))
                o.write("one iteration, first kernel's start to last kernel's end (us): median %.2f p10 %.2f p90 %.2f\n" % (st.median(per), per[len(per) // 10], per[9 * len(per) // 10]))
                o.write("period between consecutive iterations' starts (us): median %.2f p10 %.2f p90 %.2f n %d\n" % (st.median(gaps), gaps[len(gaps) // 10], gaps[9 * len(gaps) // 10], len(gaps)))


if len(sys.argv) > 1 and sys.argv[1] == "summary":
    summary()
    sys.exit(0)

import flashpca_amd as fp  # noqa: E402


N, P, k = 500_000, 100_000, 10
mode = sys.argv[1] if len(sys.argv) > 1 else "measure"
out = {}
rng = np.random.default_rng(1)
t0 = time.time()
ctx = fp.Context.synthetic(N, P, seed=20261016, realistic=True, accum="auto")
print("context %.1fs accum %s" % (time.time() - t0, ctx.accum), flush=True)

def phenos(k, ncausal=2000):
    B = np.zeros((P, k), order="F")
    B[rng.choice(P, ncausal, replace=False)] = rng.standard_normal((ncausal, k))
    XB = ctx.apply_x(B)
    return XB / XB.std(axis=0) + 3 * rng.standard_normal((N, k))

def wall(f, reps=3):
    ts = []
    for _ in range(reps):
        t = time.time(); r = f(); ts.append(time.time() - t)
    return ts, r

Y = phenos(k)
V0 = rng.standard_normal((k, 5))
if mode == "profile":
    ctx.scca_prepare(Y)
    Vw = ctx.scca_fit(1e-9, 1e-9, 5, V0, tol=1e-6)["V"]
    r = ctx.scca_fit(float(sys.argv[2]), 1e-3, 5, Vw, tol=1e-6)
    print("profile fit k=10 iters", r["iters"].tolist(), "nzero_x", r["nzero_x"].tolist(), flush=True)
    Y2 = phenos(256)
    ctx.scca_prepare(Y2)
    r = ctx.scca_fit(float(sys.argv[2]), 1e-3, 2, rng.standard_normal((256, 2)), tol=1e-6)
    print("profile fit k=256 iters", r["iters"].tolist(), "nzero_x", r["nzero_x"].tolist(), flush=True)
    sys.exit(0)

ctx.ucca(Y); ctx.scca_prepare(Y)  # warm-up
out["ucca_wall_s"], _ = wall(lambda: ctx.ucca(Y))
out["prepare_wall_s"], _ = wall(lambda: ctx.scca_prepare(Y))
print(json.dumps(out), flush=True)
out["bench_apply_b16"] = ctx.bench_apply(b=16, steps=10, warmup=2)
print(json.dumps(out["bench_apply_b16"]), flush=True)
t = time.time(); w = ctx.scca_fit(1e-9, 1e-9, 5, V0, tol=1e-6); out["warm_start"] = dict(wall_s=time.time() - t, iters=w["iters"].tolist(), converged=w["converged"])
print(json.dumps(out["warm_start"]), flush=True)
Vw = w["V"]
scan = {}
for l1 in (2e-3, 4e-3, 6e-3, 8e-3, 1.2e-2):
    t = time.time(); r = ctx.scca_fit(l1, 1e-3, 1, Vw[:, :1], tol=1e-6)
    scan[l1] = dict(nzero_x=int(r["nzero_x"][0]), iters=int(r["iters"][0]), wall_s=time.time() - t, status=r["status"])
    print("scan", l1, scan[l1], flush=True)
out["lambda1_scan_ndim1"] = scan
ok = [l for l in scan if scan[l]["status"] == "ok" and scan[l]["nzero_x"] > 0]
l1 = min(ok, key=lambda l: abs(np.log(scan[l]["nzero_x"] / 3000.0)))
out["lambda1"] = l1
ts, r = wall(lambda: ctx.scca_fit(l1, 1e-3, 5, Vw, tol=1e-6))
out["fit_one"] = dict(wall_s=ts, iters=r["iters"].tolist(), nzero_x=r["nzero_x"].tolist(), nzero_y=r["nzero_y"].tolist(), converged=r["converged"], d=r["d"].tolist(),
                      ms_per_iteration_wall=1e3 * min(ts) / max(1, int(r["iters"].sum()) + 5))
print(json.dumps(out["fit_one"]), flush=True)
l1s = [l1 * f for f in (0.5, 0.75, 1.0, 1.25, 1.5)]
l2s = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2]
t = time.time()
grid = [[ctx.scca_fit(a, b, 5, Vw, tol=1e-6) for b in l2s] for a in l1s]
out["grid_5x5"] = dict(wall_s=time.time() - t, lambda1=l1s, lambda2=l2s, iters=[[g["iters"].tolist() for g in row] for row in grid],
                       status=[[g["status"] for g in row] for row in grid], nzero_x0=[[int(g["nzero_x"][0]) for g in row] for row in grid])
print("grid wall", out["grid_5x5"]["wall_s"], flush=True)
Y2 = phenos(256)
t = time.time(); ctx.scca_prepare(Y2); tp = time.time() - t
V2 = rng.standard_normal((256, 2))
ts, r = wall(lambda: ctx.scca_fit(l1, 1e-3, 2, V2, tol=1e-6), reps=2)
out["k256"] = dict(prepare_wall_s=tp, fit_wall_s=ts, iters=r["iters"].tolist(), nzero_x=r["nzero_x"].tolist(), status=r["status"],
                   ms_per_iteration_wall=1e3 * min(ts) / max(1, int(r["iters"].sum()) + 2))
print(json.dumps(out["k256"]), flush=True)
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "scca_measure.json", "w"), indent=1)
