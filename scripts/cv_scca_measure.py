"""Cross-validated SCCA, the numbers of DESIGN 7c (profiles/cv_scca_measure.json):

  python scripts/cv_scca_measure.py measure [OUT.json]   whole-call walls of fpca_scca_cv at 500,000 x 100,000 (realistic profile, k = 10,
                                                          10 folds, 5 x 5 grid, ndim 3, tol 1e-6) with the library's own split into phases
                                                          (FPCA_TIMING: a device synchronise closes every phase), then at 50,000 x 20,000 the
                                                          new call alternating with the public route it replaces: per fold a context on the
                                                          re-packed training rows + scca_prepare + the scca_fit grid + a projection context
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cv -- python scripts/cv_scca_measure.py profile
                                                          k_fold_counts (10 folds) and k_bed_stats on the same context, three launches each
  python scripts/cv_scca_measure.py summary DIR [OUT.json]  launch times of the two kernels from that trace, bytes/s of the packed stream
"""
import csv, glob, json, os, re, statistics as st, sys, tempfile, time

import numpy as np

sys.path.insert(0, ".")

N, P, k = 500_000, 100_000, 10


def summary():
    rows = []
    for f in glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = {}
    nbytes = ((N + 3) // 4 + 127) // 128 * 128 * P
    for name in ("k_fold_counts", "k_bed_stats"):
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if name in r["Kernel_Name"])
        if d:
            out[name] = dict(launches=len(d), ms=d, median_ms=st.median(d), packed_bytes=nbytes, tb_per_s=nbytes / (st.median(d) * 1e-3) / 1e12)
    print(json.dumps(out))
    json.dump(out, open(sys.argv[3] if len(sys.argv) > 3 else "cv_scca_kernels.json", "w"), indent=1)


if len(sys.argv) > 1 and sys.argv[1] == "summary":
    summary()
    sys.exit(0)

import flashpca_amd as fp  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "measure"
rng = np.random.default_rng(1)


class stderr_to_file:
    """The library reports its phases on the C stderr: redirect the descriptor for the length of one call."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def phenos(ctx, k, ncausal=2000):
    B = np.zeros((ctx.P, k), order="F")
    B[rng.choice(ctx.P, ncausal, replace=False)] = rng.standard_normal((ncausal, k))
    XB = ctx.apply_x(B)
    return XB / XB.std(axis=0) + 3 * rng.standard_normal((ctx.N, k))


def spread(ts):
    return dict(wall_s=ts, min_s=min(ts), median_s=st.median(ts), max_s=max(ts))


t0 = time.time()
ctx = fp.Context.synthetic(N, P, seed=20261016, realistic=True, accum="auto")
print("context %.1fs accum %s" % (time.time() - t0, ctx.accum), flush=True)
folds = rng.integers(0, 10, N)
if mode == "profile":
    for _ in range(3):
        ctx.fold_stats(folds, 10, 0)
        ctx.bench_stats(reps=1)
    sys.exit(0)

out = {}
Y = phenos(ctx, k)
l1s, l2s = [2e-3, 3e-3, 4e-3, 6e-3, 8e-3], [1e-4, 3e-4, 1e-3, 3e-3, 1e-2]
V0 = rng.standard_normal((10, k, 3))
call = lambda: ctx.scca_cv(Y, folds, l1s, l2s, 3, V0, standy="sd", tol=1e-6)  # noqa: E731
r = call()  # warm-up (allocations of the operator's workspaces, the sample-major copy)
ts = []
for _ in range(3):
    t = time.time(); r = call(); ts.append(time.time() - t)
out["headline"] = dict(N=N, P=P, k=k, nfolds=10, grid=[5, 5], ndim=3, tol=1e-6, lambda1=l1s, lambda2=l2s, **spread(ts), total_iterations=int(r["iters"].sum() + r["warm_iters"].sum()),
                       converged_models=int(r["converged"].sum()), corr_dim1=r["corr"][0].tolist(), best=[r["best_lambda1"], r["best_lambda2"], r["best_corr"]],
                       missing_mode=ctx.missing_mode(16))
print(json.dumps(out["headline"]), flush=True)
os.environ["FPCA_TIMING"] = "1"
with stderr_to_file() as cap:
    t = time.time(); call(); tw = time.time() - t
del os.environ["FPCA_TIMING"]
m = re.search(r"scca_cv: fold counts ([\d.]+) ms, per-fold setup ([\d.]+) ms, K2 ([\d.]+) ms, fits ([\d.]+) ms \((\d+) iterations\), K3 \+ gather ([\d.]+) ms, correlation ([\d.]+) ms", cap.text)
out["headline_phases_ms"] = dict(zip(("fold_counts", "per_fold_setup", "k2", "fits", "iterations", "k3_gather", "correlation"), map(float, m.groups())), wall_s_with_phase_syncs=tw)
out["headline_phases_ms"]["us_per_iteration_in_fits"] = 1e3 * out["headline_phases_ms"]["fits"] / max(1.0, out["headline_phases_ms"]["iterations"])
print(json.dumps(out["headline_phases_ms"]), flush=True)
ms1, by = ctx.bench_stats(reps=5)
out["k_bed_stats_event_ms"] = ms1
ctx.close()

# ---- the comparator: the public route of the parent commit, at a size where re-packing on the host is still reasonable
Nc, Pc, nf = 50_000, 20_000, 4
l1c, l2c = [4e-3, 8e-3, 1.6e-2], [1e-3, 3e-3, 1e-2]
with fp.Context.synthetic(Nc, Pc, seed=20261016, realistic=True, accum="auto") as ctx:
    Yc = phenos(ctx, k, ncausal=500)
    fc = rng.integers(0, nf, Nc)
    V0c = rng.standard_normal((nf, k, 3))
    packed = ctx.download_packed().reshape(Pc, -1)
    t = time.time()
    codes = np.stack([(packed >> (2 * s)) & 3 for s in range(4)], axis=-1).reshape(Pc, -1)[:, :Nc]

    def pack(c):
        n = c.shape[1]
        z = np.zeros((Pc, (n + 3) // 4 * 4), dtype=np.uint8)
        z[:, :n] = c
        return np.ascontiguousarray(z[:, 0::4] | (z[:, 1::4] << 2) | (z[:, 2::4] << 4) | (z[:, 3::4] << 6))

    parts = [(pack(codes[:, fc != f]), pack(codes[:, fc == f])) for f in range(nf)]
    out["comparator_repack_host_s"] = time.time() - t
    del codes

    def new_route():
        return ctx.scca_cv(Yc, fc, l1c, l2c, 3, V0c, standy="sd", tol=1e-6, return_pred=True)

    def public_route():
        xp = np.zeros((Nc, 3, 3, 3))
        for f in range(nf):
            w = fc != f
            with fp.Context.from_packed(parts[f][0], int(w.sum()), Pc, accum="auto") as ct, fp.Context.from_packed(parts[f][1], int((~w).sum()), Pc, accum="auto") as ch:
                ch.set_meansd(ct.stats()[0])
                ct.scca_prepare(Yc[w], standy="sd")
                Vw = ct.scca_fit(1e-12, 1e-12, 3, V0c[f], tol=1e-6)["V"]
                for i, a in enumerate(l1c):
                    for j, b in enumerate(l2c):
                        mdl = ct.scca_fit(a, b, 3, Vw, tol=1e-6)
                        xp[~w, :, i, j] = ch.apply_x(mdl["U"]) if mdl["converged"] else np.nan
        return xp

    rn, xo = new_route(), public_route()  # warm-up of both
    fin = np.isfinite(xo) & np.isfinite(rn["xpred"])
    out["comparator_max_rel_dxpred"] = float(np.abs(xo - rn["xpred"])[fin].max() / np.abs(xo[fin]).max())
    tn, to = [], []
    for _ in range(3):
        t = time.time(); new_route(); tn.append(time.time() - t)
        t = time.time(); public_route(); to.append(time.time() - t)
    out["comparator"] = dict(N=Nc, P=Pc, k=k, nfolds=nf, grid=[3, 3], ndim=3, new_call=spread(tn), public_route=spread(to), converged_models=int(rn["converged"].sum()),
                             total_iterations=int(rn["iters"].sum() + rn["warm_iters"].sum()))
print(json.dumps(out["comparator"]), flush=True)
json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else "cv_scca_measure.json", "w"), indent=1)
