"""python scripts/summarise_gather_trace.py <rocprofv3 output dir> <label>: the last 10 applies of a traced bench.py run (rocprofv3
--kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --steps 12 --warmup 1) -- K2 / K3 GEMM durations, the gather of
each stage relative to its GEMM, apply period; grids in threads.  The trace lines of profiles/gather_resident_ab.txt."""
import csv, glob, statistics as st, sys

d, label = sys.argv[1], sys.argv[2]
gemm, gath = [], []
for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        grid = r.get("Grid_Size", r.get("Grid_Size_X", ""))
        if "k_gemm_i8" in n:
            gemm.append((s, e, n[n.find("I8Cfg"):].split(">")[0] + ">", grid))
        elif "k_sparse_rows_sum" in n:
            gath.append((s, e, n[n.find("k_sparse"):].split("(")[0], grid))
gemm.sort()
gath.sort()
# the big launches only (the two GEMMs of an apply have the largest grids of the run)
if not gemm:
    sys.exit("%s: no k_gemm_i8 launch in the trace" % label)
big = max(int(g[3]) for g in gemm)
gemm = [g for g in gemm if int(g[3]) * 2 > big]
gemm = gemm[len(gemm) % 2:]  # K2, K3, K2, K3 ...: an even count, ending with a K3
last = gemm[-20:]
med = st.median
for stage, off in (("K2", 0), ("K3", 1)):
    gs = last[off::2]
    dur = [(e - s) / 1e6 for s, e, _, _ in gs]
    line = "  trace %-22s %s %s grid %s n=%d median %.3f min %.3f max %.3f ms" % (label, stage, gs[0][2], gs[0][3], len(gs), med(dur), min(dur), max(dur))
    rel = []
    for s, e, _, _ in gs:
        near = [g for g in gath if abs(g[0] - s) < 0.5e6]
        if near:
            g = min(near, key=lambda g: abs(g[0] - s))
            rel.append(((g[0] - s) / 1e6, (g[1] - s) / 1e6, (e - g[1]) / 1e6, (g[1] - g[0]) / 1e6, g[2], g[3]))
    if rel:
        line += " | gather %s grid %s: starts %+.3f, ends %+.3f after the GEMM's start = %.3f before its end (min %.3f); own duration %.3f ms" % (
            rel[0][4], rel[0][5], med([r[0] for r in rel]), med([r[1] for r in rel]), med([r[2] for r in rel]), min(r[2] for r in rel), med([r[3] for r in rel]))
    print(line)
k2 = [g[0] for g in last[0::2]]
if len(k2) > 1:
    print("  trace %-22s apply period (K2 GEMM start to start, last %d applies) %.3f ms" % (label, len(k2), med([(b - a) / 1e6 for a, b in zip(k2, k2[1:])])))
