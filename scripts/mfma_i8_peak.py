import ctypes as C, sys
sys.path.insert(0, ".")
import flashpca_amd as fp
L = fp.lib()
for pat, nm in ((10, "zero operands"), (11, "random operands")):
    res = []
    for w in (1, 2, 4):
        t = C.c_double()
        rc = L.fpca_debug_mfma_peak(w, 20000, pat, C.byref(t))
        res.append("%d w/SIMD: %.0f TOP/s" % (w, t.value))
    print("v_mfma_i32_32x32x32_i8 (%s): %s" % (nm, ", ".join(res)), flush=True)

# which operand port pays for the bytes (source A / source B), and what the order of the two register sets costs: `reps` rounds over
# all patterns, interleaved, so that a drift of the box lands on every pattern alike
PORTS = ((12, "A random, B zero; equal sets"), (13, "A zero, B random; equal sets"),
         (14, "A geno, B random; A alternates, B holds 2"), (15, "A random, B geno; A alternates, B holds 2"),
         (16, "A geno, B random; A holds 2, B alternates"), (17, "A geno, B random; B holds 2 (= 14)"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
runs = {(p, w): [] for p, _ in PORTS for w in (1, 2)}
for _ in range(reps):
    for pat, _nm in PORTS:
        for w in (1, 2):
            t = C.c_double()
            fp._lib.check(L.fpca_debug_mfma_peak(w, 20000, pat, C.byref(t)))
            runs[pat, w].append(t.value)
for pat, nm in PORTS:
    for w in (1, 2):
        v = runs[pat, w]
        print("pattern %d (%s), %d w/SIMD: %s  min %.0f max %.0f TOP/s" % (pat, nm, w, " ".join("%.0f" % x for x in v), min(v), max(v)), flush=True)
