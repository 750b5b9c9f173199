"""numpy-level mirror of the C ABI (include/fpca.h) -- used by the tests, bench.py and smoke().

`Context` is one SNP shard of a genotype matrix resident on one MI355X.  `flashpca()` mirrors the reference's
scripting entry point (the R function flashpca(), flashpcaR/R/flashpca.R:99-204: same argument names and the same
result fields values / vectors / projection / loadings / center / scale / pve) because no R toolchain exists here;
the compiled drop-in is the `flashpca` CLI built from flashpca_amd/csrc/cli_main.cpp.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DIVISOR, STANDARDISE, BenchResult, FpcaError, PcaInfo, PcaOpts, check, lib  # noqa: F401


ACCUM = {"auto": 0, 0: 0, "fp64": 64, "fp32": 32, 64: 64, 32: 32, "i8": 807}
ACCUM.update({"i8x%d" % s: 800 + s for s in range(2, 9)})
ACCUM.update({800 + s: 800 + s for s in range(2, 9)})


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def count_fam_rows(path):
    """N = number of newline-terminated lines of the .fam (the reference drops an unterminated last line,
    data.cpp:526)."""
    with open(path, "rb") as f:
        return f.read().count(b"\n")


def _snp_mask(snps, P):
    """A boolean mask over P SNPs from a boolean mask or an array of unique, in-range indices."""
    a = np.asarray(snps)
    if a.dtype == np.bool_:
        if a.shape != (P,):
            raise ValueError("a SNP mask must have one entry per SNP (%d), it has shape %s" % (P, a.shape))
        return a.copy()
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("SNPs are selected by a boolean mask or by a one-dimensional array of integer indices")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= P):
        raise ValueError("SNP indices must be in 0 .. %d" % (P - 1))
    if np.unique(a).size != a.size:
        raise ValueError("SNP indices must be unique")
    mask = np.zeros(P, dtype=bool)
    mask[a] = True
    return mask


def _pair_indices(pairs, name):
    """(i, j) as two contiguous uint32 arrays of one length from a pair of index arrays (None: two empty ones); the library checks them
    against N."""
    if pairs is None:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)
    try:
        i, j = pairs
    except (TypeError, ValueError):
        raise ValueError("%s is (i, j): two arrays of sample indices" % name)
    out = []
    for a in (i, j):
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("%s holds one-dimensional arrays of integer sample indices" % name)
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError("%s holds sample indices between 0 and 2^32 - 1" % name)
        out.append(np.ascontiguousarray(a, dtype=np.uint32))
    if out[0].shape != out[1].shape:
        raise ValueError("%s: i and j have one entry per pair; they have shapes %s and %s" % (name, out[0].shape, out[1].shape))
    return out[0], out[1]


def _kin_pairs(kin_pairs):
    """(i, j, kin) of PC-AiR's outside relatives as contiguous uint32 / uint32 / float64 arrays of one length."""
    try:
        i, j, kin = kin_pairs
    except (TypeError, ValueError):
        raise ValueError("kin_pairs is (i, j, kin): two arrays of sample indices and the kinship of each pair")
    i, j = _pair_indices((i, j), "kin_pairs")
    kin = np.ascontiguousarray(kin, dtype=np.float64)
    if kin.shape != i.shape:
        raise ValueError("kin_pairs: kin has one entry per pair (%d), it has shape %s" % (i.size, kin.shape))
    return i, j, kin


def _synth_model(n_pop, fst, missing_rate, realistic, maf_model, missing_model, conc_frac, lognormal_sigma):
    return _lib.SynthModel(n_pop, fst, missing_rate, int(realistic if maf_model is None else maf_model),
                           int(realistic if missing_model is None else missing_model), conc_frac, lognormal_sigma)


def debug_synth_host(N, P, snp_begin=0, seed=20260928, n_pop=40, fst=0.05, missing_rate=0.001, realistic=False, maf_model=None,
                     missing_model=None, conc_frac=0.05, lognormal_sigma=0.0):
    """fpca_debug_synth_host: records [snp_begin, snp_begin + P) of the matrix Context.synthetic(N, ...) generates with the same
    arguments, computed on the host (no device involved).  Returns (packed, fixed): a uint8 array of shape (P, (N + 3) // 4) and the
    five integers the model was reduced to, as a dict (fst_fp, miss_thr, conc_fp, med_q32, sig2_fp)."""
    m = _synth_model(n_pop, fst, missing_rate, realistic, maf_model, missing_model, conc_frac, lognormal_sigma)
    out = np.empty((int(P), (int(N) + 3) // 4), dtype=np.uint8)
    fixed = (C.c_uint64 * 5)()
    check(lib().fpca_debug_synth_host(N, snp_begin, P, seed, C.byref(m), _p(out), fixed))
    return out, dict(zip(("fst_fp", "miss_thr", "conc_fp", "med_q32", "sig2_fp"), (int(v) for v in fixed)))


class Context:
    def __init__(self, handle, accum="auto"):
        self.h = handle
        self._accum_req = accum  # the arithmetic the context was asked for (snp_subset passes it on)
        L = lib()
        self.N = int(L.fpca_nsamples(handle))
        self.P = int(L.fpca_nsnps(handle))
        self.P_total = self.P
        self._keep = []

    def missing_mode(self, b=32):
        """How the exact-integer path treats the missing-call indicator (fpca_missing_mode): 0 full, 1 skip empty blocks,
        2 nothing missing, 3 sparse gathers, 4 hybrid (sparse gathers + a dense sub-matrix for the SNPs that hold most of the
        missing calls); -1 for the fp64 / fp32 kernels."""
        return int(lib().fpca_missing_mode(self.h, b))

    def debug_pass_slices(self, Sc):
        """fpca_debug_set_pass_slices (test-hook build): the next apply_xt / apply_x / apply_xxt run on Sc slices inside this context, as
        the eigensolver's cheap passes do; 0: exact passes again.  pca() clears the setting."""
        check(lib().fpca_debug_set_pass_slices(self.h, int(Sc)))

    def allreduce_chunks(self):
        """Row chunks of Y whose all-reduce overlaps the computation of the next chunk (fpca_allreduce_chunks)."""
        return int(lib().fpca_allreduce_chunks(self.h))

    @property
    def accum(self):
        """The arithmetic mode in effect: 'fp64', 'fp32' or 'i8xS' ("auto" resolved)."""
        code = int(lib().fpca_accum(self.h))
        return {64: "fp64", 32: "fp32"}.get(code, "i8x%d" % (code - 800))

    # ---- constructors -----------------------------------------------------------------------------
    @classmethod
    def from_packed(cls, packed, N, P, stand="binom2", device=0, accum="fp64"):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        assert packed.size >= ((N + 3) // 4) * P
        h = C.c_void_p()
        check(lib().fpca_create(C.byref(h), _p(packed), N, P, STANDARDISE[stand], device, ACCUM[accum]))
        return cls(h, accum)

    @classmethod
    def from_bed(cls, bed_path, N, snp_begin=0, P=0, stand="binom2", device=0, accum="fp64"):
        h = C.c_void_p()
        ptot = C.c_uint64(0)
        check(lib().fpca_create_from_bed(C.byref(h), bed_path.encode(), N, snp_begin, P, STANDARDISE[stand], device, ACCUM[accum],
                                         C.byref(ptot)))
        c = cls(h, accum)
        c.P_total = int(ptot.value)
        check(lib().fpca_set_total_snps(h, c.P_total))
        return c

    @classmethod
    def from_dense(cls, X, stand="binom2", device=0):
        """In-memory N x P fp64 matrix (NaN = missing), standardised on the GPU like standardise() (util.cpp:24-192)."""
        X = np.asfortranarray(X, dtype=np.float64)
        h = C.c_void_p()
        check(lib().fpca_create_dense(C.byref(h), _p(X), X.shape[0], X.shape[0], X.shape[1], _lib.STANDARDISE_DENSE[stand], device))
        return cls(h)

    @classmethod
    def synthetic(cls, N, P, snp_begin=0, seed=20260928, n_pop=40, fst=0.05, missing_rate=0.001, stand="binom2", device=0,
                  accum="fp64", realistic=False, maf_model=None, missing_model=None, conc_frac=0.05, lognormal_sigma=0.0):
        """realistic=True: the round-4 profile (synth.hpp) -- rare-variant allele-frequency spectrum, missing calls concentrated in
        5 % of the SNPs (maf_model / missing_model = 1; either can be chosen alone).  missing_model=2: per-SNP rates log-normally
        distributed with log-sd lognormal_sigma; missing_rate is the NOMINAL mean -- the realised mean of the per-SNP thresholds is
        0.87-1.00 of it (the tail is cut), see profiles/synth_model_figures.txt."""
        h = C.c_void_p()
        m = _synth_model(n_pop, fst, missing_rate, realistic, maf_model, missing_model, conc_frac, lognormal_sigma)
        check(lib().fpca_create_synthetic_model(C.byref(h), N, snp_begin, P, seed, C.byref(m), STANDARDISE[stand], device, ACCUM[accum]))
        return cls(h, accum)

    def close(self):
        if self.h:
            lib().fpca_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data / statistics --------------------------------------------------------------------------
    def download_packed(self):
        out = np.empty(((self.N + 3) // 4) * self.P, dtype=np.uint8)
        check(lib().fpca_download_packed(self.h, _p(out)))
        return out

    def stats(self):
        ms = np.empty((self.P, 2), order="F")
        tr = C.c_double(0)
        check(lib().fpca_stats(self.h, _p(ms), C.byref(tr)))
        return ms, tr.value

    def set_meansd(self, meansd):
        m = np.asfortranarray(meansd, dtype=np.float64)
        check(lib().fpca_set_meansd(self.h, _p(m)))

    def set_sample_mask(self, keep):
        """fpca_set_sample_mask: keep is a boolean array with one entry per sample (True = kept), or None to clear the mask.  While a
        mask is set, stats() / pca() are those of the kept samples, apply_xt / apply_xxt treat the held-out rows as zero and apply_x
        computes every row; pca() returns U with zero held-out rows and Px with the held-out samples projected onto the PCs."""
        if keep is None:
            check(lib().fpca_set_sample_mask(self.h, None))
            return
        keep = np.asarray(keep)
        if keep.shape != (self.N,):
            raise ValueError("keep must have one entry per sample (%d), it has shape %s" % (self.N, keep.shape))
        k8 = np.ascontiguousarray(keep != 0, dtype=np.uint8)
        check(lib().fpca_set_sample_mask(self.h, _p(k8)))

    @property
    def nkept(self):
        """Samples the statistics and pca() run on (fpca_nkept): the kept ones under a mask, else N."""
        return int(lib().fpca_nkept(self.h))

    # ---- SNP subsets ---------------------------------------------------------------------------------
    def snp_missing(self):
        """fpca_snp_missing: K1's per-SNP counts of missing calls over all N samples, a uint32 array."""
        out = np.empty(self.P, dtype=np.uint32)
        check(lib().fpca_snp_missing(self.h, _p(out)))
        return out

    def snp_qc(self, maf=0.0, geno=1.0, keep=None):
        """fpca_snp_qc: the boolean mask of the SNPs with minor-allele frequency >= maf and missing-call rate <= geno (PLINK's --maf /
        --geno; maf <= 0 and geno >= 1 switch a filter off), among those of `keep` (a mask or an index array; None: all)."""
        k8 = np.ascontiguousarray(np.ones(self.P, dtype=bool) if keep is None else _snp_mask(keep, self.P), dtype=np.uint8)
        n = C.c_uint64(0)
        check(lib().fpca_snp_qc(self.h, float(maf), float(geno), _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def snp_subset(self, keep, accum=None):
        """fpca_create_snp_subset: a new Context holding the SNPs of `keep` (a boolean mask, or unique in-range indices, which are applied
        in ascending order), compacted on the device.  accum: the new context's arithmetic (None: what this one was asked for).  This
        context stays as it is; both matrices are resident until it is closed."""
        k8 = np.ascontiguousarray(_snp_mask(keep, self.P), dtype=np.uint8)
        accum = self._accum_req if accum is None else accum
        h = C.c_void_p()
        check(lib().fpca_create_snp_subset(C.byref(h), self.h, _p(k8), ACCUM[accum]))
        return Context(h, accum)

    def snp_subset_bench(self, keep, reps=5):
        """fpca_debug_snp_subset_bench: (milliseconds per launch, bytes moved per launch) of the record gather alone."""
        k8 = np.ascontiguousarray(_snp_mask(keep, self.P), dtype=np.uint8)
        ms, by = C.c_double(0), C.c_double(0)
        check(lib().fpca_debug_snp_subset_bench(self.h, _p(k8), int(reps), C.byref(ms), C.byref(by)))
        return ms.value, by.value

    # ---- LD pruning --------------------------------------------------------------------------------
    def ld_band(self, snp0, nsnp, span):
        """fpca_ld_band: the nsnp x span array of pairwise-complete r2 between SNP snp0 + i and SNP snp0 + i + d (column d - 1); NaN past
        the end of the range, where a pair shares no call, and where a SNP is constant on the shared calls."""
        snp0, nsnp, span = int(snp0), int(nsnp), int(span)
        if snp0 < 0 or nsnp < 0 or not 0 <= span < 2 ** 32:
            raise ValueError("snp0, nsnp and span are non-negative (span below 2^32)")
        out = np.empty((max(nsnp, 1), max(span, 1)), dtype=np.float64)  # (a zero-sized request still reaches the library's refusal)
        check(lib().fpca_ld_band(self.h, snp0, nsnp, span, _p(out)))
        return out[:nsnp, :span]

    def ld_prune(self, window=1000, step=50, r2=0.05, chrom=None, keep=None):
        """fpca_ld_prune: the boolean mask of the SNPs a PLINK-1.9-style --indep-pairwise window step r2 keeps (windows and steps in
        SNPs), among those of `keep` (a mask or an index array; None: all).  chrom: one integer code per SNP, a chromosome being a
        maximal run of equal codes (None: one chromosome)."""
        window, step = int(window), int(step)
        if not (0 <= window < 2 ** 32 and 0 <= step < 2 ** 32):
            raise ValueError("window and step are SNP counts in 0 .. 2^32 - 1")
        k8 = np.ascontiguousarray(np.ones(self.P, dtype=bool) if keep is None else _snp_mask(keep, self.P), dtype=np.uint8)
        c32 = None
        if chrom is not None:
            c32 = np.ascontiguousarray(chrom, dtype=np.uint32)
            if c32.shape != (self.P,):
                raise ValueError("chrom must have one entry per SNP (%d), it has shape %s" % (self.P, c32.shape))
        n = C.c_uint64(0)
        check(lib().fpca_ld_prune(self.h, _p(c32), window, step, float(r2), _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def bench_ld(self, span, reps=5):
        """fpca_bench_ld: (milliseconds of each of `reps` launches of the bitmap kernel over all SNPs, int8 MACs one launch issues)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        macs = C.c_double(0)
        check(lib().fpca_bench_ld(self.h, int(span), int(reps), _p(ms), C.byref(macs)))
        return ms, macs.value

    # ---- kinship ------------------------------------------------------------------------------------
    def _sample_keep(self, keep):
        if keep is None:
            return None
        keep = np.asarray(keep)
        if keep.shape != (self.N,):
            raise ValueError("keep must have one entry per sample (%d), it has shape %s" % (self.N, keep.shape))
        return np.ascontiguousarray(keep != 0, dtype=np.uint8)

    def king_block(self, i0, ni, j0, nj):
        """fpca_king_block: the ni x nj array of KING-robust kinship between sample i0 + a and sample j0 + b, any rectangle (at i == j the
        formula gives 0.5, or NaN for a sample without a heterozygous call); NaN where the pair shares no heterozygous call of the less
        heterozygous sample."""
        i0, ni, j0, nj = int(i0), int(ni), int(j0), int(nj)
        if min(i0, ni, j0, nj) < 0:
            raise ValueError("i0, ni, j0 and nj are non-negative")
        out = np.empty((max(ni, 1), max(nj, 1)), dtype=np.float64)  # (a zero-sized request still reaches the library's refusal)
        check(lib().fpca_king_block(self.h, i0, ni, j0, nj, _p(out)))
        return out[:ni, :nj]

    def king_pairs(self, thr, keep=None, max_pairs=1 << 24):
        """fpca_king_pairs: (i, j, phi) of every pair of samples i < j with kinship phi > thr, sorted by (i, j), among the samples of `keep`
        (a boolean array with one entry per sample; None: all).  FpcaError (code -4, the message names the count) when more than max_pairs
        qualify."""
        k8 = self._sample_keep(keep)
        max_pairs = int(max_pairs)
        if max_pairs < 0:
            raise ValueError("max_pairs is non-negative")
        room = max(min(max_pairs, self.N * (self.N - 1) // 2), 1)
        i = np.empty(room, dtype=np.uint32)
        j = np.empty(room, dtype=np.uint32)
        phi = np.empty(room, dtype=np.float64)
        n = C.c_uint64(0)
        check(lib().fpca_king_pairs(self.h, _p(k8), float(thr), max_pairs, _p(i), _p(j), _p(phi), C.byref(n)))
        return i[:n.value].copy(), j[:n.value].copy(), phi[:n.value].copy()

    def king_cutoff(self, thr=0.0884, keep=None):
        """fpca_king_cutoff: the boolean mask of the samples left after removing, among those of `keep` (None: all), one sample at a time
        -- the one in most pairs with kinship above thr, the largest index among equals -- until no such pair remains.  0.0884 separates
        second-degree relatives from third-degree ones (0.177: first from second, 0.354: duplicates)."""
        k8 = self._sample_keep(keep)
        if k8 is None:
            k8 = np.ones(self.N, dtype=np.uint8)
        n = C.c_uint64(0)
        check(lib().fpca_king_cutoff(self.h, float(thr), _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def bench_king(self, reps=5):
        """fpca_bench_king: (milliseconds of each of `reps` passes of the pair kernel over the whole triangle, int8 MACs one pass issues)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        macs = C.c_double(0)
        check(lib().fpca_bench_king(self.h, int(reps), _p(ms), C.byref(macs)))
        return ms, macs.value

    def king_counts_block(self, i0, ni, j0, nj):
        """fpca_king_counts_block: (counts, phi) of any rectangle of samples -- counts is the ni x nj x 6 uint32 array of (shared, ibs0,
        hethet, het_i, het_j, D) per pair: the SNPs called in both samples, those at which they hold opposite homozygotes, those at which
        both are heterozygous, and the sums phi is made of; phi is king_block's array, bit for bit."""
        i0, ni, j0, nj = int(i0), int(ni), int(j0), int(nj)
        if min(i0, ni, j0, nj) < 0:
            raise ValueError("i0, ni, j0 and nj are non-negative")
        counts = np.empty((max(ni, 1), max(nj, 1), 6), dtype=np.uint32)  # (a zero-sized request still reaches the library's refusal)
        phi = np.empty((max(ni, 1), max(nj, 1)), dtype=np.float64)
        check(lib().fpca_king_counts_block(self.h, i0, ni, j0, nj, _p(counts), _p(phi)))
        return counts[:ni, :nj], phi[:ni, :nj]

    def king_related(self, thr=0.0442, keep=None, min_shared=0, max_pairs=1 << 24, po_ibs0=0.005):
        """fpca_king_related + fpca_king_classify: the relationship table of the pairs i < j with kinship phi > thr that share at least
        min_shared called SNPs, among the samples of `keep` (None: all), sorted by (i, j) -- a dict of arrays with one entry per pair:
        i, j, phi, shared, ibs0, hethet, het_i, het_j, dist (= D, the sum of squared dosage differences), ibs (PLINK's IBS similarity,
        1 - (D - 2 ibs0) / (2 shared)) and type (0 unrelated, 1 parent-offspring, 2 full sibs, 3 second degree, 4 third degree, 5
        duplicate / MZ, 255 no value; first degree is parent-offspring when ibs0 / shared < po_ibs0).  min_shared = 0 lists the pairs of
        king_pairs.  FpcaError (code -4, the message names the count) when more than max_pairs qualify."""
        k8 = self._sample_keep(keep)
        max_pairs, min_shared = int(max_pairs), int(min_shared)
        if max_pairs < 0:
            raise ValueError("max_pairs is non-negative")
        if not 0 <= min_shared <= 0xFFFFFFFF:
            raise ValueError("min_shared is a count of SNPs between 0 and 2^32 - 1")
        room = max(min(max_pairs, self.N * (self.N - 1) // 2), 1)
        i = np.empty(room, dtype=np.uint32)
        j = np.empty(room, dtype=np.uint32)
        phi = np.empty(room, dtype=np.float64)
        counts = np.empty((room, 6), dtype=np.uint32)
        n = C.c_uint64(0)
        check(lib().fpca_king_related(self.h, _p(k8), float(thr), min_shared, max_pairs, _p(i), _p(j), _p(phi), _p(counts), C.byref(n)))
        return _king_table(i[:n.value].copy(), j[:n.value].copy(), phi[:n.value].copy(), counts[:n.value].copy(), po_ibs0)

    def king_cutoff_shared(self, thr=0.0884, min_shared=0, keep=None):
        """fpca_king_cutoff_shared: king_cutoff in which a pair that shares fewer than min_shared called SNPs counts as unrelated, whatever
        its phi -- so that a poorly genotyped sample neither goes nor makes others go on the strength of a noisy coefficient.
        min_shared = 0 gives king_cutoff's mask."""
        k8 = self._sample_keep(keep)
        if k8 is None:
            k8 = np.ones(self.N, dtype=np.uint8)
        min_shared = int(min_shared)
        if not 0 <= min_shared <= 0xFFFFFFFF:
            raise ValueError("min_shared is a count of SNPs between 0 and 2^32 - 1")
        n = C.c_uint64(0)
        check(lib().fpca_king_cutoff_shared(self.h, float(thr), min_shared, _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def bench_king_rel(self, reps=5):
        """fpca_bench_king_rel: bench_king for the pair kernel of king_related."""
        ms = np.zeros(int(reps), dtype=np.float64)
        macs = C.c_double(0)
        check(lib().fpca_bench_king_rel(self.h, int(reps), _p(ms), C.byref(macs)))
        return ms, macs.value

    # ---- PC-AiR's partition ---------------------------------------------------------------------------
    def king_census(self, kin_thr=2 ** -5.5, div_thr=-2 ** -5.5, keep=None, exclude=None):
        """fpca_king_census: (n_rel, n_div), two uint32 arrays with one entry per sample -- the number of pairs with the sample whose
        KING-robust kinship phi is above kin_thr (related) and the number whose phi is below div_thr, that are not related, and that are
        not listed in `exclude` (divergent in ancestry), both among the samples of `keep` (None: all; a sample outside counts 0).
        exclude: (i, j), two arrays of sample indices -- pairs in either order, repeats allowed.  One pass over the triangle; a NaN phi is
        neither; kin_thr may be +inf."""
        k8 = self._sample_keep(keep)
        ei, ej = _pair_indices(exclude, "exclude")
        n_rel = np.zeros(self.N, dtype=np.uint32)
        n_div = np.zeros(self.N, dtype=np.uint32)
        check(lib().fpca_king_census(self.h, _p(k8), float(kin_thr), float(div_thr), _p(ei), _p(ej), ei.size, _p(n_rel), _p(n_div)))
        return n_rel, n_div

    def pcair_partition(self, kin_thr=2 ** -5.5, div_thr=-2 ** -5.5, keep=None, kin_pairs=None, counts=False):
        """fpca_pcair_king / fpca_pcair_pairs: PC-AiR's unrelated set as a boolean mask over the samples -- among those of `keep` (None:
        all), one sample at a time goes until no related pair remains: the one in most related pairs; among equals the one in fewest
        divergent pairs (king_census's n_div, fixed); among equals the one whose kinship to its remaining relatives sums lowest; among
        equals the largest index.  Related pairs are those with KING-robust phi > kin_thr, from one fused pass with the census; or, with
        kin_pairs=(i, j, kin), exactly the listed pairs (PC-Relate's, the relationship matrix's) -- KING then only counts the divergent
        pairs, never one of the listed ones, and kin_thr is unused.  counts=True: (mask, n_rel, n_div) as the rule saw them; n_rel is None
        with kin_pairs.  GENESIS::pcairPartition in structure; parity with it is not claimed."""
        k8 = self._sample_keep(keep)
        if k8 is None:
            k8 = np.ones(self.N, dtype=np.uint8)
        n = C.c_uint64(0)
        n_div = np.zeros(self.N, dtype=np.uint32)
        if kin_pairs is None:
            n_rel = np.zeros(self.N, dtype=np.uint32)
            check(lib().fpca_pcair_king(self.h, float(kin_thr), float(div_thr), _p(k8), C.byref(n), _p(n_rel), _p(n_div)))
        else:
            n_rel = None
            pi, pj, kin = _kin_pairs(kin_pairs)
            check(lib().fpca_pcair_pairs(self.h, float(div_thr), pi.size, _p(pi), _p(pj), _p(kin), _p(k8), C.byref(n), _p(n_div)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return (out, n_rel, n_div) if counts else out

    def bench_king_census(self, reps=5):
        """fpca_bench_king_census: milliseconds of each of `reps` passes of the census kernel over the whole triangle (bench_king's
        products, so its MAC count applies)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        check(lib().fpca_bench_king_census(self.h, int(reps), _p(ms)))
        return ms

    # ---- relationship matrix ------------------------------------------------------------------------
    def grm_block(self, i0, ni, j0, nj, divisor="shared", counts=False):
        """fpca_grm_block: the ni x nj array G of the genetic relationship matrix between sample i0 + a and sample j0 + b, any rectangle --
        S_ij = sum over the SNPs of the products of the two samples' standardised genotypes (the context's own table; 0 at a missing
        call), divided by n_ij, the live SNPs called in both (divisor "shared", GCTA's form; NaN when there is none), by the number of SNPs
        ("p": the X X' / P of the PCA) or not at all ("none").  counts=True: (G, n) with n the ni x nj uint32 array of shared calls."""
        i0, ni, j0, nj = int(i0), int(ni), int(j0), int(nj)
        if min(i0, ni, j0, nj) < 0:
            raise ValueError("i0, ni, j0 and nj are non-negative")
        out = np.empty((max(ni, 1), max(nj, 1)), dtype=np.float64)  # (a zero-sized request still reaches the library's refusal)
        n = np.empty(out.shape, dtype=np.uint32) if counts else None
        check(lib().fpca_grm_block(self.h, i0, ni, j0, nj, _grm_divisor(divisor), _p(out), _p(n)))
        return (out[:ni, :nj], n[:ni, :nj]) if counts else out[:ni, :nj]

    def grm_tri(self, divisor="shared", counts=False):
        """fpca_grm_tri: the lower triangle of the relationship matrix with its diagonal, row by row -- entry i (i + 1) / 2 + j is G_ij, j <= i
        (GCTA's order), N (N + 1) / 2 doubles.  counts=True: (G, n) with the shared calls in the same order."""
        size = self.N * (self.N + 1) // 2
        out = np.empty(size, dtype=np.float64)
        n = np.empty(size, dtype=np.uint32) if counts else None
        check(lib().fpca_grm_tri(self.h, _grm_divisor(divisor), _p(out), _p(n)))
        return (out, n) if counts else out

    def grm_pairs(self, thr, keep=None, divisor="shared", max_pairs=1 << 24):
        """fpca_grm_pairs: (i, j, g, shared) of every pair of samples i < j with relationship G > thr, sorted by (i, j), among the samples of
        `keep` (a boolean array with one entry per sample; None: all).  FpcaError (code -4, the message names the count) when more than
        max_pairs qualify."""
        k8 = self._sample_keep(keep)
        max_pairs = int(max_pairs)
        if max_pairs < 0:
            raise ValueError("max_pairs is non-negative")
        room = max(min(max_pairs, self.N * (self.N - 1) // 2), 1)
        i = np.empty(room, dtype=np.uint32)
        j = np.empty(room, dtype=np.uint32)
        g = np.empty(room, dtype=np.float64)
        sh = np.empty(room, dtype=np.uint32)
        n = C.c_uint64(0)
        check(lib().fpca_grm_pairs(self.h, _p(k8), float(thr), _grm_divisor(divisor), max_pairs, _p(i), _p(j), _p(g), _p(sh), C.byref(n)))
        return i[:n.value].copy(), j[:n.value].copy(), g[:n.value].copy(), sh[:n.value].copy()

    def grm_cutoff(self, thr=0.025, keep=None, divisor="shared"):
        """fpca_grm_cutoff: the boolean mask of the samples left after removing, among those of `keep` (None: all), one sample at a time
        -- the one in most pairs with relationship above thr, the largest index among equals (king_cutoff's rule) -- until no such pair
        remains.  The purpose of plink --rel-cutoff / gcta --grm-cutoff; 0.025 is the customary threshold."""
        k8 = self._sample_keep(keep)
        if k8 is None:
            k8 = np.ones(self.N, dtype=np.uint8)
        n = C.c_uint64(0)
        check(lib().fpca_grm_cutoff(self.h, float(thr), _grm_divisor(divisor), _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def bench_grm(self, reps=5):
        """fpca_bench_grm: (milliseconds of each of `reps` passes of the FP64 Gram kernel over the whole lower triangle, floating-point
        operations one pass issues)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        flops = C.c_double(0)
        check(lib().fpca_bench_grm(self.h, int(reps), _p(ms), C.byref(flops)))
        return ms, flops.value

    # ---- PC-Relate ------------------------------------------------------------------------------------
    def _pcr_args(self, pcs, train, beta=None):
        pcs = np.asarray(pcs, dtype=np.float64)
        if pcs.ndim == 1 and pcs.size == self.N:
            pcs = pcs.reshape(self.N, 1)
        if pcs.ndim != 2 or pcs.shape[0] != self.N:
            raise ValueError("pcs must have one row per sample (%d), it has shape %s" % (self.N, pcs.shape))
        pcs = np.ascontiguousarray(pcs)
        if beta is not None:
            beta = np.ascontiguousarray(beta, dtype=np.float64)
            if beta.shape != (self.P, pcs.shape[1] + 1):
                raise ValueError("beta must be %d x %d (one row per SNP, the intercept first), it has shape %s" % (self.P, pcs.shape[1] + 1, beta.shape))
        return pcs, self._sample_keep(train), beta

    def pcrelate_beta(self, pcs, train=None):
        """fpca_pcrelate_beta: the P x (npc + 1) coefficients of every SNP's regression on [1 | pcs] over the samples of `train` (a boolean
        array with one entry per sample, the unrelated set; None: all) -- dosages with the context's mean at a missing call.  pcs: N x npc,
        npc <= 31.  Half the fitted value is PC-Relate's individual-specific allele frequency."""
        pcs, t8, _ = self._pcr_args(pcs, train)
        out = np.empty((self.P, pcs.shape[1] + 1), dtype=np.float64)
        check(lib().fpca_pcrelate_beta(self.h, _p(pcs), pcs.shape[1], _p(t8), _p(out)))
        return out

    def pcrelate_block(self, pcs, i0, ni, j0, nj, train=None, eps=0.01, beta=None, den=False):
        """fpca_pcrelate_block: the ni x nj array of PC-Relate kinship between sample i0 + a and sample j0 + b, any rectangle: with mu =
        [1 | pcs] beta / 2, the sum of (x_i - 2 mu_i)(x_j - 2 mu_j) over 4 x the sum of sqrt(mu_i (1 - mu_i) mu_j (1 - mu_j)), both over the
        SNPs that are live, called and have eps < mu < 1 - eps in both samples (NaN when there is none).  beta: what pcrelate_beta returned
        (None: estimated from `train` inside the call, the same bits).  den=True: (kin, the denominator sums)."""
        pcs, t8, beta = self._pcr_args(pcs, train, beta)
        i0, ni, j0, nj = int(i0), int(ni), int(j0), int(nj)
        if min(i0, ni, j0, nj) < 0:
            raise ValueError("i0, ni, j0 and nj are non-negative")
        out = np.empty((max(ni, 1), max(nj, 1)), dtype=np.float64)  # (a zero-sized request still reaches the library's refusal)
        dn = np.empty(out.shape, dtype=np.float64) if den else None
        check(lib().fpca_pcrelate_block(self.h, _p(pcs), pcs.shape[1], _p(beta), _p(t8), float(eps), i0, ni, j0, nj, _p(out), _p(dn)))
        return (out[:ni, :nj], dn[:ni, :nj]) if den else out[:ni, :nj]

    def pcrelate_tri(self, pcs, train=None, eps=0.01, beta=None, den=False):
        """fpca_pcrelate_tri: the lower triangle of the PC-Relate kinship matrix with its diagonal, row by row -- entry i (i + 1) / 2 + j is
        kin_ij, j <= i, N (N + 1) / 2 doubles; the diagonal is (1 + inbreeding) / 2.  den=True: (kin, the denominator sums in the same order)."""
        pcs, t8, beta = self._pcr_args(pcs, train, beta)
        size = self.N * (self.N + 1) // 2
        out = np.empty(size, dtype=np.float64)
        dn = np.empty(size, dtype=np.float64) if den else None
        check(lib().fpca_pcrelate_tri(self.h, _p(pcs), pcs.shape[1], _p(beta), _p(t8), float(eps), _p(out), _p(dn)))
        return (out, dn) if den else out

    def bench_pcrelate(self, npc=4, reps=5):
        """fpca_bench_pcrelate: (milliseconds of each of `reps` passes of PC-Relate's Gram kernel over the whole lower triangle,
        floating-point operations one pass issues, both Grams counted)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        flops = C.c_double(0)
        check(lib().fpca_bench_pcrelate(self.h, int(npc), int(reps), _p(ms), C.byref(flops)))
        return ms, flops.value

    def _ibd_f(self, f):
        if f is None:
            return None
        f = np.ascontiguousarray(f, dtype=np.float64)
        if f.shape != (self.N,):
            raise ValueError("f must have one entry per sample (%d), it has shape %s" % (self.N, f.shape))
        return f

    def pcrelate_ibd_block(self, pcs, i0, ni, j0, nj, f=None, train=None, eps=0.01, beta=None):
        """fpca_pcrelate_ibd_block: PC-Relate's IBD sharing between sample i0 + a and sample j0 + b, any rectangle -- a dict of ni x nj arrays:
        `k2` = sum q_i q_j / sum v_i v_j - f_i f_j, `k0` = the opposite homozygotes over sum (mu_i^2 (1 - mu_j)^2 + (1 - mu_i)^2 mu_j^2), both
        over the SNPs usable in both samples (NaN when there is none), and `nsnp`, their number (uint32).  f: the inbreeding coefficients,
        2 x the diagonal of pcrelate_tri - 1 (None: zeros).  pcs, train, eps, beta as in pcrelate_block."""
        pcs, t8, beta = self._pcr_args(pcs, train, beta)
        f = self._ibd_f(f)
        i0, ni, j0, nj = int(i0), int(ni), int(j0), int(nj)
        if min(i0, ni, j0, nj) < 0:
            raise ValueError("i0, ni, j0 and nj are non-negative")
        shape = (max(ni, 1), max(nj, 1))  # (a zero-sized request still reaches the library's refusal)
        k2, k0, n = np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.uint32)
        check(lib().fpca_pcrelate_ibd_block(self.h, _p(pcs), pcs.shape[1], _p(beta), _p(t8), float(eps), _p(f), i0, ni, j0, nj, _p(k2), _p(k0), _p(n)))
        return dict(k2=k2[:ni, :nj], k0=k0[:ni, :nj], nsnp=n[:ni, :nj])

    def pcrelate_ibd_tri(self, pcs, f=None, train=None, eps=0.01, beta=None):
        """fpca_pcrelate_ibd_tri: what pcrelate_ibd_block returns for the lower triangle with its diagonal, row by row -- entry
        i (i + 1) / 2 + j, j <= i, N (N + 1) / 2 entries in each of `k2`, `k0`, `nsnp`.  The diagonal carries no meaning."""
        pcs, t8, beta = self._pcr_args(pcs, train, beta)
        f = self._ibd_f(f)
        size = self.N * (self.N + 1) // 2
        k2, k0, n = np.empty(size, dtype=np.float64), np.empty(size, dtype=np.float64), np.empty(size, dtype=np.uint32)
        check(lib().fpca_pcrelate_ibd_tri(self.h, _p(pcs), pcs.shape[1], _p(beta), _p(t8), float(eps), _p(f), _p(k2), _p(k0), _p(n)))
        return dict(k2=k2, k0=k0, nsnp=n)

    def bench_pcrelate_ibd(self, npc=4, reps=5):
        """fpca_bench_pcrelate_ibd: (milliseconds of each of `reps` passes of the three Gram instances of PC-Relate's IBD sharing over the
        whole lower triangle, floating-point operations one pass issues, seven products counted)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        flops = C.c_double(0)
        check(lib().fpca_bench_pcrelate_ibd(self.h, int(npc), int(reps), _p(ms), C.byref(flops)))
        return ms, flops.value

    # ---- genotype census ------------------------------------------------------------------------------
    def snp_counts(self, samples=None):
        """fpca_snp_counts: the P x 4 uint32 array of genotype counts per SNP by raw .bed code (0 homozygous A1, 1 missing, 2 heterozygous,
        3 homozygous A2) over the samples of `samples` (a boolean array with one entry per sample; None: all)."""
        out = np.empty((self.P, 4), dtype=np.uint32)
        check(lib().fpca_snp_counts(self.h, _p(self._sample_keep(samples)), _p(out)))
        return out

    def sample_counts(self, snps=None):
        """fpca_sample_counts: the N x 4 uint32 array of genotype counts per sample by raw .bed code over the SNPs of `snps` (a mask or an
        index array; None: all)."""
        s8 = None if snps is None else np.ascontiguousarray(_snp_mask(snps, self.P), dtype=np.uint8)
        out = np.empty((self.N, 4), dtype=np.uint32)
        check(lib().fpca_sample_counts(self.h, _p(s8), _p(out)))
        return out

    def hwe_exact(self, counts):
        """fpca_hwe_exact: the Hardy-Weinberg exact-test p-value (Wigginton, Cutler & Abecasis 2005; no mid-p) of every row of `counts`,
        an n x 4 array of non-negative integers by raw code as snp_counts() returns it (column 1, the missing calls, is not read)."""
        c = np.asarray(counts)
        if c.ndim != 2 or c.shape[1] != 4 or not (c.size == 0 or np.issubdtype(c.dtype, np.integer)):
            raise ValueError("counts is an n x 4 array of integers (hom A1, missing, het, hom A2), found shape %s" % (c.shape,))
        if c.size and (c.min() < 0 or c.max() >= 2 ** 32):
            raise ValueError("counts must be in 0 .. 2^32 - 1")
        c32 = np.ascontiguousarray(c, dtype=np.uint32)
        out = np.empty(c32.shape[0], dtype=np.float64)
        check(lib().fpca_hwe_exact(self.h, _p(c32), c32.shape[0], _p(out)))
        return out

    def sample_qc(self, mind, snps=None, keep=None):
        """fpca_sample_qc: the boolean mask of the samples whose missing-call rate over the SNPs of `snps` (a mask or an index array; None:
        all) is <= mind (PLINK's --mind; mind >= 1 switches the filter off), among those of `keep` (one entry per sample; None: all)."""
        s8 = None if snps is None else np.ascontiguousarray(_snp_mask(snps, self.P), dtype=np.uint8)
        k8 = self._sample_keep(keep)
        if k8 is None:
            k8 = np.ones(self.N, dtype=np.uint8)
        n = C.c_uint64(0)
        check(lib().fpca_sample_qc(self.h, _p(s8), float(mind), _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def snp_qc_samples(self, samples, maf=0.0, geno=1.0, hwe=0.0, keep=None):
        """fpca_snp_qc_samples: the boolean mask of the SNPs with minor-allele frequency >= maf, missing-call rate <= geno and HWE exact-test
        p-value >= hwe (PLINK's --maf / --geno / --hwe; maf <= 0, geno >= 1 and hwe <= 0 switch a filter off), all three taken over the
        samples of `samples` (one entry per sample; None: all), among the SNPs of `keep` (a mask or an index array; None: all)."""
        k8 = np.ascontiguousarray(np.ones(self.P, dtype=bool) if keep is None else _snp_mask(keep, self.P), dtype=np.uint8)
        n = C.c_uint64(0)
        check(lib().fpca_snp_qc_samples(self.h, _p(self._sample_keep(samples)), float(maf), float(geno), float(hwe), _p(k8), C.byref(n)))
        out = k8 != 0
        assert int(out.sum()) == n.value
        return out

    def bench_qc(self, reps=5):
        """fpca_bench_qc: (milliseconds per launch of the per-SNP count pass, of the per-sample count pass and of the HWE kernel; the
        recurrence steps one HWE launch makes at most)."""
        ms = np.zeros(3, dtype=np.float64)
        steps = C.c_double(0)
        check(lib().fpca_bench_qc(self.h, int(reps), _p(ms), C.byref(steps)))
        return ms, steps.value

    def set_total_snps(self, P_total):
        check(lib().fpca_set_total_snps(self.h, int(P_total)))
        self.P_total = int(P_total)

    # ---- operator -------------------------------------------------------------------------------------
    def apply_xxt(self, B):
        B = np.asfortranarray(np.atleast_2d(B.T).T if B.ndim == 1 else B, dtype=np.float64)
        Y = np.empty_like(B, order="F")
        check(lib().fpca_apply_xxt(self.h, _p(B), B.shape[0], B.shape[1], _p(Y), Y.shape[0]))
        return Y

    def apply_xt(self, B):
        B = np.asfortranarray(B.reshape(self.N, -1), dtype=np.float64)
        T = np.empty((self.P, B.shape[1]), order="F")
        check(lib().fpca_apply_xt(self.h, _p(B), B.shape[0], B.shape[1], _p(T), self.P))
        return T

    def apply_x(self, T):
        T = np.asfortranarray(T.reshape(self.P, -1), dtype=np.float64)
        Y = np.empty((self.N, T.shape[1]), order="F")
        check(lib().fpca_apply_x(self.h, _p(T), self.P, T.shape[1], _p(Y), self.N))
        return Y

    # ---- multi-GPU -------------------------------------------------------------------------------------
    def set_allreduce(self, pyfunc):
        """pyfunc(dev_ptr:int, count:int, stream:int) -> 0 on success; sums `count` fp64 in place across ranks."""
        cb = _lib.ALLREDUCE_FN(lambda user, ptr, count, stream: int(pyfunc(ptr, count, stream) or 0))
        self._keep.append(cb)
        check(lib().fpca_set_allreduce(self.h, cb, None))

    def set_collectives(self, allgather, reducescatter):
        """allgather(send_ptr, recv_ptr, count_per_rank, stream) / reducescatter(send_ptr, recv_ptr, count_per_rank, stream) -> 0:
        fp64 collectives on raw device pointers beside set_allreduce (fpca_set_collectives); the row-sharded solver then issues
        the call sequence it issues over RCCL."""
        ag = _lib.COLLECTIVE_FN(lambda user, snd, rcv, count, stream: int(allgather(snd, rcv, count, stream) or 0))
        rs = _lib.COLLECTIVE_FN(lambda user, snd, rcv, count, stream: int(reducescatter(snd, rcv, count, stream) or 0))
        self._keep += [ag, rs]
        check(lib().fpca_set_collectives(self.h, ag, rs, None))

    def set_rank(self, nranks, rank):
        """rank / size beside a caller-supplied all-reduce: lets fpca_pca row-shard the solver (fpca_set_rank)."""
        check(lib().fpca_set_rank(self.h, nranks, rank))

    def collective_stats(self):
        calls, nbytes = C.c_uint64(0), C.c_uint64(0)
        check(lib().fpca_collective_stats(self.h, C.byref(calls), C.byref(nbytes)))
        return int(calls.value), int(nbytes.value)

    def comm_init_rank(self, nranks, rank, unique_id):
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        check(lib().fpca_comm_init_rank(self.h, nranks, rank, buf))

    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * _lib.UNIQUE_ID_BYTES)()
        check(lib().fpca_comm_unique_id(buf))
        return bytes(buf)

    # ---- driver ---------------------------------------------------------------------------------------
    def pca(self, ndim=10, tol=1e-6, maxiter=500, div="p", do_loadings=False, blockvec=0, max_blocks=0, seed=1, verbose=0,
            allow_unconverged=False, max_applies=0, replicated_solver=False, mixed=0, cheap_slices=0, partial_rows=False):
        """fpca_pca.  allow_unconverged: FPCA_ENOTCONVERGED comes back as a result (info["converged"] == 0) whose U / d / Px / pve hold
        the current Rayleigh-Ritz pairs (pca_driver.hpp) instead of raising.  partial_rows (several ranks): U / Px carry only this
        rank's rows (result["row_ranges"]), NaN elsewhere."""
        o = PcaOpts()
        lib().fpca_pca_init_opts(C.byref(o), C.sizeof(PcaOpts), C.sizeof(PcaInfo))
        o.ndim, o.tol, o.maxiter, o.divisor = ndim, tol, maxiter, DIVISOR[div]
        o.do_loadings, o.blockvec, o.max_blocks, o.seed, o.verbose = int(do_loadings), blockvec, max_blocks, seed, verbose
        o.max_applies = max_applies
        o.replicated_solver = int(replicated_solver)
        o.mixed, o.cheap_slices = int(mixed), int(cheap_slices)  # mixed: 0 automatic (on), 1 on, -1 off (every pass exact)
        o.partial_rows = int(partial_rows)
        # (the small outputs are NaN-filled: what the library does not write can never pass for a result; the N x ndim ones only
        #  under partial_rows, where another rank's rows stay unwritten -- filling 160 MB costs a timed solve 8 ms of page faults,
        #  and a call that fails raises, FPCA_ENOTCONVERGED fills everything)
        mk = (lambda shape: np.full(shape, np.nan, order="F")) if partial_rows else (lambda shape: np.empty(shape, order="F"))
        U = mk((self.N, ndim))
        d = np.full(ndim, np.nan)
        Px = mk((self.N, ndim))
        pve = np.full(ndim, np.nan)
        V = np.empty((self.P, ndim), order="F") if do_loadings else None
        ms = np.empty((self.P, 2), order="F")
        info = PcaInfo()
        rc = lib().fpca_pca(self.h, C.byref(o), _p(U), _p(d), _p(Px), _p(pve), _p(V), _p(ms), C.byref(info))
        if rc != 0 and not (allow_unconverged and rc == -5):
            check(rc)
        out = dict(U=U, d=d, Px=Px, pve=pve, V=V, meansd=ms, info={f[0]: getattr(info, f[0]) for f in PcaInfo._fields_})
        if partial_rows:
            rg = (C.c_uint64 * 16)()
            n = lib().fpca_pca_row_ranges(self.h, C.byref(o), rg, 8)
            if n < 0:
                check(n)
            out["row_ranges"] = [(int(rg[2 * i]), int(rg[2 * i + 1])) for i in range(n)]
        return out

    def check(self, evec, evals, div="p"):
        evec = np.asfortranarray(evec, dtype=np.float64)
        evals = np.ascontiguousarray(evals, dtype=np.float64)
        k = evec.shape[1]
        err = np.empty(k)
        mse, rmse = C.c_double(0), C.c_double(0)
        check(lib().fpca_check(self.h, _p(evec), evec.shape[0], _p(evals), k, DIVISOR[div], _p(err), C.byref(mse), C.byref(rmse)))
        return err, mse.value, rmse.value

    def ucca(self, Y, standy="sd"):
        """fpca_ucca: per-SNP association of this shard's SNPs with the N x k phenotypes Y (NaN = missing), standardised by `standy`
        (none / sd / binom / binom2 / center).  Returns a (P, 3) array: R, Fstat, P (RandomPCA::ucca + wilks, randompca.cpp:103-119,
        530-625)."""
        if standy not in _lib.STANDARDISE_DENSE:
            raise ValueError("standy must be one of %s" % sorted(_lib.STANDARDISE_DENSE))
        Y = np.asarray(Y, dtype=np.float64)
        Y = np.asfortranarray(Y.reshape(-1, 1) if Y.ndim == 1 else Y)
        if Y.ndim != 2 or Y.shape[0] != self.N:
            raise ValueError("Y must have %d rows (one per sample), it has %d" % (self.N, Y.shape[0]))
        res = np.empty((self.P, 3), order="F")
        check(lib().fpca_ucca(self.h, _p(Y), Y.shape[0], Y.shape[1], _lib.STANDARDISE_DENSE[standy], _p(res), self.P))
        return res

    def scca_prepare(self, Y, standy="sd", divisor="n1"):
        """fpca_scca_prepare: standardise the N x k phenotypes Y (NaN = missing) by `standy`, scale by 1 / sqrt(N - 1) for divisor
        "n1", and form C = X'Y on the device with one pass over the genotypes; kept until the next scca_prepare or close()."""
        if standy not in _lib.STANDARDISE_DENSE:
            raise ValueError("standy must be one of %s" % sorted(_lib.STANDARDISE_DENSE))
        if divisor not in ("n1", "none"):
            raise ValueError("divisor must be 'n1' or 'none'")
        Y = np.asarray(Y, dtype=np.float64)
        Y = np.asfortranarray(Y.reshape(-1, 1) if Y.ndim == 1 else Y)
        if Y.ndim != 2 or Y.shape[0] != self.N:
            raise ValueError("Y must have %d rows (one per sample), it has %d" % (self.N, Y.shape[0]))
        check(lib().fpca_scca_prepare(self.h, _p(Y), Y.shape[0], Y.shape[1], _lib.STANDARDISE_DENSE[standy], DIVISOR[divisor]))
        self._scca_k = Y.shape[1]

    def scca_fit(self, lambda1, lambda2, ndim, V0, maxiter=1000, tol=1e-4):
        """fpca_scca_fit: one sparse CCA model on the prepared phenotypes from the k x ndim starting vectors V0 (RandomPCA::scca,
        randompca.cpp:387-528).  Returns U (P x ndim), V (k x ndim), d, Px, Py (N x ndim), converged, iters, nzero_x, nzero_y and
        status ("ok", "maxiter reached", "lambda1 too large", "lambda2 too large")."""
        k = getattr(self, "_scca_k", None)
        V0 = np.asarray(V0, dtype=np.float64)
        V0 = np.asfortranarray(V0.reshape(-1, 1) if V0.ndim == 1 else V0)
        ndim = int(ndim)
        if k is not None and ndim >= 1 and V0.shape != (k, ndim):
            raise ValueError("dimensions of V must be (ncol(Y) x (ndim))")
        n = max(ndim, 1)
        U = np.full((self.P, n), np.nan, order="F")
        V = np.full((max(k or 1, 1), n), np.nan, order="F")
        d = np.full(n, np.nan)
        Px = np.full((self.N, n), np.nan, order="F")
        Py = np.full((self.N, n), np.nan, order="F")
        conv, status = C.c_int(0), C.c_int(0)
        iters = np.zeros(n, dtype=np.intc)
        nzx = np.zeros(n, dtype=np.int64)
        nzy = np.zeros(n, dtype=np.int64)
        check(lib().fpca_scca_fit(self.h, float(lambda1), float(lambda2), ndim, int(maxiter), float(tol), _p(V0), V0.shape[0], _p(U), self.P,
                                  _p(V), V.shape[0], _p(d), _p(Px), self.N, _p(Py), self.N, C.byref(conv), _p(iters), _p(nzx), _p(nzy),
                                  C.byref(status)))
        return dict(U=U, V=V, d=d, Px=Px, Py=Py, converged=bool(conv.value), iters=iters, nzero_x=nzx, nzero_y=nzy,
                    status=_lib.SCCA_STATUS[status.value])

    def scca_cv(self, Y, folds, lambda1, lambda2, ndim, V0, standy="sd", divisor="n1", maxiter=1000, tol=1e-4, warm_lambda=1e-12, opt_dim=1,
                return_pred=False):
        """fpca_scca_cv: K-fold cross-validation of the SCCA penalties (the R function cv.scca(), flashpcaR/R/scca.R:410-557) on this
        context's packed genotypes.  folds: one id in 0 .. nfolds - 1 per sample; V0: (nfolds, k, ndim), or (k, ndim) for every fold;
        warm_lambda < 0 (or None): no warm start.  Returns corr, nzero_x, nzero_y (ndim, n1, n2), converged (nfolds, n1, n2), iters
        (nfolds, n1, n2, ndim), warm_iters (nfolds, ndim), best_lambda1, best_lambda2, best_corr and, with return_pred, xpred / ypred
        (N, ndim, n1, n2)."""
        if standy not in _lib.STANDARDISE_DENSE:
            raise ValueError("standy must be one of %s" % sorted(_lib.STANDARDISE_DENSE))
        if divisor not in ("n1", "none"):
            raise ValueError("divisor must be 'n1' or 'none'")
        Y = np.asarray(Y, dtype=np.float64)
        Y = np.asfortranarray(Y.reshape(-1, 1) if Y.ndim == 1 else Y)
        if Y.ndim != 2 or Y.shape[0] != self.N:
            raise ValueError("Y must have %d rows (one per sample), it has %d" % (self.N, Y.shape[0]))
        k, ndim = Y.shape[1], int(ndim)
        folds = np.asarray(folds)
        if folds.shape != (self.N,):
            raise ValueError("'folds' must be of same number of rows as X and Y")
        if folds.min() < 0 or folds.max() > 255:
            raise ValueError("fold ids must be in 0 .. 63")
        nfolds = int(folds.max()) + 1
        folds8 = np.ascontiguousarray(folds, dtype=np.uint8)
        l1 = np.ascontiguousarray(np.atleast_1d(lambda1), dtype=np.float64)
        l2 = np.ascontiguousarray(np.atleast_1d(lambda2), dtype=np.float64)
        n1, n2, nd = l1.size, l2.size, max(ndim, 1)
        V0 = np.asarray(V0, dtype=np.float64)
        if V0.ndim == 2:
            V0 = V0[None]
        if V0.ndim != 3 or V0.shape[1:] != (k, nd) or V0.shape[0] not in (1, nfolds):
            raise ValueError("dimensions of V must be (ncol(Y) x (ndim)), one matrix per fold")
        V0 = np.ascontiguousarray(V0.transpose(0, 2, 1))  # [fold][dimension][phenotype]: column-major k x ndim matrices
        corr = np.full((nd, n1, n2), np.nan)
        nzx = np.full((nd, n1, n2), np.nan)
        nzy = np.full((nd, n1, n2), np.nan)
        conv = np.zeros((nfolds, n1, n2), dtype=np.intc)
        iters = np.zeros((nfolds, n1, n2, nd), dtype=np.intc)
        witers = np.zeros((nfolds, nd), dtype=np.intc)
        b1, b2, bc = C.c_double(np.nan), C.c_double(np.nan), C.c_double(np.nan)
        xp = np.empty((n1, n2, nd, self.N)) if return_pred else None
        yp = np.empty((n1, n2, nd, self.N)) if return_pred else None
        check(lib().fpca_scca_cv(self.h, _p(Y), Y.shape[0], k, _p(folds8), nfolds, _p(l1), n1, _p(l2), n2, ndim, _lib.STANDARDISE_DENSE[standy],
                                 DIVISOR[divisor], int(maxiter), float(tol), _p(V0), k, k * nd if V0.shape[0] > 1 else 0,
                                 -1.0 if warm_lambda is None else float(warm_lambda), int(opt_dim), _p(corr), _p(nzx), _p(nzy), _p(conv), _p(iters),
                                 _p(witers), C.byref(b1), C.byref(b2), C.byref(bc), _p(xp), _p(yp)))
        out = dict(corr=corr, nzero_x=nzx, nzero_y=nzy, converged=conv.astype(bool), iters=iters, warm_iters=witers, best_lambda1=b1.value,
                   best_lambda2=b2.value, best_corr=bc.value)
        if return_pred:
            out["xpred"], out["ypred"] = xp.transpose(3, 2, 0, 1), yp.transpose(3, 2, 0, 1)
        return out

    def fold_stats(self, folds, nfolds, which_fold=None):
        """fpca_debug_fold_stats: counts (nfolds, P, 3) of the samples of every fold with dosage 0 / 1 / 2 and, for which_fold, the
        (P, 2) mean / sd over the samples outside it as scca_cv installs them."""
        folds8 = np.ascontiguousarray(folds, dtype=np.uint8)
        assert folds8.shape == (self.N,)
        counts = np.zeros((nfolds, self.P, 3), dtype=np.uint32)
        ms = np.empty((self.P, 2), order="F") if which_fold is not None else None
        check(lib().fpca_debug_fold_stats(self.h, _p(folds8), int(nfolds), _p(counts), -1 if which_fold is None else int(which_fold), _p(ms)))
        return counts, ms

    def missing_lists(self, b, by_sample):
        """fpca_debug_missing_lists: (ptr, idx) of the missing-call index lists of a list route (missing_mode(b) 3 or 4), by SNP
        (by_sample False: P + 1 pointers, sample indices) or by sample (N + 1 pointers, SNP indices); FpcaError on any other route."""
        ptr = np.zeros((self.N if by_sample else self.P) + 1, dtype=np.uint32)
        nnz = C.c_uint64(0)
        check(lib().fpca_debug_missing_lists(self.h, int(b), int(bool(by_sample)), _p(ptr), None, 0, C.byref(nnz)))
        idx = np.zeros(max(nnz.value, 1), dtype=np.uint32)
        check(lib().fpca_debug_missing_lists(self.h, int(b), int(bool(by_sample)), _p(ptr), _p(idx), idx.size, C.byref(nnz)))
        return ptr, idx[:nnz.value]

    # ---- measurement -----------------------------------------------------------------------------------
    def bench_apply(self, b=32, steps=10, warmup=2):
        r = BenchResult()
        check(lib().fpca_bench_apply(self.h, b, steps, warmup, C.byref(r)))
        return {f[0]: getattr(r, f[0]) for f in BenchResult._fields_}

    def block_rows(self):
        return int(lib().fpca_block_rows(self.h))

    def apply_xxt_dev(self, dB_ptr, b, dY_ptr, stream=None):
        """Device-resident operator on row-major [block_rows][b] fp64 blocks given by raw device pointers."""
        check(lib().fpca_apply_xxt_dev(self.h, C.c_void_p(dB_ptr), b, C.c_void_p(dY_ptr), C.c_void_p(stream) if stream else None))

    def synchronize(self):
        check(lib().fpca_synchronize(self.h))

    def profile_begin(self, max_steps, sample_every=1):
        check(lib().fpca_profile_sample_every(self.h, sample_every))
        check(lib().fpca_profile_begin(self.h, max_steps))

    def profile_end(self, b):
        r = BenchResult()
        n = C.c_int(0)
        check(lib().fpca_profile_end(self.h, b, C.byref(r), C.byref(n)))
        out = {f[0]: getattr(r, f[0]) for f in BenchResult._fields_}
        out["nsteps"] = n.value
        return out

    def bench_stats(self, reps=5):
        ms, by = C.c_double(0), C.c_double(0)
        check(lib().fpca_bench_stats(self.h, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value


def debug_gather(ptr, idx, V, b, rows_out=None, rowscale=None, colw=None, init=None, short_lists=False, avg_len=0.0):
    """fpca_debug_gather: the gather-sum kernels of the missing-call list routes on caller data.  ptr (nrec + 1), idx: the lists; V:
    v_rows x b, fp64 or fp32 (fp32 takes colw, b factors; fp64 may take rowscale, v_rows factors); init: rows_out x b or None.
    Returns (out, rows_out x b fp64; the kernel that ran: 1, 2 or 3)."""
    ptr = np.ascontiguousarray(ptr, dtype=np.uint32)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    f32 = np.asarray(V).dtype == np.float32
    V = np.ascontiguousarray(V, dtype=np.float32 if f32 else np.float64)
    nrec = ptr.size - 1
    rows_out = nrec if rows_out is None else int(rows_out)
    if V.ndim != 2 or V.shape[1] != b or nrec < 0 or int(ptr[-1]) != idx.size:
        raise ValueError("V is v_rows x b, ptr has one entry more than there are lists and ends at len(idx)")
    rowscale = None if rowscale is None else np.ascontiguousarray(rowscale, dtype=np.float64)
    colw = None if colw is None else np.ascontiguousarray(colw, dtype=np.float64)
    init = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    if (rowscale is not None and rowscale.shape != (V.shape[0],)) or (colw is not None and colw.shape != (b,)) or (
            init is not None and init.shape != (rows_out, b)):
        raise ValueError("rowscale has one entry per row of V, colw one per column, init is rows_out x b")
    out = np.empty((max(rows_out, 1), b), dtype=np.float64)
    variant = C.c_int(0)
    idx_arg = idx if idx.size else np.zeros(1, dtype=np.uint32)
    check(lib().fpca_debug_gather(int(b), int(f32), _p(ptr), _p(idx_arg), idx.size, _p(V), V.shape[0], _p(rowscale), _p(colw), _p(init), nrec,
                                  rows_out, int(bool(short_lists)), float(avg_len), _p(out), C.byref(variant)))
    return out[:rows_out], variant.value


def debug_i8_slices(V, b, S, rows=None, route=0, rowscales=(), peers=None, rows_valid=0, colsum=(True, True), copy=(None, None), dequant=()):
    """fpca_debug_i8_slices: the int8 slicing kernels on caller data.  V: rows_pad x b fp64, of which `rows` rows count (default all); route 0:
    the operator's own slicing (i8_colmax, i8_slice), route 1: the row-sharded exchange (i8_slice_rows, i8_unpack_slices, i8_dequant_rows);
    rowscales: 0, 1 or 2 vectors of `rows` factors (2: two operands from one pass, route 0); peers: G-1 x 64 maxima of other ranks;
    colsum[o]: ask operand o for its column sums; copy[o]: None, 32 or 64, the copy of the scaled operand the slicing pass leaves;
    dequant: which of (32, 64) i8_dequant_rows is run for (route 1).  Returns one dict per operand: colmax [64], maxbits_own and maxbits
    [8][64] uint64, Q [nsc_pad][rows_pad] int8, colw [nsc_pad], nsc_pad, and where asked for colsum [640] int64 (the shards summed) with
    colsum_shards [8][640], copy32 / copy64 [rows_pad][b], and on route 1 Qrm [rows_pad][S b], dq32 / dq64."""
    V = np.ascontiguousarray(V, dtype=np.float64)
    if V.ndim != 2 or V.shape[1] != b:
        raise ValueError("V is rows_pad x b")
    rows_pad = V.shape[0]
    rows = rows_pad if rows is None else int(rows)
    rs = [np.ascontiguousarray(r, dtype=np.float64) for r in rowscales]
    if len(rs) > 2 or any(r.shape != (rows,) for r in rs):
        raise ValueError("at most two row scales, of `rows` factors each")
    if peers is not None:
        peers = np.ascontiguousarray(peers, dtype=np.float64)
        if peers.ndim != 2 or peers.shape[1] != 64:
            raise ValueError("peers is (G - 1) x 64")
    nsc = C.c_int(0)
    check(lib().fpca_debug_i8_nsc_pad(int(S), int(b), C.byref(nsc)))
    nsc, nops = nsc.value, max(1, len(rs))
    res, structs, keep = [], [], []
    for o in range(nops):
        a = dict(colmax=np.empty(64), maxbits_own=np.empty((8, 64), dtype=np.uint64), maxbits=np.empty((8, 64), dtype=np.uint64),
                 Q=np.empty((nsc, rows_pad), dtype=np.int8), colw=np.empty(nsc))
        if colsum[o]:
            a["colsum"] = np.empty((8, 640), dtype=np.int64)
        if copy[o] is not None:
            a["copy%d" % copy[o]] = np.empty((rows_pad, b), dtype=np.float32 if copy[o] == 32 else np.float64)
        if route == 1:
            a["Qrm"] = np.empty((rows_pad, S * b), dtype=np.int8)
            for w in dequant:
                a["dq%d" % w] = np.empty((rows_pad, b), dtype=np.float32 if w == 32 else np.float64)
        st = _lib.SlicesOut()
        for name, arr in a.items():
            setattr(st, name, arr.ctypes.data)
        structs.append(st)
        res.append(a)
    got = C.c_int(0)
    check(lib().fpca_debug_i8_slices(int(route), int(b), int(S), rows, rows_pad, int(rows_valid), _p(V), _p(rs[0]) if rs else None,
                                     _p(rs[1]) if len(rs) > 1 else None, _p(peers), 0 if peers is None else peers.shape[0], C.byref(structs[0]),
                                     C.byref(structs[1]) if nops > 1 else None, C.byref(got)))
    for a in res:
        a["nsc_pad"] = got.value
        if "colsum" in a:
            a["colsum_shards"] = a["colsum"]
            a["colsum"] = a["colsum_shards"].sum(axis=0)
    return res


def debug_i8_instances():
    """fpca_debug_i8_instances: every int8 GEMM kernel instance as a tuple (two operands, mode, nt, half tile, tile rows, band-tiled), in the
    order of the table; host only."""
    n = C.c_int(0)
    check(lib().fpca_debug_i8_instances(None, 0, C.byref(n)))
    keys = np.zeros((n.value, 6), dtype=np.int32)
    check(lib().fpca_debug_i8_instances(_p(keys), n.value, C.byref(n)))
    return [(bool(k[0]), int(k[1]), int(k[2]), bool(k[3]), int(k[4]), bool(k[5])) for k in keys[:n.value]]


def debug_gather_blocks(gemm_waves, gemm_vgprs, gemm_lds, gather_vgprs, ncu, rows_out=1 << 30):
    """fpca_debug_gather_blocks: the grid of a side-stream gather beside a GEMM whose workgroup has gemm_waves waves, gemm_vgprs registers per
    lane and gemm_lds bytes of LDS, for a gather kernel of gather_vgprs registers on ncu CUs; host only.  Returns (the block limit, the
    grid of a side-stream launch over rows_out rows, the grid of an inline one)."""
    lim, side, inline = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(lib().fpca_debug_gather_blocks(int(gemm_waves), int(gemm_vgprs), int(gemm_lds), int(gather_vgprs), int(ncu), int(rows_out),
                                         C.byref(lim), C.byref(side), C.byref(inline)))
    return lim.value, side.value, inline.value


def flashpca(X, ndim=10, stand="binom2", divisor="p", maxiter=500, tol=1e-6, do_loadings=False, return_scale=True,
             device=0, verbose=False, accum="auto", keep=None, snps=None, maf=0.0, geno=1.0, ld=None, unrelated=None,
             mind=1.0, hwe=0.0, unrelated_min_shared=0, **solver_kw):
    """PCA of a PLINK fileset; mirrors flashpca() of the reference's R package for the PLINK-prefix input
    (flashpcaR/R/flashpca.R:99-204 -> flashpca_plink_internal, flashpcaR/src/flashpca.cpp:96-197).

    X: PLINK root name (X.bed / X.bim / X.fam), or a numeric N x P matrix (NaN = missing; the R function's matrix
    input, flashpcaR/src/flashpca.cpp:17-93, which also accepts stand = "sd" / "center" / "none").
    keep: a boolean array with one entry per sample (PLINK input only): the PCA runs on the kept samples -- values, vectors,
    projection, loadings, center, scale and pve are what a run on the subset fileset returns, rows in input order -- and the result
    gains `projection_all` (N x ndim): the kept samples' rows of `projection`, everyone else projected onto the same PCs.
    snps: a boolean mask over the .bim rows or an array of unique row indices, e.g. from snp_filter(); maf / geno: PLINK's --maf /
    --geno on the uploaded matrix (minor-allele frequency >= maf, missing-call rate <= geno; both over all samples, so not together
    with keep=).  PLINK input only.  The selected SNPs are compacted once on the device and the PCA runs on them: loadings, center and
    scale have one row per kept SNP, divisor "p" is the kept count, and the result gains `snps_kept`, the mask over the .bim rows.
    ld: (window, step, r2) -- LD pruning in the style of PLINK's --indep-pairwise, windows and steps in SNPs, chromosomes from the .bim,
    applied to the survivors of snps / maf / geno (Context.ld_prune); r2 is over all samples, so not together with keep=.
    unrelated: a kinship threshold (0.0884: no pair closer than third degree).  PLINK input only.  After snps / maf / geno / ld -- which
    stay over all samples, the usual QC-then-KING order, and are allowed with it as long as keep is None -- Context.king_cutoff on the
    selected SNPs picks the samples (among those of keep=, if given), and the PCA runs on them as under keep=: the result gains
    `unrelated_kept`, the mask over the samples, and `projection_all`.  unrelated_min_shared: a pair that shares fewer called SNPs than
    this is no relative, whatever its coefficient (Context.king_cutoff_shared); 0, the default, is king_cutoff itself.
    mind / hwe: PLINK's --mind (missing-call rate per sample <= mind) and --hwe (Hardy-Weinberg exact-test p-value per SNP >= hwe; no
    mid-p).  PLINK input only.  With either of them the order is: the snps list; mind, whose rate is over the listed SNPs and all samples
    (among the samples of keep=, if given); geno / hwe / maf over the samples mind left (Context.snp_qc_samples); ld, whose r2 stays over
    all samples; unrelated among the samples left; the PCA on those samples as under keep=.  With mind the result gains `mind_kept`, the
    mask over the samples, and `projection_all`.  keep= goes with mind=, not with hwe= (nor maf / geno): for frequencies over a
    hand-picked subset of the samples take the masks from qc_filter(..., keep=) and pass them as snps= and keep=.
    Returns values, vectors, projection, loadings, center, scale, pve.
    """
    if divisor not in DIVISOR:
        raise ValueError("divisor must be one of %s" % sorted(DIVISOR))
    qc = not (maf <= 0 and geno >= 1)  # (a NaN threshold counts as a filter: fpca_snp_qc refuses it)
    by_mind, by_hwe = not mind >= 1, not hwe <= 0  # (a NaN threshold counts as a filter here too)
    if (snps is not None or qc) and not isinstance(X, str):
        raise ValueError("snps / maf / geno select SNPs of a PLINK fileset; they do not apply to a numeric matrix")
    if (by_mind or by_hwe) and not isinstance(X, str):
        raise ValueError("mind / hwe filter the samples / SNPs of a PLINK fileset; they do not apply to a numeric matrix")
    if qc and keep is not None:
        raise ValueError("maf / geno cannot be combined with keep: PLINK takes these frequencies over the kept samples, the counts here "
                         "are those of all samples")
    if by_hwe and keep is not None:
        raise ValueError("hwe cannot be combined with keep: flashpca() takes the genotype counts over the samples mind= leaves; for a "
                         "hand-picked subset take the masks from qc_filter(..., keep=) and pass them as snps= and keep=")
    if ld is not None:
        ld = _ld_args(ld)
        if not isinstance(X, str):
            raise ValueError("ld prunes the SNPs of a PLINK fileset; it does not apply to a numeric matrix")
        if keep is not None:
            raise ValueError("ld cannot be combined with keep: PLINK takes r2 over the kept samples, r2 here is over all samples")
    if unrelated is not None:
        unrelated = float(unrelated)
        if not isinstance(X, str):
            raise ValueError("unrelated selects samples by the kinship of a PLINK fileset's genotypes; it does not apply to a numeric matrix")
    if isinstance(X, str):
        if stand not in STANDARDISE:
            raise ValueError("stand must be one of %s" % sorted(STANDARDISE))  # R: match.arg
        N = count_fam_rows(X + ".fam")
        ctx = Context.from_bed(X + ".bed", N, stand=stand, device=device, accum=accum)
    else:
        if stand not in _lib.STANDARDISE_DENSE:
            raise ValueError("stand must be one of %s" % sorted(_lib.STANDARDISE_DENSE))
        ctx = Context.from_dense(np.asarray(X, dtype=np.float64), stand=stand, device=device)
    snps_kept = mind_kept = None
    if by_mind or by_hwe:
        select = snps is not None or qc or by_hwe or ld is not None
        full = ctx
        try:
            mind_kept, mask = _qc_masks(full, X, snps, mind, maf, geno, hwe, ld, keep)
            if not by_mind:
                mind_kept = None
            elif int(mind_kept.sum()) < 2:
                raise ValueError("mind = %g leaves %d of %d samples; at least 2 are needed" % (mind, int(mind_kept.sum()), full.N))
            else:
                keep = mind_kept
            if select:  # (mind alone drops no SNP: the PCA runs on the uploaded matrix itself)
                ctx, snps_kept = full.snp_subset(mask), mask
        except BaseException:
            full.close()
            raise
        if ctx is not full:
            full.close()
    elif snps is not None or qc or ld is not None:
        with ctx as full:  # (the source is closed on the way out)
            ctx, snps_kept = _select_snps(full, X, snps, qc, maf, geno, ld)
    with ctx:
        if keep is not None:
            keep = np.asarray(keep)
            if keep.shape != (ctx.N,):
                raise ValueError("keep must have one entry per sample (%d), it has shape %s" % (ctx.N, keep.shape))
            keep = keep != 0
        unrelated_kept = None
        if unrelated is not None:
            if unrelated_min_shared:
                keep = unrelated_kept = ctx.king_cutoff_shared(unrelated, unrelated_min_shared, keep=keep)
            else:
                keep = unrelated_kept = ctx.king_cutoff(unrelated, keep=keep)
        if keep is not None:
            ctx.set_sample_mask(keep)
        r = ctx.pca(ndim=ndim, tol=tol, maxiter=maxiter, div=divisor, do_loadings=do_loadings, verbose=int(verbose),
                    **solver_kw)
    res = dict(values=r["d"], vectors=r["U"], projection=r["Px"], loadings=r["V"], pve=r["pve"], info=r["info"])
    if keep is not None:
        res.update(vectors=r["U"][keep], projection=r["Px"][keep], projection_all=r["Px"])
    if unrelated_kept is not None:
        res["unrelated_kept"] = unrelated_kept
    if mind_kept is not None:
        res["mind_kept"] = mind_kept
    if snps_kept is not None:
        res["snps_kept"] = snps_kept
    if return_scale:
        res["center"] = r["meansd"][:, 0]
        res["scale"] = r["meansd"][:, 1]
    return res


_STAND_ORDER = ("binom2", "binom", "sd", "center", "none")  # R: match.arg's choices, first = default


def _match_arg(name, value):
    if value not in _STAND_ORDER:
        raise ValueError("'arg' should be one of %s" % ", ".join('"%s"' % m for m in _STAND_ORDER) + " (%s)" % name)
    return value


def _is_012(A):
    return bool(np.all(np.isin(A[~np.isnan(A)], (0.0, 1.0, 2.0))))


def ucca(X, Y, standx="binom2", standy="binom2", check_geno=True, check_fam=True, verbose=False, device=0, snps=None, ld=None):
    """Per-SNP canonical correlation (ANOVA of all phenotypes on each SNP, plink.multivariate); mirrors ucca() of the reference's R
    package (flashpcaR/R/ucca.R): same arguments and defaults, its stop() checks raised as ValueError with R's wording.

    X: PLINK root name (X.bed / X.bim / X.fam; standx binom or binom2), or a numeric N x P matrix (NaN = missing; any of the five
    standardisations).  Y: N x k phenotypes (NaN = missing, mean-imputed).
    snps (PLINK input only): a boolean mask over the .bim rows or an array of unique row indices, e.g. from snp_filter(); the scan
    runs on those SNPs, result and snp_ids have one row per kept SNP, and the mask comes back as snps_kept.
    ld (PLINK input only): (window, step, r2), LD pruning of those SNPs as in flashpca(ld=); snps_kept is the final mask.
    Returns result (P x 3: R, Fstat, P), npheno and, for the PLINK input, snp_ids in .bim order (ucca_plink_internal,
    flashpcaR/src/flashpca.cpp:275-334).
    """
    import warnings

    standx = _match_arg("standx", standx)
    standy = _match_arg("standy", standy)
    if snps is not None and not isinstance(X, str):
        raise ValueError("snps selects SNPs of a PLINK fileset; it does not apply to a numeric matrix")
    if ld is not None:
        ld = _ld_args(ld)
        if not isinstance(X, str):
            raise ValueError("ld prunes the SNPs of a PLINK fileset; it does not apply to a numeric matrix")
    try:
        Y = np.asarray(Y, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("Y must be a numeric matrix")
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)  # R: cbind(Y)
    if Y.ndim != 2:
        raise ValueError("Y must be a numeric matrix")
    if np.isnan(Y).any():
        warnings.warn("Y contains missing values, will be mean-imputed")
    if isinstance(X, str):
        if standx not in STANDARDISE:
            raise ValueError("When using PLINK data, you must use standx='binom' or 'binom2'")
        n = count_fam_rows(X + ".fam")
        if check_fam:
            if Y.shape[1] > n:
                raise ValueError("The phenotype matrix Y cannot have more columns than the sample size")
            if Y.shape[0] != n:
                raise ValueError("The number of rows in %s.fam and Y don't match" % X)
    else:
        try:
            X = np.asarray(X, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("X must be a numeric matrix or a string naming a PLINK fileset")
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2:
            raise ValueError("X must be a numeric matrix or a string naming a PLINK fileset")
        if np.isnan(X).any():
            warnings.warn("X contains missing values, will be mean-imputed")
        if Y.shape[1] > X.shape[0]:
            raise ValueError("The phenotype matrix Y cannot have more columns than the sample size")
        if Y.shape[0] != X.shape[0]:
            raise ValueError("The number of rows in X and Y don't match")
        if standx in STANDARDISE and check_geno and not _is_012(X):
            raise ValueError("Your X matrix contains values other than {0, 1, 2}, standx='binom'/'binom2' can't be used here")
    if standy in STANDARDISE and check_geno and not _is_012(Y):
        raise ValueError("Your Y matrix contains values other than {0, 1, 2}, standy='binom'/'binom2' can't be used here")
    if isinstance(X, str):
        ctx = Context.from_bed(X + ".bed", n, stand=standx, device=device, accum="auto")
    else:
        ctx = Context.from_dense(X, stand=standx, device=device)
    snps_kept = None
    if snps is not None or ld is not None:
        with ctx as full:
            ctx, snps_kept = _select_snps(full, X, snps, False, 0.0, 1.0, ld)
    with ctx:
        if verbose:
            print("UCCA online mode, N=%d p=%d" % (ctx.N, ctx.P))
        res = ctx.ucca(Y, standy=standy)
    out = dict(result=res, npheno=Y.shape[1])
    if isinstance(X, str):
        out["snp_ids"] = _read_bim(X)[0]
    if snps_kept is not None:
        out["snp_ids"] = [s for s, k in zip(out["snp_ids"], snps_kept) if k]
        out["snps_kept"] = snps_kept
    return out


def scca(X, Y, lambda1=0, lambda2=0, standx="binom2", standy="binom2", ndim=10, divisor="n1", maxiter=1000, tol=1e-4, seed=1,
         V=None, check_geno=True, check_fam=True, simplify=True, device=0, verbose=False):
    """Sparse canonical correlation analysis; mirrors scca() of the reference's R package (flashpcaR/R/scca.R:98-316): same
    arguments and defaults, its stop() checks raised as ValueError with R's wording.

    X: PLINK root name (standx binom or binom2), or a numeric N x P matrix (NaN = missing; any of the five standardisations).
    Y: N x k phenotypes (NaN = missing, mean-imputed).  lambda1 / lambda2: scalars or vectors of penalties.  V: k x ndim starting
    vectors; None takes R's warm start -- one fit at lambda1 = lambda2 = 1e-9 from a Gaussian matrix drawn from `seed` (numpy's
    generator, not the reference's), whose V starts every model.
    Returns the model (U, V, d, Px, Py, converged, iters, nzero_x, nzero_y, status) when both penalties are scalars and `simplify`,
    else the nested list res[i][j] of the models at lambda1[i], lambda2[j].  The genotypes are read once, whatever the grid.
    """
    import warnings

    standx = _match_arg("standx", standx)
    standy = _match_arg("standy", standy)
    if divisor not in ("n1", "none"):
        raise ValueError("'arg' should be one of \"n1\", \"none\" (divisor)")
    try:
        Y = np.asarray(Y, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("Y must be a numeric matrix")
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)  # R: cbind(Y)
    if Y.ndim != 2:
        raise ValueError("Y must be a numeric matrix")
    if np.isnan(Y).any():
        warnings.warn("Y cantains missing values, will be mean imputed")
    if isinstance(X, str):
        if standx not in STANDARDISE:
            raise ValueError("When using PLINK data, you must use standx='binom' or 'binom2'")
        n = count_fam_rows(X + ".fam")
        p = len(_read_bim(X)[0])
        if check_fam and Y.shape[0] != n:
            raise ValueError("The number of rows in %s.fam and Y don't match" % X)
    else:
        try:
            X = np.asarray(X, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("X must be a numeric matrix or a string naming a PLINK fileset")
        if X.ndim != 2:
            raise ValueError("X must be a numeric matrix or a string naming a PLINK fileset")
        if np.isnan(X).any():
            warnings.warn("X cantains missing values, will be mean imputed")
        if X.shape[1] < 2:
            raise ValueError("X must have at least two columns")
        if X.shape[0] < 2:
            raise ValueError("X must have at least two rows")
        if Y.shape[0] != X.shape[0]:
            raise ValueError("The number of rows in X and Y don't match")
        if standx in STANDARDISE and check_geno and not _is_012(X):
            raise ValueError("Your data contains values other than {0, 1, 2}, standx='binom'/'binom2' can't be used here")
        n, p = X.shape
    l1 = None if lambda1 is None else np.atleast_1d(np.asarray(lambda1, dtype=np.float64))
    l2 = None if lambda2 is None else np.atleast_1d(np.asarray(lambda2, dtype=np.float64))
    if l1 is None or np.any(l1 < 0):
        raise ValueError("lambda1 must be non-negative")
    if l2 is None or np.any(l2 < 0):
        raise ValueError("lambda2 must be non-negative")
    if ndim < 1:
        raise ValueError("ndim can't be less than 1")
    max_dim = min(p, n, Y.shape[1], Y.shape[0])
    if ndim > max_dim:
        raise ValueError("You asked for %d dimensions, but only %d allowed" % (ndim, max_dim))
    if V is not None:
        V = np.asarray(V, dtype=np.float64)
        if V.ndim == 1:
            V = V.reshape(-1, 1)  # R: cbind(V)
        if V.shape != (Y.shape[1], ndim):
            raise ValueError("dimensions of V must be (ncol(Y) x (ndim))")
    if isinstance(X, str):
        ctx = Context.from_bed(X + ".bed", n, stand=standx, device=device, accum="auto")
    else:
        ctx = Context.from_dense(X, stand=standx, device=device)
    with ctx:
        ctx.scca_prepare(Y, standy=standy, divisor=divisor)
        if V is None:
            if verbose:
                print("initialising V")
            V0 = np.random.default_rng(seed).standard_normal((Y.shape[1], ndim))
            V = ctx.scca_fit(1e-9, 1e-9, ndim, V0, maxiter=maxiter, tol=tol)["V"]
        res = [[ctx.scca_fit(a, b, ndim, V, maxiter=maxiter, tol=tol) for b in l2] for a in l1]
    if isinstance(X, str):
        ids = _read_bim(X)[0]
        for row in res:
            for m in row:
                m["snp_ids"] = ids  # R: rownames(s$U) <- bim$V2
    if simplify and len(l1) == 1 and len(l2) == 1:
        return res[0][0]
    return res


def pack_dosages(X):
    """A numeric N x P matrix of {0, 1, 2, NaN} -> PLINK's packed records (P x ceil(N / 4) bytes; codes 3, 2, 0 and 1 = missing)."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    codes = np.ones(((n + 3) // 4 * 4, p), dtype=np.uint8)  # missing
    codes[:n][X == 0] = 3
    codes[:n][X == 1] = 2
    codes[:n][X == 2] = 0
    codes[n:] = 0  # PLINK writes the pad bits as 0
    c = codes.T
    return np.ascontiguousarray(c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6))


def cv_scca(X, Y, lambda1=np.linspace(1e-6, 1e-3, 5), lambda2=np.linspace(1e-6, 1e-3, 5), ndim=3, nfolds=10, folds=None, opt_dim=1, init=True,
            standx="binom2", standy="binom2", divisor="n1", maxiter=1000, tol=1e-4, seed=1, device=0, verbose=False, return_pred=False):
    """Cross-validation of the SCCA penalties; mirrors cv.scca() of the reference's R package (flashpcaR/R/scca.R:410-557): same
    arguments and defaults, its stop() checks (and those of scca() that apply) raised as ValueError with R's wording before any
    device work.

    X: PLINK root name, or a numeric N x P matrix of {0, 1, 2, NaN}, which is packed on the host; standx binom or binom2 -- every fold
    standardises the genotypes on its training samples, which needs genotype input (R supports numeric matrices only and standardises
    the held-out rows with everything).  folds: ids 1 .. nfolds as in R (overrides nfolds); None draws them from `seed`, and each
    fold's starting matrix from the same generator.  init: R's warm start at 1e-12; False starts from scca()'s own at 1e-9.
    Returns R's fields (ndim, lambda1, lambda2, opt_dim, best_lambda1, best_lambda2, best_corr, corr, nzero_x, nzero_y, nfolds,
    converged) plus iters, warm_iters, folds and, with return_pred, xpred / ypred (N, ndim, n1, n2)."""
    import warnings

    standx = _match_arg("standx", standx)
    standy = _match_arg("standy", standy)
    if divisor not in ("n1", "none"):
        raise ValueError("'arg' should be one of \"n1\", \"none\" (divisor)")
    try:
        Y = np.asarray(Y, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("Y must be a numeric matrix")
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)  # R: cbind(Y)
    if Y.ndim != 2:
        raise ValueError("Y must be a numeric matrix")
    n = Y.shape[0]
    if nfolds > n:
        raise ValueError("nfolds is too large for the number of samples")
    if opt_dim <= 0 or opt_dim > ndim:
        raise ValueError("opt.dim must be between 1 and ndim")
    if not isinstance(init, (bool, np.bool_)):
        raise ValueError("init muct be TRUE or FALSE")
    if folds is not None:
        try:
            folds = np.asarray(folds).astype(np.int64).ravel()
        except (TypeError, ValueError):
            raise ValueError("'folds' must be a set of contiguous integers from 1 to nfolds")
        if folds.size != n:
            raise ValueError("'folds' must be of same number of rows as X and Y")
        if np.any(np.diff(np.sort(folds)) > 1) or folds.min() < 1:
            raise ValueError("'folds' must be a set of contiguous integers from 1 to nfolds")
        warnings.warn("'folds' will override 'nfolds' parameter")
        nfolds = int(folds.max())
    if np.isnan(Y).any():
        warnings.warn("Y cantains missing values, will be mean imputed")
    if standx not in STANDARDISE:
        raise ValueError("Cross-validation re-standardises the genotypes on every fold's training samples and needs genotype input: "
                         "standx must be 'binom' or 'binom2'")
    if isinstance(X, str):
        nx = count_fam_rows(X + ".fam")
        p = len(_read_bim(X)[0])
        if Y.shape[0] != nx:
            raise ValueError("The number of rows in %s.fam and Y don't match" % X)
    else:
        try:
            X = np.asarray(X, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("X must be a numeric matrix or a string naming a PLINK fileset")
        if X.ndim != 2:
            raise ValueError("X must be a numeric matrix or a string naming a PLINK fileset")
        if X.shape[1] < 2:
            raise ValueError("X must have at least two columns")
        if X.shape[0] < 2:
            raise ValueError("X must have at least two rows")
        if Y.shape[0] != X.shape[0]:
            raise ValueError("The number of rows in X and Y don't match")
        if not _is_012(X):
            raise ValueError("Your data contains values other than {0, 1, 2}; cross-validation re-standardises the genotypes on every "
                             "fold's training samples and needs genotype input")
        if np.isnan(X).any():
            warnings.warn("X cantains missing values, will be mean imputed")
        p = X.shape[1]
    if standy in STANDARDISE and not _is_012(Y):
        raise ValueError("Your data contains values other than {0, 1, 2}, standy='binom'/'binom2' can't be used here")
    l1 = None if lambda1 is None else np.atleast_1d(np.asarray(lambda1, dtype=np.float64))
    l2 = None if lambda2 is None else np.atleast_1d(np.asarray(lambda2, dtype=np.float64))
    if l1 is None or l1.size == 0 or not np.all(l1 >= 0):
        raise ValueError("lambda1 must be non-negative")
    if l2 is None or l2.size == 0 or not np.all(l2 >= 0):
        raise ValueError("lambda2 must be non-negative")
    if ndim < 1:
        raise ValueError("ndim can't be less than 1")
    rng = np.random.default_rng(seed)
    if folds is None:
        folds = rng.integers(1, nfolds + 1, n)
    if nfolds < 2 or nfolds > 64:
        raise ValueError("between 2 and 64 folds are supported, not %d" % nfolds)
    min_train = n - int(np.bincount(folds, minlength=nfolds + 1).max())
    max_dim = min(p, min_train, Y.shape[1])
    if ndim > max_dim:
        raise ValueError("You asked for %d dimensions, but only %d allowed" % (ndim, max_dim))
    V0 = rng.standard_normal((nfolds, Y.shape[1], ndim))  # scca.R:478: a fresh Gaussian matrix per fold
    if isinstance(X, str):
        ctx = Context.from_bed(X + ".bed", n, stand=standx, device=device, accum="auto")
    else:
        ctx = Context.from_packed(pack_dosages(X), n, p, stand=standx, device=device, accum="auto")
    with ctx:
        if verbose:
            print("cv.scca: N=%d p=%d, %d folds, %d x %d penalties" % (ctx.N, ctx.P, nfolds, l1.size, l2.size))
        r = ctx.scca_cv(Y, folds - 1, l1, l2, ndim, V0, standy=standy, divisor=divisor, maxiter=maxiter, tol=tol,
                        warm_lambda=1e-12 if init else 1e-9, opt_dim=opt_dim, return_pred=return_pred)
    r.update(ndim=ndim, lambda1=l1, lambda2=l2, opt_dim=opt_dim, nfolds=nfolds, folds=folds)
    return r


def _read_bim(prefix):
    rows = [l.split() for l in open(prefix + ".bim").read().splitlines() if l.strip()]
    return [r[1] for r in rows], [r[4] for r in rows]


def _first_fields(src):
    """SNP ids from an iterable of ids, or from a file in PLINK's --extract / --exclude format (the id is the first field of a line)."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        with open(src) as f:
            return {l.split()[0] for l in f if l.strip()}
    return {str(s) for s in src}


def _chrom(c):
    c = str(c)
    return c[3:] if c[:3].lower() == "chr" else c


def _ranges(src):
    """(chrom, first_bp, last_bp) triples from an iterable of them, or from a file of lines `chr start end [label]`."""
    if isinstance(src, (str, bytes)) or hasattr(src, "__fspath__"):
        with open(src) as f:
            src = [l.split()[:3] for l in f if l.strip()]
    out = []
    for r in src:
        if len(r) < 3:
            raise ValueError("a range is (chrom, first_bp, last_bp), found %r" % (r,))
        out.append((_chrom(r[0]), int(r[1]), int(r[2])))
    return out


def snp_filter(prefix, extract=None, exclude=None, extract_ranges=None, exclude_ranges=None):
    """A boolean mask over the rows of prefix.bim, for flashpca(snps=), ucca(snps=) and Context.snp_subset().

    extract / exclude: an iterable of SNP ids, or the path of a file in PLINK's format (the id is the first field of each line, blank
    lines are skipped, duplicates are harmless).  Ids that are not in the .bim are ignored, as PLINK does; an `extract` that matches
    nothing raises ValueError.  Every .bim row carrying a listed id is selected.
    extract_ranges / exclude_ranges: (chrom, first_bp, last_bp) triples, or the path of a file of lines `chr start end [label]` (the
    layout of the reference's exclusion_regions_hg19.txt).  Both ends are inclusive; chromosomes compare as strings after stripping a
    leading "chr" in either case.
    Order: extract, then extract_ranges, then exclude, then exclude_ranges."""
    rows = [l.split() for l in open(prefix + ".bim").read().splitlines() if l.strip()]
    chrom = np.array([_chrom(r[0]) for r in rows])
    ids = np.array([r[1] for r in rows])
    bp = np.array([int(r[3]) for r in rows], dtype=np.int64)

    def in_ranges(src):
        hit = np.zeros(len(rows), dtype=bool)
        for c, lo, hi in _ranges(src):
            hit |= (chrom == c) & (bp >= lo) & (bp <= hi)
        return hit

    mask = np.ones(len(rows), dtype=bool)
    if extract is not None:
        mask &= np.isin(ids, sorted(_first_fields(extract)))
        if not mask.any():
            raise ValueError("extract: none of the listed SNP ids is in %s.bim" % prefix)
    if extract_ranges is not None:
        mask &= in_ranges(extract_ranges)
    if exclude is not None:
        mask &= ~np.isin(ids, sorted(_first_fields(exclude)))
    if exclude_ranges is not None:
        mask &= ~in_ranges(exclude_ranges)
    return mask


def _ld_args(ld):
    try:
        w, s, t = ld
        w, s, t = int(w), int(s), float(t)
    except (TypeError, ValueError):
        raise ValueError("ld is (window, step, r2): two SNP counts and a threshold, found %r" % (ld,))
    return w, s, t


def _bim_chrom_codes(prefix):
    """One integer per .bim row, equal for equal chromosome fields: fpca_ld_prune's chromosomes are the runs of equal codes."""
    col = np.array([l.split()[0] for l in open(prefix + ".bim").read().splitlines() if l.strip()])
    return np.unique(col, return_inverse=True)[1].astype(np.uint32)


def _selection_mask(full, prefix, snps, qc, maf, geno, ld):
    """The SNP selection of flashpca() / ucca() / ld_prune() on the uploaded fileset `full`, as a mask over the .bim rows: list filter,
    QC filter, then LD pruning of the survivors."""
    mask = np.ones(full.P, dtype=bool) if snps is None else _snp_mask(snps, full.P)
    if qc:
        mask = full.snp_qc(maf=maf, geno=geno, keep=mask)
    return _ld_survivors(full, prefix, mask, ld, snps is None and not qc)


def _ld_survivors(full, prefix, mask, ld, untouched):
    """LD pruning (ld: (window, step, r2) or None) of the SNPs of `mask` on the uploaded fileset `full`; untouched: nothing was filtered
    before, the mask is all ones."""
    if ld is None:
        return mask
    chrom = _bim_chrom_codes(prefix)
    if chrom.shape != (full.P,):
        raise ValueError("%s.bim has %d rows, the .bed holds %d SNPs" % (prefix, chrom.size, full.P))
    if untouched:  # nothing filtered before: the windows count the fileset's own SNPs, no first compaction
        return full.ld_prune(*ld, chrom=chrom)
    # the windows count the survivors of the earlier filters, as in PLINK: prune on their compaction (gone again before the caller
    # compacts the final mask from the source: a gather of a gather is a gather)
    with full.snp_subset(mask, accum="fp64") as mid:
        kept = mid.ld_prune(*ld, chrom=chrom[mask])
    mask = mask.copy()
    mask[np.flatnonzero(mask)] = kept
    return mask


def _qc_masks(full, prefix, snps, mind, maf, geno, hwe, ld, keep):
    """(sample mask, SNP mask) of flashpca()'s QC order on the uploaded fileset `full`: the snps list; mind over the listed SNPs among the
    samples of keep; geno / hwe / maf over the samples left; LD pruning of the surviving SNPs, its r2 over all samples."""
    mask = np.ones(full.P, dtype=bool) if snps is None else _snp_mask(snps, full.P)
    samples = full.sample_qc(mind, snps=mask, keep=keep)  # (mind >= 1: keep itself, or everyone)
    if not (maf <= 0 and geno >= 1 and hwe <= 0):
        mask = full.snp_qc_samples(samples, maf=maf, geno=geno, hwe=hwe, keep=mask)
    return samples, _ld_survivors(full, prefix, mask, ld, False)


def qc_filter(prefix, mind=1.0, geno=1.0, hwe=0.0, maf=0.0, snps=None, keep=None, device=0):
    """The four QC filters the reference's README asks for before a PCA, on the GPU: (sample_mask, snp_mask), boolean masks over the rows of
    prefix.fam and prefix.bim, in the manner of `plink --mind mind --geno geno --hwe hwe --maf maf` and in flashpca()'s order: the snps
    list (a mask or an index array); mind, the missing-call rate per sample over the listed SNPs, among the samples of keep (a boolean
    array with one entry per sample; None: all); then geno, hwe and maf per SNP over the samples left.  Unlike flashpca(), keep= goes
    with every filter: qc_filter(..., keep=) followed by flashpca(prefix, snps=snp_mask, keep=sample_mask) is the route when the
    frequencies of a hand-picked subset of the samples are wanted.  hwe is the exact test without mid-p, over all the samples counted
    (no founders-only or controls-only counting); not byte-compatible with the plink binary."""
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        return _qc_masks(full, prefix, snps, mind, maf, geno, hwe, None, keep)


def _select_snps(full, prefix, snps, qc, maf, geno, ld):
    """(a new Context holding the selected SNPs of `full`, compacted once from it; the mask over the .bim rows).  `full` stays open."""
    mask = _selection_mask(full, prefix, snps, qc, maf, geno, ld)
    return full.snp_subset(mask), mask


def ld_prune(prefix, window=1000, step=50, r2=0.05, snps=None, maf=0.0, geno=1.0, device=0):
    """LD pruning of a PLINK fileset on the GPU, in the style of `plink --indep-pairwise window step r2` (windows and steps in SNPs):
    a boolean mask over the rows of prefix.bim.  snps / maf / geno as in flashpca(): they are applied first, and the windows count
    their survivors.  Not byte-compatible with the plink binary (its window refill and its MAF epsilon differ in detail)."""
    qc = not (maf <= 0 and geno >= 1)
    ld = _ld_args((window, step, r2))
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        return _selection_mask(full, prefix, snps, qc, maf, geno, ld)


def king_cutoff(prefix, thr=0.0884, snps=None, maf=0.0, geno=1.0, ld=None, keep=None, device=0):
    """The unrelated samples of a PLINK fileset, picked on the GPU in the manner of `plink2 --king-cutoff thr`: a boolean mask over the
    rows of prefix.fam in which no pair has KING-robust kinship above thr (Context.king_cutoff).  snps / maf / geno / ld as in flashpca():
    they are applied first, over all samples, and the kinship is that of the selected SNPs.  keep: a boolean array with one entry per
    sample; the cutoff runs among those.  Not byte-compatible with plink2 or KING (the order in which samples go differs)."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            return full.king_cutoff(thr, keep=keep)
        with _select_snps(full, prefix, snps, qc, maf, geno, ld)[0] as sub:
            return sub.king_cutoff(thr, keep=keep)


def king_classify(phi, counts, po_ibs0=0.005):
    """fpca_king_classify (host only): the uint8 type of every pair from phi[n] and counts[n][6] -- see Context.king_related."""
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    if phi.ndim != 1 or counts.shape != (phi.size, 6):
        raise ValueError("phi has one entry and counts six per pair; they have shapes %s and %s" % (phi.shape, counts.shape))
    out = np.empty(phi.size, dtype=np.uint8)
    check(lib().fpca_king_classify(phi.size, _p(phi), _p(counts), float(po_ibs0), _p(out)))
    return out


def _king_table(i, j, phi, counts, po_ibs0):
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ibs = 1.0 - (c[:, 5] - 2.0 * c[:, 1]) / (2.0 * c[:, 0])
    return dict(i=i, j=j, phi=phi, shared=counts[:, 0].copy(), ibs0=counts[:, 1].copy(), hethet=counts[:, 2].copy(), het_i=counts[:, 3].copy(),
                het_j=counts[:, 4].copy(), dist=counts[:, 5].copy(), ibs=ibs, type=king_classify(phi, counts, po_ibs0))


def king_related(prefix, thr=0.0442, min_shared=0, po_ibs0=0.005, snps=None, maf=0.0, geno=1.0, ld=None, keep=None, device=0):
    """The relationship table of a PLINK fileset (Context.king_related): every pair of rows i < j of prefix.fam with KING-robust kinship
    above thr (0.0442: third degree and closer) that shares at least min_shared called SNPs, with the shared-SNP count, IBS0, het-het,
    PLINK's IBS similarity and the inferred type (parent-offspring apart from full sibs by ibs0 / shared < po_ibs0).  snps / maf / geno /
    ld as in king_cutoff(): applied first, over all samples.  keep: a boolean array with one entry per sample.  write_kin0() writes the
    table in KING's .kin0 format.  Not byte-compatible with the KING binary."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            return full.king_related(thr, keep=keep, min_shared=min_shared, po_ibs0=po_ibs0)
        with _select_snps(full, prefix, snps, qc, maf, geno, ld)[0] as sub:
            return sub.king_related(thr, keep=keep, min_shared=min_shared, po_ibs0=po_ibs0)


def write_kin0(path, prefix, table):
    """Write a king_related() table as KING's .kin0: a header and one tab-separated line per pair, FID1 ID1 FID2 ID2 N_SNP HetHet IBS0
    Kinship -- family and individual IDs from the first two columns of prefix.fam, N_SNP = shared, HetHet and IBS0 as proportions of
    N_SNP.  The three real columns are printed with %.17g, so they read back to the same doubles."""
    ids = []
    with open(prefix + ".fam") as f:
        for line in f:
            w = line.split()
            if w:
                ids.append((w[0], w[1]))
    with open(path, "w") as f:
        f.write("FID1\tID1\tFID2\tID2\tN_SNP\tHetHet\tIBS0\tKinship\n")
        for i, j, n, hh, z, phi in zip(table["i"], table["j"], table["shared"], table["hethet"], table["ibs0"], table["phi"]):
            i, j, n = int(i), int(j), int(n)
            if max(i, j) >= len(ids):
                raise ValueError("the table names sample %d; %s.fam has %d rows" % (max(i, j), prefix, len(ids)))
            f.write("%s\t%s\t%s\t%s\t%d\t%.17g\t%.17g\t%.17g\n" % (ids[i] + ids[j] + (n, float(hh) / n if n else float("nan"),
                                                                                float(z) / n if n else float("nan"), float(phi))))


GRM_DIVISOR = {"shared": 0, "p": 1, "none": 2}  # FPCA_GRM_DIV_*


def _grm_divisor(divisor):
    if isinstance(divisor, str):
        if divisor not in GRM_DIVISOR:
            raise ValueError("divisor must be one of %s" % sorted(GRM_DIVISOR))
        return GRM_DIVISOR[divisor]
    return int(divisor)  # (a number goes to the library as it is: its refusal names the three values)


def _fam_ids(prefix):
    ids = []
    with open(prefix + ".fam") as f:
        for line in f:
            w = line.split()
            if w:
                ids.append((w[0], w[1]))
    return ids


def grm(prefix, divisor="shared", snps=None, maf=0.0, geno=1.0, ld=None, device=0):
    """The genetic relationship matrix of a PLINK fileset (Context.grm_tri): a dict with `tri`, the packed lower triangle with the diagonal
    (entry i (i + 1) / 2 + j, j <= i, over the rows of prefix.fam), `shared`, the SNPs called in both samples in the same order, and `ids`,
    the (FID, IID) pairs -- what write_grm() takes.  Genotypes standardised as in flashpca() (binom2: the GRM of GCTA); snps / maf / geno /
    ld as in king_cutoff(): applied first, over all samples, and the frequencies are those of the selected SNPs over all samples."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            tri, shared = full.grm_tri(divisor, counts=True)
        else:
            with _select_snps(full, prefix, snps, qc, maf, geno, ld)[0] as sub:
                tri, shared = sub.grm_tri(divisor, counts=True)
    return dict(tri=tri, shared=shared, ids=_fam_ids(prefix))


def pcrelate(prefix, pcs, train=None, eps=0.01, snps=None, maf=0.0, geno=1.0, ld=None, device=0):
    """PC-Relate kinship of a PLINK fileset (Context.pcrelate_tri): a dict with `tri`, the packed lower triangle with the diagonal (entry
    i (i + 1) / 2 + j, j <= i, over the rows of prefix.fam), `den`, the denominator sums in the same order, `inbreeding` (2 x the diagonal -
    1), `beta`, the per-SNP coefficients on [1 | pcs] over the selected SNPs, and `ids`, the (FID, IID) pairs.  pcs: one row per sample --
    flashpca(unrelated=...)["projection_all"][:, :k]; train: the samples the regression is fitted on -- its "unrelated_kept".  snps / maf /
    geno / ld as in grm(): applied first, over all samples."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")

    def run(ctx):
        beta = ctx.pcrelate_beta(pcs, train=train)
        tri, den = ctx.pcrelate_tri(pcs, eps=eps, beta=beta, den=True)
        return tri, den, beta

    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            tri, den, beta = run(full)
        else:
            with _select_snps(full, prefix, snps, qc, maf, geno, ld)[0] as sub:
                tri, den, beta = run(sub)
    diag = tri[np.arange(N) * (np.arange(N) + 3) // 2]
    return dict(tri=tri, den=den, inbreeding=2.0 * diag - 1.0, beta=beta, ids=_fam_ids(prefix))


def pcrelate_classify(kin, k0, k2, nsnp, k0_switch=2 ** -5.5, po_k0=0.1):
    """fpca_pcrelate_classify (host only): (k0_out, k1_out, type) of every pair from its PC-Relate kinship, the IBS0 form of k0, k2 and the
    shared-SNP count: k0_out = k0 where kin > k0_switch, else 1 - 4 kin + k2; k1_out = 1 - k0_out - k2; type: king_classify's codes at KING's
    cut points on kin, parent-offspring (1) apart from full sibs (2) by k0_out < po_k0.  Both thresholds are conventions."""
    kin = np.ascontiguousarray(kin, dtype=np.float64)
    k0 = np.ascontiguousarray(k0, dtype=np.float64)
    k2 = np.ascontiguousarray(k2, dtype=np.float64)
    nsnp = np.ascontiguousarray(nsnp, dtype=np.uint32)
    if kin.ndim != 1 or not (k0.shape == k2.shape == nsnp.shape == kin.shape):
        raise ValueError("kin, k0, k2 and nsnp have one entry per pair; they have shapes %s, %s, %s and %s" % (kin.shape, k0.shape, k2.shape, nsnp.shape))
    k0_out, k1_out, typ = np.empty(kin.size), np.empty(kin.size), np.empty(kin.size, dtype=np.uint8)
    check(lib().fpca_pcrelate_classify(kin.size, _p(kin), _p(k0), _p(k2), _p(nsnp), float(k0_switch), float(po_k0), _p(k0_out), _p(k1_out), _p(typ)))
    return k0_out, k1_out, typ


def pcrelate_ibd(prefix, pcs, train=None, eps=0.01, k0_switch=2 ** -5.5, snps=None, maf=0.0, geno=1.0, ld=None, device=0):
    """PC-Relate kinship and IBD sharing of a PLINK fileset: what pcrelate() returns (`tri`, `den`, `inbreeding`, `beta`, `ids`) and the
    packed lower triangles `k0`, `k1`, `k2` (the probabilities of sharing 0, 1, 2 alleles identical by descent) and `nsnp` (the SNPs usable
    in both samples), entry i (i + 1) / 2 + j.  beta is estimated once; f of the k2 correction is `inbreeding`; k0 is the IBS0 form where
    the kinship is above k0_switch and 1 - 4 kin + k2 elsewhere (pcrelate_classify).  The diagonal of the four carries no meaning."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")

    def run(ctx):
        beta = ctx.pcrelate_beta(pcs, train=train)
        tri, den = ctx.pcrelate_tri(pcs, eps=eps, beta=beta, den=True)
        f = 2.0 * tri[np.arange(N) * (np.arange(N) + 3) // 2] - 1.0
        # (a sample without a usable SNP has a NaN diagonal; its k2 is NaN whatever f is, and the library refuses a non-finite f)
        return tri, den, beta, f, ctx.pcrelate_ibd_tri(pcs, f=np.nan_to_num(f), eps=eps, beta=beta)

    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            tri, den, beta, f, ibd = run(full)
        else:
            with _select_snps(full, prefix, snps, qc, maf, geno, ld)[0] as sub:
                tri, den, beta, f, ibd = run(sub)
    k0, k1, _ = pcrelate_classify(tri, ibd["k0"], ibd["k2"], ibd["nsnp"], k0_switch=k0_switch)
    return dict(tri=tri, den=den, inbreeding=f, beta=beta, ids=_fam_ids(prefix), k0=k0, k1=k1, k2=ibd["k2"], nsnp=ibd["nsnp"])


def pcrelate_related(prefix, pcs, train=None, thr=2 ** -5.5, min_snps=0, po_k0=0.1, eps=0.01, k0_switch=2 ** -5.5, snps=None, maf=0.0, geno=1.0,
                     ld=None, device=0):
    """The PC-Relate relationship table of a PLINK fileset: every pair of rows i < j of prefix.fam with PC-Relate kinship above thr (2^-5.5:
    third degree and closer) and at least min_snps SNPs usable in both, sorted by (i, j) -- a dict of the columns `i`, `j`, `kin`, `k0`,
    `k1`, `k2`, `nsnp`, `type` (pcrelate_classify: parent-offspring apart from full sibs by k0 < po_k0).  Built on the host from
    pcrelate_ibd()'s triangles; the other arguments are its."""
    r = pcrelate_ibd(prefix, pcs, train=train, eps=eps, k0_switch=k0_switch, snps=snps, maf=maf, geno=geno, ld=ld, device=device)
    N = len(r["inbreeding"])
    i, j = np.tril_indices(N, -1)  # (row-major over the strict lower triangle: sorted by (larger, smaller))
    at = i * (i + 1) // 2 + j
    with np.errstate(invalid="ignore"):
        sel = (r["tri"][at] > thr) & (r["nsnp"][at] >= min_snps)
    lo, hi, at = j[sel].astype(np.uint32), i[sel].astype(np.uint32), at[sel]
    order = np.lexsort((hi, lo))
    lo, hi, at = lo[order], hi[order], at[order]
    kin, k2, nsnp = r["tri"][at], r["k2"][at], r["nsnp"][at]
    # (k0 of the triangle is already the chosen estimator: a switch below every kinship hands it through)
    k0, k1, typ = pcrelate_classify(kin, r["k0"][at], k2, nsnp, k0_switch=-np.finfo(np.float64).max, po_k0=po_k0)
    return dict(i=lo, j=hi, kin=kin, k0=k0, k1=k1, k2=k2, nsnp=nsnp, type=typ)


def pcair_partition_rule(N, i, j, kin, n_div, keep=None):
    """fpca_pcair_partition (host only): PC-AiR's partition rule on caller arrays -- the boolean mask of the samples left when, among those
    of `keep` (None: all N), one sample at a time goes until no listed pair (i[k], j[k]) remains: the one in most pairs; among equals the
    one of smallest n_div; among equals the one whose kin over its remaining pairs sums lowest (fp64, in ascending order of the partner's
    index); among equals the largest index.  Repeated and reversed pairs count once, with the first kin listed."""
    N = int(N)
    pi, pj, kin = _kin_pairs((i, j, kin))
    n_div = np.ascontiguousarray(n_div, dtype=np.uint32)
    if n_div.shape != (N,):
        raise ValueError("n_div must have one entry per sample (%d), it has shape %s" % (N, n_div.shape))
    if keep is None:
        k8 = np.ones(N, dtype=np.uint8)
    else:
        keep = np.asarray(keep)
        if keep.shape != (N,):
            raise ValueError("keep must have one entry per sample (%d), it has shape %s" % (N, keep.shape))
        k8 = np.ascontiguousarray(keep != 0, dtype=np.uint8)
    n = C.c_uint64(0)
    check(lib().fpca_pcair_partition(N, pi.size, _p(pi), _p(pj), _p(kin), _p(n_div), _p(k8), C.byref(n)))
    out = k8 != 0
    assert int(out.sum()) == n.value
    return out


def _pcair_partition(prefix, kin_thr, div_thr, snps, maf, geno, ld, keep, kin_pairs, device):
    """(mask, n_rel, n_div, the SNP mask over the .bim rows) of Context.pcair_partition on the selected SNPs of a PLINK fileset."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            return full.pcair_partition(kin_thr, div_thr, keep=keep, kin_pairs=kin_pairs, counts=True) + (np.ones(full.P, dtype=bool),)
        sub, mask = _select_snps(full, prefix, snps, qc, maf, geno, ld)
        with sub:
            return sub.pcair_partition(kin_thr, div_thr, keep=keep, kin_pairs=kin_pairs, counts=True) + (mask,)


def pcair_partition(prefix, kin_thr=2 ** -5.5, div_thr=-2 ** -5.5, snps=None, maf=0.0, geno=1.0, ld=None, keep=None, kin_pairs=None, device=0):
    """PC-AiR's unrelated set of a PLINK fileset (Context.pcair_partition): a boolean mask over the rows of prefix.fam in which no pair is
    related -- KING-robust kinship above kin_thr, or, with kin_pairs=(i, j, kin), one of the listed pairs -- chosen so that of two
    relatives the one with more partners of divergent ancestry (kinship below div_thr) stays.  snps / maf / geno / ld as in king_cutoff():
    they are applied first, over all samples.  keep: a boolean array with one entry per sample; the partition runs among those.
    GENESIS::pcairPartition in structure; parity with GENESIS is not claimed."""
    return _pcair_partition(prefix, kin_thr, div_thr, snps, maf, geno, ld, keep, kin_pairs, device)[0]


def pcair(prefix, ndim=10, kin_thr=2 ** -5.5, div_thr=-2 ** -5.5, iterations=1, relate_pcs=None, eps=0.01, snps=None, maf=0.0, geno=1.0,
          ld=None, keep=None, device=0, **flashpca_kw):
    """PC-AiR (Conomos, Miller & Thornton 2015) of a PLINK fileset: PCs that describe ancestry and not family structure.  snps / maf / geno
    / ld select the SNPs (over all samples, as in king_cutoff()); pcair_partition() on them picks the unrelated set, among the samples of
    keep if given; the PCA runs on the unrelated samples and everyone else is projected -- exactly flashpca(prefix, ndim=ndim,
    snps=<snps_kept>, keep=<the mask>, **flashpca_kw), whose dict is returned with `unrelated_kept`, `n_rel`, `n_div` (the census the
    partition saw) and `snps_kept` added; `projection_all` holds every sample's PCs.
    iterations=2 adds GENESIS's second round: pcrelate_related() on the same SNPs with pcs = projection_all[:, :relate_pcs] (relate_pcs:
    min(ndim, 4) by default), train = the first mask, thr = kin_thr and eps; its pairs are the relatives of a second partition
    (kin_pairs=) and a second PCA.  The result is the second round's -- n_rel then counts the PC-Relate pairs per sample -- with the first
    mask kept as `unrelated_kept_1`.  Not claimed: parity with GENESIS::pcair."""
    if iterations not in (1, 2):
        raise ValueError("iterations is 1 (the KING partition) or 2 (a second round on PC-Relate kinship), found %r" % (iterations,))
    if not isinstance(prefix, str):
        raise ValueError("pcair() takes a PLINK fileset; the partition is made from its packed genotypes, not from a numeric matrix")
    for name in ("keep", "snps", "maf", "geno", "ld", "unrelated", "mind", "hwe", "unrelated_min_shared"):
        if name in flashpca_kw:
            raise ValueError("%s is not passed on to flashpca() by pcair()" % name)
    ndim = int(ndim)
    relate_pcs = min(ndim, 4) if relate_pcs is None else int(relate_pcs)
    if iterations == 2 and not 0 <= relate_pcs <= ndim:
        raise ValueError("relate_pcs is between 0 and ndim (%d), found %d" % (ndim, relate_pcs))
    unrel, n_rel, n_div, snps_kept = _pcair_partition(prefix, kin_thr, div_thr, snps, maf, geno, ld, keep, None, device)
    r = flashpca(prefix, ndim=ndim, snps=snps_kept, keep=unrel, device=device, **flashpca_kw)
    first = None
    if iterations == 2:
        first = unrel
        t = pcrelate_related(prefix, r["projection_all"][:, :relate_pcs], train=first, thr=kin_thr, eps=eps, snps=snps_kept, device=device)
        unrel, _, n_div, _ = _pcair_partition(prefix, kin_thr, div_thr, snps_kept, 0.0, 1.0, None, keep, (t["i"], t["j"], t["kin"]), device)
        among = np.ones(unrel.size, dtype=bool) if keep is None else np.asarray(keep) != 0
        both = among[t["i"]] & among[t["j"]]
        n_rel = (np.bincount(t["i"][both], minlength=unrel.size) + np.bincount(t["j"][both], minlength=unrel.size)).astype(np.uint32)
        r = flashpca(prefix, ndim=ndim, snps=snps_kept, keep=unrel, device=device, **flashpca_kw)
    r.update(unrelated_kept=unrel, n_rel=n_rel, n_div=n_div, snps_kept=snps_kept)
    if first is not None:
        r["unrelated_kept_1"] = first
    return r


def rel_cutoff(prefix, thr=0.025, divisor="shared", snps=None, maf=0.0, geno=1.0, ld=None, keep=None, device=0):
    """The unrelated samples of a PLINK fileset by the relationship matrix, in the manner of `plink --rel-cutoff thr` / `gcta --grm-cutoff
    thr`: a boolean mask over the rows of prefix.fam in which no pair has G above thr (Context.grm_cutoff), to pass to flashpca(keep=).
    snps / maf / geno / ld as in king_cutoff().  keep: a boolean array with one entry per sample; the cutoff runs among those (the
    frequencies stay those of all samples).  Not byte-compatible with plink or gcta (the order in which samples go differs)."""
    qc = not (maf <= 0 and geno >= 1)
    if ld is not None:
        ld = _ld_args(ld)
    N = count_fam_rows(prefix + ".fam")
    with Context.from_bed(prefix + ".bed", N, device=device, accum="fp64") as full:
        if snps is None and not qc and ld is None:
            return full.grm_cutoff(thr, keep=keep, divisor=divisor)
        with _select_snps(full, prefix, snps, qc, maf, geno, ld)[0] as sub:
            return sub.grm_cutoff(thr, keep=keep, divisor=divisor)


def write_grm(path, ids, tri, shared):
    """Write a relationship matrix in GCTA's binary format: path.grm.bin (float32, the packed lower triangle with the diagonal, row by
    row), path.grm.N.bin (float32, the shared-SNP counts in the same order) and path.grm.id (one `FID<tab>IID` line per sample).  ids:
    (FID, IID) pairs; tri and shared: N (N + 1) / 2 entries each, as grm() returns them."""
    ids = [tuple(x) for x in ids]
    n = len(ids)
    tri = np.asarray(tri)
    shared = np.asarray(shared)
    if tri.shape != (n * (n + 1) // 2,) or shared.shape != tri.shape:
        raise ValueError("%d samples have a triangle of %d entries; tri and shared have shapes %s and %s"
                         % (n, n * (n + 1) // 2, tri.shape, shared.shape))
    if any(len(x) != 2 for x in ids):
        raise ValueError("ids holds one (FID, IID) pair per sample")
    tri.astype("<f4").tofile(path + ".grm.bin")
    shared.astype("<f4").tofile(path + ".grm.N.bin")
    with open(path + ".grm.id", "w") as f:
        for fid, iid in ids:
            f.write("%s\t%s\n" % (fid, iid))


def read_grm(path):
    """Read path.grm.bin / .grm.N.bin / .grm.id (GCTA's binary format) back: a dict `tri` (float32), `shared` (float32), `ids`."""
    ids = []
    with open(path + ".grm.id") as f:
        for line in f:
            w = line.rstrip("\n").split("\t") if "\t" in line else line.split()
            if w and w != [""]:
                ids.append((w[0], w[1]))
    n = len(ids)
    tri = np.fromfile(path + ".grm.bin", dtype="<f4")
    shared = np.fromfile(path + ".grm.N.bin", dtype="<f4")
    if tri.shape != (n * (n + 1) // 2,) or shared.shape != tri.shape:
        raise ValueError("%s.grm.id names %d samples: a triangle of %d entries; .grm.bin holds %d and .grm.N.bin %d"
                         % (path, n, n * (n + 1) // 2, tri.size, shared.size))
    return dict(tri=tri, shared=shared, ids=ids)


def project(X, loadings, orig_mean=None, orig_sd=None, ref_alleles=None, divisor="p", device=0, check_bim=True):
    """Project samples onto existing principal components; mirrors project() of the reference's R package
    (flashpcaR/R/project.R:56-163): same arguments, same input checks (raised as ValueError), same result
    `{"projection": Z V / sqrt(div)}` with Z standardised by orig_mean / orig_sd and missing -> 0.

    X: PLINK root name, or a numeric N x P matrix (NaN = missing).  ref_alleles: mapping SNP name -> reference allele in
    .bim order (the R function's named character vector); required for the PLINK input unless check_bim=False.
    """
    if divisor not in DIVISOR:
        raise ValueError("divisor must be one of %s" % sorted(DIVISOR))
    if orig_mean is None:
        raise ValueError("The vector of means used for standardising the data must be provided via 'orig_mean'")
    if orig_sd is None:
        raise ValueError("The vector of standard deviations used for standardising the data must be provided via 'orig_sd'")
    loadings = np.asarray(loadings, dtype=np.float64)
    orig_mean = np.asarray(orig_mean, dtype=np.float64).ravel()
    orig_sd = np.asarray(orig_sd, dtype=np.float64).ravel()
    if isinstance(X, str):
        snp, ref = _read_bim(X)
        p = len(snp)
        if check_bim:
            if loadings.ndim != 2 or loadings.shape[0] != p:
                raise ValueError("The number of rows in %s.bim and the number of columns in the loadings don't match" % X)
            if ref_alleles is None or list(ref_alleles.keys()) != snp:
                raise ValueError("The SNP names in %s.bim do not match the names of the ref_alleles vector" % X)
            if list(ref_alleles.values()) != ref:
                raise ValueError("The reference alleles in %s.bim do not match the ref_alleles vector" % X)
            if orig_mean.size != p:
                raise ValueError("The number of rows in %s.bim and the length of orig_mean don't match" % X)
            if orig_sd.size != p:
                raise ValueError("The number of rows in %s.bim and the length of orig_sd don't match" % X)
            if np.any(orig_sd <= 0):
                raise ValueError("orig_sd cannot be zero or negative")
        n = count_fam_rows(X + ".fam")
        ctx = Context.from_bed(X + ".bed", n, device=device, accum="auto")
        with ctx:
            ctx.set_meansd(np.column_stack([orig_mean, orig_sd]))
            Z = ctx.apply_x(np.asfortranarray(loadings))
    else:
        Xm = np.asarray(X, dtype=np.float64)
        if loadings.ndim != 2 or loadings.shape[0] != Xm.shape[1]:
            raise ValueError("The number of rows in X and number of columns of the loadings don't match")
        if orig_mean.size != Xm.shape[1]:
            raise ValueError("The number of rows in X and length of orig_mean don't match")
        if orig_sd.size != Xm.shape[1]:
            raise ValueError("The number of rows in X and length of orig_sd don't match")
        if np.any(orig_sd <= 0):
            raise ValueError("orig_sd cannot be zero or negative")
        if np.isnan(Xm).any():
            import warnings

            warnings.warn("X contains missing values, will be mean imputed")
        n = Xm.shape[0]
        S = (Xm - orig_mean) / orig_sd  # R: scale(X, center, scale); the product itself runs on the GPU
        S[np.isnan(S)] = 0.0
        with Context.from_dense(S, stand="none", device=device) as ctx:
            Z = ctx.apply_x(np.asfortranarray(loadings))
    div_val = {"p": loadings.shape[0], "n1": n, "none": 1}[divisor]  # project.R:137-142 (as written there)
    return dict(projection=Z / np.sqrt(div_val))


def check_pca(X, evec, eval, stand="binom2", divisor="p", device=0, check_fam=True):  # noqa: A002 (R's argument name)
    """Check the accuracy of an eigen-decomposition; mirrors check() of the reference's R package
    (flashpcaR/R/check.R): err_j = || X X' u_j / div - d_j u_j ||^2, mse, rmse (RandomPCA::check, randompca.cpp:663-703)."""
    if divisor not in DIVISOR:
        raise ValueError("divisor must be one of %s" % sorted(DIVISOR))
    evec = np.asarray(evec, dtype=np.float64)
    evals = np.asarray(eval, dtype=np.float64).ravel()
    if isinstance(X, str):
        if stand not in STANDARDISE:
            raise ValueError("When using PLINK data, you must use stand='binom' or 'binom2'")
        n = count_fam_rows(X + ".fam")
        if check_fam and n != evec.shape[0]:
            raise ValueError("The number of rows in %s.fam and evec don't match" % X)
        ctx = Context.from_bed(X + ".bed", n, stand=stand, device=device, accum="auto")
    else:
        Xm = np.asarray(X, dtype=np.float64)
        if stand not in _lib.STANDARDISE_DENSE:
            raise ValueError("stand must be one of %s" % sorted(_lib.STANDARDISE_DENSE))
        if stand in ("binom", "binom2") and not np.all(np.isin(Xm[~np.isnan(Xm)], (0.0, 1.0, 2.0))):
            raise ValueError("Your data contains values other than {0, 1, 2}, stand='binom'/'binom2' can't be used here")
        if evec.shape[0] != Xm.shape[0]:
            raise ValueError("The number of rows in X and evec don't match")
        ctx = Context.from_dense(Xm, stand=stand, device=device)
    if evec.ndim != 2 or evec.shape[1] != evals.size:
        ctx.close()
        raise ValueError("The number of columns of evec doesn't match the number of eigenvalues eval")
    with ctx:
        err, mse, rmse = ctx.check(evec, evals, div=divisor)
    return dict(err=err, mse=mse, rmse=rmse)
