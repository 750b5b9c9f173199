/*
 * include/fpca.h -- C ABI of the MI355X-native flashpca PCA hot path (libfpca.so).
 *
 * The reference (gabraham/flashpca 2.1) has no C ABI of its own on this path; its seams are
 *   (1) the Spectra operator concept implemented by SVDWideOnline:
 *          unsigned rows(); unsigned cols(); void perform_op(const double* x_in, double* y_out);
 *                                                                    (svdwide.h:77-81, svdwide.cpp:21-68)
 *   (2) the C++ driver  RandomPCA::pca_fast(Data&, block_size, ndim, maxiter, tol, seed, do_loadings)
 *          with inputs  stand_method_x / divisor and outputs U, d, V, Px, pve, trace, X_meansd
 *                                                                    (randompca.h:56-80, randompca.cpp:168-218)
 *   (3) the data object  Data::{get_size, prepare, read_snp_block}   (data.h:60-101, data.cpp:150-335)
 * Every entry point below names the reference interface it replaces.  Conventions:
 *   - plain pointers and sizes only; no C++/torch types;
 *   - host matrices are fp64 COLUMN-major with an explicit leading dimension (what Eigen::MatrixXd /
 *     Map<VectorXd> hand to the reference operator);
 *   - functions return 0 on success, a negative FPCA_E* code on failure; fpca_last_error() returns the
 *     message of the last failure on the calling thread (the reference throws std::runtime_error,
 *     flashpca.cpp:882-892 turns that into EXIT_FAILURE);
 *   - a context owns ONE SNP shard [snp_begin, snp_begin+P_g) of the genotype matrix on ONE GPU:
 *     packed 2-bit stream resident in HBM, per-SNP mean/sd/lookup table, workspaces and a HIP stream.
 *     Multi-GPU = one context per process per GPU; the N x b product is summed across ranks either by
 *     RCCL inside the library (fpca_comm_init_rank) or by a caller-supplied all-reduce (fpca_set_allreduce);
 *   - there is NO CPU fallback: fpca_create* fail with FPCA_ENODEVICE when no gfx950 device is usable.
 */
#ifndef FPCA_H
#define FPCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPCA_VERSION "0.3.0"
/* Binary interface revision: bumped whenever a struct below changes size or a field changes meaning.  A binding checks
 * fpca_abi_version() == FPCA_ABI_VERSION once after loading the library (flashpca_amd/_lib.py does).
 *   2 (library 0.2.0): fpca_pca_opts / fpca_pca_info carry their own size and the mixed-precision fields; `maxiter` counts the
 *     reference's restarts (it was a cap on block applies in 0.1.0 -- use max_applies for that).
 *   3 (library 0.3.0): fpca_pca_opts.partial_rows, fpca_pca_info.solver_path; the struct sizes are the CALLER's
 *     (FPCA_PCA_OPTS_INIT / fpca_pca_init_opts); fpca_pca_row_ranges. */
#define FPCA_ABI_VERSION 4

/* standardisation methods: same numeric values as the reference (util.h:34-38); the packed-genotype constructors
 * accept BINOM / BINOM2 like the CLI (flashpca.cpp:336-349), fpca_create_dense accepts all five */
#define FPCA_STANDARDISE_NONE 0
#define FPCA_STANDARDISE_SD 1
#define FPCA_STANDARDISE_BINOM 2
#define FPCA_STANDARDISE_BINOM2 3
#define FPCA_STANDARDISE_CENTER 4
/* eigenvalue divisor: same numeric values as the reference (randompca.h:41-43) */
#define FPCA_DIVISOR_NONE 0
#define FPCA_DIVISOR_N1 1
#define FPCA_DIVISOR_P 2
/* arithmetic of the two genotype GEMMs.  AUTO = the exact-integer path FPCA_ACCUM_I8(7) for 2-bit input, FP64 for dense input.  If
 * the second, sample-major 2-bit copy the integer X T needs does not fit in device memory, AUTO keeps X'B on the int8 cores and runs
 * X T on the FP64 kernel (same results; 30 instead of 11 ms per 16-column pass at 500,000 x 100,000); if the int8 operands do not
 * fit either, both stages run FP64 (47 ms) */
#define FPCA_ACCUM_AUTO 0
#define FPCA_ACCUM_FP64 64
#define FPCA_ACCUM_FP32 32
/* exact-integer mode: the fp64 operand is rounded to (8S-2)-bit fixed point (shared power-of-two scale per column), cut
 * into its S bytes and multiplied with the integer genotype matrices on the int8 matrix cores with exact int32
 * accumulation; S = 7 keeps 54 bits below the column maximum (fp64-equivalent, the default), S = 4 (30 bits) roughly
 * single precision but still without accumulation error.  S = 2..8. */
#define FPCA_ACCUM_I8(S) (800 + (S))

#define FPCA_OK 0
#define FPCA_EINVAL -1      /* bad argument */
#define FPCA_ENODEVICE -2   /* no usable gfx950 device / HIP runtime error at init */
#define FPCA_EHIP -3        /* HIP runtime or kernel failure */
#define FPCA_ENOMEM -4      /* host or device allocation failed */
#define FPCA_ENOTCONVERGED -5 /* eigensolver hit maxiter (reference: "Spectra eigen-decomposition was not successful", randompca.cpp:212-217) */
#define FPCA_ECOMM -6       /* RCCL / all-reduce failure */
#define FPCA_EIO -7         /* file error (reference: "[Data::read_bed] Error reading file", data.cpp:156-161) */

typedef struct fpca_ctx fpca_ctx;

const char *fpca_last_error(void);
const char *fpca_version(void);
int fpca_abi_version(void);
/* number of visible HIP devices (<0 on error); name/arch of one device into buf */
int fpca_device_count(void);
int fpca_device_name(int device, char *buf, int buflen);
/* start the HIP runtime and the device's primary context (0.1-0.2 s the first time in a process).  Thread-safe and
 * idempotent: a caller may run it on a helper thread while it parses its text inputs (the CLI does); every fpca_create*
 * does the same work itself if nobody has. */
int fpca_warmup(int device);

/* ------------------------------------------------------------------------------------------------
 * Data: replaces Data::get_size + Data::prepare (data.cpp:150-206).  `packed` is the body of a SNP-major
 * PLINK .bed for this shard: P_g records of ceil(N/4) bytes (i.e. file offset 3 + ceil(N/4)*snp_begin),
 * sample 4i+s of a record in bits 2s..2s+1 of byte i (data.cpp:128-148).  The bytes are copied to HBM
 * (re-pitched to 128-byte rows, pad positions rewritten to the "missing" code so they contribute 0);
 * the caller may free `packed` on return. */
int fpca_create(fpca_ctx **out, const uint8_t *packed, uint64_t N, uint64_t P_g, int stand_method,
                int device, int accum);

/* Same, reading the shard straight from a .bed file: records [snp_begin, snp_begin + P_g) (P_g = 0 means
 * "to the end of the file").  N comes from the .fam as in the reference (flashpca.cpp:589). The total SNP
 * count of the file, (filesize-3)/ceil(N/4) by integer division (data.cpp:165-170), is returned in *P_total. */
int fpca_create_from_bed(fpca_ctx **out, const char *bed_path, uint64_t N, uint64_t snp_begin, uint64_t P_g,
                         int stand_method, int device, int accum, uint64_t *P_total);

/* Synthetic shard generated directly in HBM (bench / scale tests): structured
 * population model, counter-based RNG keyed by (seed, snp, sample) so that any SNP range of the same
 * (N, seed, n_pop, fst, missing_rate) matrix can be generated independently on any rank. */
int fpca_create_synthetic(fpca_ctx **out, uint64_t N, uint64_t snp_begin, uint64_t P_g, uint64_t seed,
                          int n_pop, double fst, double missing_rate, int stand_method, int device, int accum);

/* The same generator with the knobs that make the matrix look like array / sequencing data instead of the survey's uniform model
 * (flashpca_amd/csrc/synth.hpp): maf_model 1 = rare-variant spectrum (minor-allele frequency 0.001 + 0.499 u^3: per-SNP sd over a
 * 16x range, SNPs monomorphic in small samples); missing_model 1 = missing calls concentrated in `conc_frac` of the SNPs (10-30 %
 * of their calls; every other SNP <= 0.1 %; missing_rate is ignored); missing_model 2 = per-SNP rates log-normally distributed
 * with log-sd lognormal_sigma (capped at 90 %): most SNPs below the mean, a long tail of poor assays.  missing_rate is the NOMINAL
 * mean: the median is missing_rate exp(-sigma^2 / 2), but the tail that carries the rest of the mean is cut (the normal ends at 6 sd,
 * the 90 % cap, 16-bit thresholds floor small rates) -- nominal mean; realised mean of the thresholds 0.87-1.00 of it, see
 * profiles/synth_model_figures.txt.
 * maf_model = missing_model = 0 is fpca_create_synthetic. */
typedef struct fpca_synth_model {
   int n_pop;            /* sub-populations (1..64): n_pop - 1 structured eigenvalues */
   double fst;
   double missing_rate;  /* missing_model 0: every call; 2: the nominal mean over SNPs (above) */
   int maf_model, missing_model;
   double conc_frac;     /* missing_model 1: fraction of SNPs with 10-30 % missing calls (e.g. 0.05) */
   double lognormal_sigma; /* missing_model 2: sd of ln(rate) over SNPs (e.g. 1.5) */
} fpca_synth_model;
int fpca_create_synthetic_model(fpca_ctx **out, uint64_t N, uint64_t snp_begin, uint64_t P_g, uint64_t seed, const fpca_synth_model *model,
                                int stand_method, int device, int accum);

/* In-memory matrix input: replaces RandomPCA::pca_fast(MatrixXd& X, ...) + standardise(X, method) (randompca.cpp:121-166,
 * util.cpp:24-192; the R entry flashpca(X) for a numeric matrix, flashpcaR/src/flashpca.cpp:17-93).  X is N x P_g fp64
 * column-major with leading dimension ldx, NaN = missing.  It is copied to HBM and standardised there column by column
 * exactly as standardise() does (missing -> 0 after standardisation, or -> mean for "none"; sd <= 1e-9 -> the column
 * becomes its mean); every operator / driver entry point then works on it like on a packed context (fp64 only). */
int fpca_create_dense(fpca_ctx **out, const double *X, int64_t ldx, uint64_t N, uint64_t P_g, int stand_method, int device);

void fpca_destroy(fpca_ctx *ctx);

uint64_t fpca_nsamples(const fpca_ctx *ctx);   /* Data::N */
uint64_t fpca_nsnps(const fpca_ctx *ctx);      /* shard's P_g (Data::nsnps for a 1-shard run) */
int fpca_accum(const fpca_ctx *ctx);           /* the FPCA_ACCUM_* mode in effect (AUTO resolved; may drop to FP64 at the first apply) */
/* how the exact-integer path treats the missing-call indicator for blocks of b columns (chosen from K1's counts of this
 * shard): 0 = both integer matrices on the matrix cores, 1 = the same, skipping blocks without a missing call, 2 = the
 * shard has no missing call (one matrix), 3 = one matrix on the matrix cores + the missing-call products as sparse fp64
 * gathers, 4 = hybrid: as 3 for most SNPs, while the SNPs whose missing calls would cost more to gather than their indicator row
 * costs on the matrix cores (above ~0.7 % each at 7 slices: failed assays, the tail of a log-normal rate profile) keep their
 * indicator there as a compacted sub-matrix -- taken when the per-SNP minima beat both uniform routes; -1 = not the exact-integer path.  Negative
 * FPCA_E* on error. */
int fpca_missing_mode(fpca_ctx *ctx, int b);
/* row chunks of Y whose all-reduce the built-in communicator overlaps with the computation of the next chunk (1 = one
 * all-reduce after K3; always 1 without a communicator or with a caller-supplied all-reduce hook) */
int fpca_allreduce_chunks(fpca_ctx *ctx);
/* copy the shard's packed stream back (P_g * ceil(N/4) bytes, .bed body layout) -- used by the tests to feed
 * the CPU oracle the exact matrix a synthetic context holds */
int fpca_download_packed(fpca_ctx *ctx, uint8_t *out);

/* K1.  Replaces the first-visit branch of Data::read_snp_block (data.cpp:257-322): per-SNP mean over
 * non-missing dosages, sd = sqrt(2P(1-P)) [binom2] / sqrt(P(1-P)) [binom], lookup table by raw code, and
 * trace = sum X^2 (svdwide.cpp:44-45,60-61) for this shard.  mean_sd: P_g x 2 column-major (mean | sd), may be
 * NULL; trace_out may be NULL.  Called implicitly by the first apply if the caller did not. */
int fpca_stats(fpca_ctx *ctx, double *mean_sd, double *trace_out);
/* preloaded mean/sd (projection path, data.cpp:293-297, randompca.cpp:753-788); P_g x 2 column-major */
int fpca_set_meansd(fpca_ctx *ctx, const double *mean_sd);

/* Sample subset: PCs fitted on the kept samples, everyone else projected onto them, on the resident packed matrix (no second
 * .bed of the subset, no --outload / --project round trip).  keep: N bytes, non-zero = kept; NULL clears the mask, after which
 * the context behaves as a fresh one.  The mask is context state.  While it is set:
 *   fpca_stats        mean, sd, lookup table and trace are those of the kept samples (K1's formulas in K1's order: bit-identical to
 *                     K1 on the re-packed subset); a SNP monomorphic among the kept samples is a zero column
 *   fpca_apply_xt     the held-out rows of B count as zero: T = X_kept' B_kept
 *   fpca_apply_xxt, fpca_apply_xxt_dev   Y = X_kept X_kept' B on the kept rows, exactly 0 on the others
 *   fpca_apply_x      all N rows (the projection of the held-out samples under the subset's standardisation)
 *   fpca_pca          the kept-sample problem: divisor n1 = n_kept - 1, ndim <= (min(n_kept, P) - 1) / 2; U (N x ndim) has zero held-out
 *                     rows and unit-norm columns; Px is U sqrt(d) on the kept rows and X V / sqrt(div) on the others (V the loadings of
 *                     the kept-sample problem: what --project computes), from one K2 + K3 pass after the solve; V, mean_sd, pve, trace
 *                     are those of the kept-sample problem
 * FPCA_EINVAL, before any device work: a dense context, fewer than 2 kept samples, a context that is one shard of several (and the
 * calls that would make a masked context one), a preloaded mean/sd (either order), and fpca_check / fpca_ucca / fpca_scca_* /
 * fpca_scca_cv while a mask is set.  Costs one pass over the packed stream. */
int fpca_set_sample_mask(fpca_ctx *ctx, const uint8_t *keep);
uint64_t fpca_nkept(const fpca_ctx *ctx); /* samples the statistics and fpca_pca run on: n_kept under a mask, else N */

/* SNP subset: the analyses run on a list of SNPs, or on those that pass a minor-allele-frequency / call-rate filter, without a second
 * fileset.  The kept records are compacted ONCE, on the device, into a new context; that context is an ordinary one, so PCA, the
 * operator, UCCA, SCCA and cv.scca run on it unchanged.
 *   fpca_snp_missing        n_missing[P_g]: K1's per-SNP counts of missing calls over all N samples (K1 runs if nobody has).
 *   fpca_snp_qc             keep[P_g] is input and output: an entry that is 0 stays 0 (list filters and QC filters compose), a non-zero
 *                           entry becomes 1 or 0; *n_kept (may be NULL) = entries left non-zero.  From K1's per-SNP mean and missing
 *                           count, on the host: p = mean / 2, maf = min(p, 1 - p), dropped when maf < min_maf; miss = n_missing / N,
 *                           dropped when miss > max_missing.  Both comparisons strict, as in PLINK (--maf, --geno): a SNP exactly at a
 *                           threshold stays.  min_maf <= 0 / max_missing >= 1 disable a filter; a SNP without a single call counts as
 *                           maf = 0.  FPCA_EINVAL for a NaN threshold, min_maf > 0.5, max_missing < 0.
 *                           Both calls: FPCA_EINVAL for a dense context, while a sample mask is set (the counts are all-sample counts)
 *                           and after fpca_set_meansd (K1 never counted).
 *   fpca_create_snp_subset  a NEW, fresh context on src's device with src's N and standardisation method, whose SNPs are the records of
 *                           src with keep[j] != 0 (keep: P_g bytes), in order; accum: any FPCA_ACCUM_*, as for fpca_create.  Nothing else
 *                           of src is inherited (statistics, sample mask, preloaded mean/sd, SCCA state); its own SNP count is its total
 *                           (fpca_set_total_snps).  src is left untouched and usable.  The new packed matrix is byte for byte what
 *                           fpca_create builds from the re-packed kept records.  One record gather at HBM speed (pitch * P_kept bytes
 *                           read, as many written); the call returns after one synchronise.  Source and subset are resident together
 *                           until the caller destroys the source: FPCA_ENOMEM, with both sizes in the message, when the second matrix
 *                           does not fit.  FPCA_EINVAL, before any device work: out, src or keep NULL, a dense src, a src that is one
 *                           shard of several (a communicator, an all-reduce hook, fpca_set_rank with more than one rank), zero kept SNPs. */
int fpca_snp_missing(fpca_ctx *ctx, uint32_t *n_missing);
int fpca_snp_qc(fpca_ctx *ctx, double min_maf, double max_missing, uint8_t *keep, uint64_t *n_kept);
int fpca_create_snp_subset(fpca_ctx **out, fpca_ctx *src, const uint8_t *keep, int accum);

/* LD pruning: windowed pairwise r2 between the SNPs of the resident matrix, on the int8 matrix cores, and a PLINK-1.9-style
 * --indep-pairwise rule on top of it.  The mask it leaves feeds fpca_create_snp_subset like any other.
 *   The statistic, for SNPs i < j, dosage x in {0,1,2}, over the samples called at BOTH SNPs (pairwise-complete):
 *      n = #samples, sx = sum x_i, sy = sum x_j, sxy = sum x_i x_j, sxx = sum x_i^2, syy = sum x_j^2     (exact integers)
 *      c = n sxy - sx sy, vx = n sxx - sx^2, vy = n syy - sy^2                                           (int64, exact)
 *      r2 = ((double)c * (double)c) / ((double)vx * (double)vy)        (two multiplies and one divide, each correctly rounded)
 *   0 / 0 is NaN (no shared call, or a SNP constant on the shared calls); a NaN is never above a threshold.
 *   fpca_ld_band   r2[nsnp][span], row-major: r2[i][d - 1] is the statistic of SNPs snp0 + i and snp0 + i + d, d = 1 .. span; NaN where
 *                  i + d >= nsnp.  FPCA_EINVAL when the buffer would exceed 1 GiB (both sizes in the message).
 *   fpca_ld_prune  keep[P_g] in and out, as for fpca_snp_qc: an entry that is 0 stays 0; *n_kept (may be NULL) = entries left non-zero.
 *                  Positions are record numbers within a chromosome; a chromosome is a maximal run of equal values of chrom[P_g] (NULL:
 *                  one chromosome).  Windows start at positions 0, step, 2 step, ... of the chromosome and cover `window` positions; the
 *                  window that reaches the chromosome's end is its last.  SNPs with keep == 0 on entry, and SNPs that are monomorphic over
 *                  their own calls (which includes "no call at all") -- these are set to 0 first --, occupy positions but are never
 *                  compared.  Within a window, for i ascending and still kept, for j > i ascending and still kept with r2(i, j) > r2:
 *                  when maf_i < maf_j (strictly; maf as fpca_snp_qc computes it) SNP i is dropped and the scan moves to the next i,
 *                  otherwise SNP j is dropped.  Not claimed: byte parity with the plink binary, whose window refill and MAF epsilon
 *                  differ in detail.  The device writes a bitmap of the pairs above the threshold (ceil((window - 1) / 32) words per
 *                  SNP, in slabs of at most 256 MiB; FPCA_ENOMEM with the sizes in the message when a slab does not fit), the rule runs
 *                  on the host.
 *   Both: FPCA_EINVAL for a NULL argument, span == 0, window < 2, step < 1, step > window, r2 NaN or outside [0, 1], a range outside the
 *   context, N > 2^25 (the integers above stay below 2^53), a dense context, a context under a sample mask or with a preloaded mean/sd
 *   (the statistic is over all N samples), and one shard of several.  The context is not changed. */
int fpca_ld_band(fpca_ctx *ctx, uint64_t snp0, uint64_t nsnp, uint32_t span, double *r2 /* [nsnp][span] */);
int fpca_ld_prune(fpca_ctx *ctx, const uint32_t *chrom /* [P_g] or NULL */, uint32_t window, uint32_t step, double r2,
                  uint8_t *keep /* in/out, like fpca_snp_qc */, uint64_t *n_kept);

/* Kinship: the KING-robust estimator (Manichaikul et al. 2010) between the samples of the resident matrix, on the int8 matrix cores, and
 * an unrelated-sample cutoff on top of it.  The mask it leaves feeds fpca_set_sample_mask.
 *   The statistic, for samples i and j, dosage x in {0,1,2}, q = x^2, h = 2x - q (1 at a heterozygous call), over the SNPs of the context
 *   called in BOTH samples:
 *      het_i = sum h_i, het_j = sum h_j, D = sum (x_i - x_j)^2, hmin = min(het_i, het_j)                   (exact integers)
 *      phi = (double)(2 hmin - D) / (double)(4 hmin)         (= 1/2 - D / (4 hmin); int64 numerator and denominator, ONE fp64 divide)
 *   phi is NaN when hmin == 0 (tested, not left to the divide); a NaN is never above a threshold; all comparisons are strict (phi > thr).
 *   A duplicate without a missing call gives exactly 0.5.
 *   fpca_king_block   phi[ni][nj], row-major: phi[a][b] is the statistic of samples i0 + a and j0 + b, for any rectangle (j <= i included;
 *                     at i == j the formula gives 0.5 or NaN).  FPCA_EINVAL when the buffer would exceed 1 GiB.
 *   fpca_king_pairs   every pair i < j with phi > thr whose samples both have keep != 0 (keep: N bytes, or NULL for all), sorted by (i, j),
 *                     in i[], j[], phi[] (max_pairs entries each); *n_pairs = their number.  When more than max_pairs qualify the call
 *                     returns FPCA_ENOMEM, *n_pairs is the number needed and the message names it; the arrays are then not written.
 *   fpca_king_cutoff  keep[N] in and out, as for fpca_snp_qc: an entry that is 0 stays 0; *n_kept (may be NULL) = entries left non-zero.
 *                     The pair pass above (room for 2^26 pairs, else FPCA_ENOMEM), then on the host: a graph on the samples with keep != 0
 *                     with an edge for every listed pair; while an edge remains, the sample of largest current degree is dropped, the one
 *                     of largest index among equals.  The purpose of plink2 --king-cutoff; byte parity with plink2 or KING is not claimed.
 *   Every call makes its own sample-major copy of the packed matrix (as large as the matrix; FPCA_ENOMEM with both sizes in the message
 *   when it does not fit) and frees it before it returns.
 *   All: FPCA_EINVAL, before any device work, for a NULL argument, a range outside the context, a NaN thr, a dense context, a context under
 *   a sample mask (pass the mask as keep instead), one shard of several, and more than 2^28 SNPs (the sums stay below 2^31).  A preloaded
 *   mean/sd is not refused: nothing here reads it.  The context is not changed. */
int fpca_king_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, double *phi /* [ni][nj] */);
int fpca_king_pairs(fpca_ctx *ctx, const uint8_t *keep /* [N] or NULL */, double thr, uint64_t max_pairs, uint32_t *i, uint32_t *j, double *phi,
                    uint64_t *n_pairs);
int fpca_king_cutoff(fpca_ctx *ctx, double thr, uint8_t *keep /* [N] in/out, like fpca_snp_qc */, uint64_t *n_kept);
/*   The relationship table: beside phi, the integers KING's own table of a pair rests on.  With a0 = 1 at a homozygous-A2 call (dosage 0),
 *   a2 = 1 at a homozygous-A1 call (dosage 2), over the SNPs called in BOTH samples:
 *      shared = their number, ibs0 = sum a0_i a2_j + a2_i a0_j (opposite homozygotes), hethet = sum h_i h_j, het_i, het_j, D as above
 *   A pair's counts are six uint32 in that order: shared, ibs0, hethet, het_i, het_j, D (het_i belongs to the first sample of the pair).
 *   The device forms them from seven exact int8 products: ibs0 = (tt - ss) / 2 with tt = shared - het_i - het_j + hethet (both homozygous)
 *   and ss = sum (x_i - m_i)(x_j - m_j) (+1 at equal, -1 at opposite homozygotes).  phi is formed as above and equals fpca_king_block /
 *   fpca_king_pairs BIT FOR BIT.
 *   fpca_king_counts_block   counts[ni][nj][6] and, when phi is not NULL, phi[ni][nj] for any rectangle, as fpca_king_block.  At i == j:
 *                            shared = the sample's calls, ibs0 = 0, D = 0.  FPCA_EINVAL when counts would exceed 1 GiB.
 *   fpca_king_related        fpca_king_pairs with a second condition and the counts: every pair i < j with phi > thr AND shared >=
 *                            min_shared whose samples both have keep != 0, sorted by (i, j), in i[], j[], phi[], counts[][6] (max_pairs
 *                            entries each); *n_pairs = their number.  min_shared = 0 lists exactly the pairs of fpca_king_pairs.  More
 *                            than max_pairs: FPCA_ENOMEM, *n_pairs is the number needed, the arrays are not written.  FPCA_EINVAL when
 *                            min(max_pairs, N (N - 1) / 2) entries of counts would exceed 1 GiB.
 *   fpca_king_cutoff_shared  fpca_king_cutoff on the pairs of fpca_king_related (the same room, the same rule on the host): a pair that
 *                            shares fewer than min_shared called SNPs is no edge.  min_shared = 0 gives exactly fpca_king_cutoff's mask.
 *   fpca_king_classify       host only, no context: type[k] of pair k from phi[k] and counts[k][6] (shared and ibs0 are read).  In this order:
 *                               255  no value: phi is NaN or shared == 0
 *                                 5  duplicate / MZ twin: phi > 0.354
 *                                 1  parent-offspring: 0.177 < phi <= 0.354 and (double)ibs0 / (double)shared < po_ibs0
 *                                 2  full sibs: 0.177 < phi <= 0.354 otherwise
 *                                 3  second degree: 0.0884 < phi <= 0.177
 *                                 4  third degree: 0.0442 < phi <= 0.0884
 *                                 0  unrelated
 *                            FPCA_EINVAL for a NULL array with n_pairs > 0 and a po_ibs0 that is NaN, infinite or negative.  The cut
 *                            points are KING's (2^-1.5, 2^-2.5, ... rounded as its manual prints them); po_ibs0 is a convention of the
 *                            caller (the Python layer passes 0.005).  Parity with the KING binary's inference is not claimed.
 *   The three device calls refuse what the calls above refuse, make the same sample-major copy and leave the context unchanged. */
int fpca_king_counts_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, uint32_t *counts /* [ni][nj][6] */,
                           double *phi /* [ni][nj] or NULL */);
int fpca_king_related(fpca_ctx *ctx, const uint8_t *keep /* [N] or NULL */, double thr, uint32_t min_shared, uint64_t max_pairs, uint32_t *i,
                      uint32_t *j, double *phi, uint32_t *counts /* [max_pairs][6] */, uint64_t *n_pairs);
int fpca_king_cutoff_shared(fpca_ctx *ctx, double thr, uint32_t min_shared, uint8_t *keep /* [N] in/out */, uint64_t *n_kept);
int fpca_king_classify(uint64_t n_pairs, const double *phi, const uint32_t *counts /* [n_pairs][6] */, double po_ibs0, uint8_t *type /* [n_pairs] */);
/*   PC-AiR's partition (Conomos, Miller & Thornton 2015): an unrelated set chosen by kinship AND by ancestry divergence -- the first half of
 *   the PC-AiR / PC-Relate pipeline.  A strongly negative phi marks a pair of divergent ancestry; of two relatives the one with more
 *   divergent partners stays, so that the unrelated set stays representative of every ancestry.
 *   Over the pairs i < j whose samples both have keep != 0, with phi exactly fpca_king_block's value (the same five integer products, the
 *   same int64 combination, the same single fp64 divide, NaN where min(het) == 0):
 *      related     phi > kin_thr
 *      divergent   phi < div_thr AND not related AND (i, j) not in the caller's exclusion list
 *   A NaN pair is neither.  kin_thr = +inf is allowed ("no relatives from KING"); kin_thr < div_thr is allowed, related wins; NaN
 *   thresholds are refused.  n_rel[s] / n_div[s] = the related / divergent pairs that contain sample s; 0 for a sample with keep == 0.
 *   2^-5.5 and -2^-5.5 are the customary thresholds (GENESIS's defaults).
 *   The rule, on the host, on the graph whose edges are the related pairs among the samples with keep != 0, each with a kinship `kin`:
 *      1. while an edge remains, one sample is moved to the related set (keep -> 0);
 *      2. it is the one of largest current degree;
 *      3. among equals, the one of smallest n_div (n_div is fixed as given: it is not recomputed as samples leave);
 *      4. among equals, the one of smallest sum of kin over its CURRENT edges -- in fp64, recomputed from the current edges each time it
 *         is needed, added in ascending order of the neighbour's index, never maintained by subtraction;
 *      5. among equals, the one of largest index (fpca_king_cutoff's tie rule).
 *   Duplicate and reversed pairs count once, with the first kin listed for the pair.  This is GENESIS::pcairPartition in structure; the
 *   order of the tie-breaks 3 - 5 is written from the paper, and PARITY WITH GENESIS IS NOT CLAIMED (as none is with plink2 or KING above).
 *   fpca_king_census      n_rel[N] and n_div[N] from ONE pass over the triangle (k_king_census: k_king's products, the counts reduced in
 *                         the wave and added with integer atomics -- exact, hence the same in any order).  (excl_i[k], excl_j[k]), k <
 *                         n_excl: pairs never counted divergent, in either order, repeats allowed; FPCA_EINVAL for i == j or an index >= N.
 *   fpca_pcair_partition  host only, no context: the rule.  (i[k], j[k], kin[k]), k < n_pairs: the edges; n_div[N]; keep[N] in and out
 *                         (entries become 0 / 1, a 0 stays 0); *n_kept (may be NULL) = entries left non-zero.  FPCA_EINVAL, with keep
 *                         untouched, for a pair with i == j or an index >= N, a kin that is NaN or infinite, a NULL array and N >= 2^32.
 *                         Memory linear in N + n_pairs.
 *   fpca_pcair_king       the census and the list of related pairs (with phi as kin) from ONE fused pass, then the rule.  Room for 2^26
 *                         related pairs, else FPCA_ENOMEM naming their number.  n_rel / n_div (may be NULL): the census the rule saw.
 *   fpca_pcair_pairs      relatives from outside (PC-Relate, the GRM): the census with kin_thr = +inf and the given pairs as the exclusion
 *                         list, then the rule on the given pairs.  n_div (may be NULL): the census the rule saw.
 *   The three device calls refuse what the calls above refuse, before any device work, make the same sample-major copy and leave the
 *   context unchanged. */
int fpca_king_census(fpca_ctx *ctx, const uint8_t *keep /* [N] or NULL */, double kin_thr, double div_thr,
                     const uint32_t *excl_i, const uint32_t *excl_j, uint64_t n_excl,      /* pairs never counted divergent; may be 0 / NULL */
                     uint32_t *n_rel /* [N] */, uint32_t *n_div /* [N] */);
int fpca_pcair_partition(uint64_t N, uint64_t n_pairs, const uint32_t *i, const uint32_t *j, const double *kin,
                         const uint32_t *n_div /* [N] */, uint8_t *keep /* [N] in/out */, uint64_t *n_kept);   /* host only, no context: the rule */
int fpca_pcair_king(fpca_ctx *ctx, double kin_thr, double div_thr, uint8_t *keep /* [N] in/out */, uint64_t *n_kept,
                    uint32_t *n_rel /* [N] or NULL */, uint32_t *n_div /* [N] or NULL */);   /* ONE fused triangle pass, then the rule */
int fpca_pcair_pairs(fpca_ctx *ctx, double div_thr, uint64_t n_pairs, const uint32_t *i, const uint32_t *j, const double *kin,
                     uint8_t *keep /* [N] in/out */, uint64_t *n_kept, uint32_t *n_div /* [N] or NULL */);

/* Relationship matrix: the genetic relationship matrix (GRM) of the samples of the resident matrix -- the X X' / P whose eigenvectors
 * fpca_pca computes without forming it -- on the FP64 matrix cores, and a relatedness cutoff on top of it (the purpose of plink
 * --rel-cutoff / gcta --grm-cutoff).  The mask it leaves feeds fpca_set_sample_mask.
 *   For SNP s of the context, t_s[code] is the context's table entry: (x - mean_s) / sd_s at a call, 0 at a missing call, all four entries 0
 *   when sd_s <= 1e-9 or NaN.  mean_s and sd_s are the context's own: over all N samples under the context's standardisation, or what
 *   fpca_set_meansd loaded (with FPCA_STANDARDISE_BINOM2 this is the GRM of Yang et al. / GCTA; no frequency is re-estimated here).  A SNP
 *   is LIVE when its table is not all zero.
 *      z_is = t_s[code_is]        S_ij = sum_s z_is z_js        n_ij = the live SNPs called in both i and j
 *   SNPs that are not live contribute to neither sum.  G_ij is
 *      S_ij / n_ij   under FPCA_GRM_DIV_SHARED (the pairwise-complete form of GCTA)
 *      S_ij / P_g    under FPCA_GRM_DIV_P      (X X' / P of fpca_pca under FPCA_DIVISOR_P: missing calls mean-imputed)
 *      S_ij          under FPCA_GRM_DIV_NONE
 *   each ONE fp64 divide of S_ij by the integer converted to double.  Under FPCA_GRM_DIV_SHARED, n_ij == 0 is tested and gives NaN.  A NaN is
 *   never above a threshold; all comparisons are strict (G > thr).  S_ij is accumulated in fp64 without atomics and without a split along
 *   the SNPs: a call is deterministic, and G_ij and G_ji are the same bits.
 *   fpca_grm_block   grm[ni][nj], row-major: grm[a][b] is G of samples i0 + a and j0 + b, for any rectangle (j <= i included); shared
 *                    (may be NULL): n likewise.  FPCA_EINVAL when grm would exceed 1 GiB.
 *   fpca_grm_tri     the lower triangle with the diagonal, row by row: entry i (i + 1) / 2 + j is G_ij, j <= i (GCTA's order), N (N + 1) / 2
 *                    entries; shared (may be NULL): n in the same order.  Host buffers of any size; computed in slabs of rows, each
 *                    downloaded as it finishes.
 *   fpca_grm_pairs   every pair i < j with G > thr whose samples both have keep != 0 (keep: N bytes, or NULL for all), sorted by (i, j), in
 *                    i[], j[], g[] and (may be NULL) shared[] (max_pairs entries each); *n_pairs = their number.  When more than max_pairs
 *                    qualify the call returns FPCA_ENOMEM, *n_pairs is the number needed and the message names it; the arrays are then not
 *                    written.
 *   fpca_grm_cutoff  keep[N] in and out, as for fpca_king_cutoff: the pair pass above (room for 2^26 pairs, else FPCA_ENOMEM), then
 *                    fpca_king_cutoff's rule on the host, unchanged.  0.025 is the customary threshold.  Byte parity with plink or gcta is
 *                    not claimed.
 *   Every call makes its own sample-major copy of the packed matrix and a scratch of at most 256 MiB for the sums and counts of a slab
 *   (FPCA_ENOMEM with both sizes in the message when one does not fit) and frees them before it returns.
 *   All: FPCA_EINVAL, before any device work, for a NULL argument, a divisor other than the three, a range outside the context or a
 *   zero-sized block, a NaN thr, a dense context, a context under a sample mask, one shard of several, more than 2^28 SNPs (n_ij fits 32
 *   bits) and 2^32 samples or more.  The context is not changed. */
#define FPCA_GRM_DIV_SHARED 0
#define FPCA_GRM_DIV_P 1
#define FPCA_GRM_DIV_NONE 2
int fpca_grm_block(fpca_ctx *ctx, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj, int divisor, double *grm /* [ni][nj] */,
                   uint32_t *shared /* [ni][nj] or NULL */);
int fpca_grm_tri(fpca_ctx *ctx, int divisor, double *grm /* [N (N + 1) / 2] */, uint32_t *shared /* same, or NULL */);
int fpca_grm_pairs(fpca_ctx *ctx, const uint8_t *keep /* [N] or NULL */, double thr, int divisor, uint64_t max_pairs, uint32_t *i, uint32_t *j,
                   double *g, uint32_t *shared /* or NULL */, uint64_t *n_pairs);
int fpca_grm_cutoff(fpca_ctx *ctx, double thr, int divisor, uint8_t *keep /* [N] in/out */, uint64_t *n_kept);

/* PC-Relate (Conomos et al. 2016): kinship between the samples of the resident matrix adjusted for principal components, on the FP64 matrix
 * cores -- the second half of the PC-AiR / PC-Relate pipeline, fed by the PCs fpca_pca fits on an unrelated set.  Every SNP is regressed on
 * the PCs; the fitted value is an individual-specific allele frequency, so that population structure inflates no pair's kinship.
 *   Dosage    x_is in {2, -, 1, 0} for the raw codes {0, 1, 2, 3}; code 1 is a missing call.
 *   Live      SNP s is LIVE when sd_s > 1e-9 and neither mean_s nor sd_s is NaN (the rule of the relationship matrix above).  A SNP that is
 *             not live contributes nowhere and has beta_s = 0.
 *   V         V = [1 | pcs], N x d, d = npc + 1, 0 <= npc <= 31.  pcs is row-major [N][npc]; the library prepends the ones.
 *   train     N bytes, or NULL for all samples: the samples whose genotypes estimate beta (the unrelated set).
 *   beta      beta_s = argmin sum_{i in train} (g_is - V_i beta)^2 with g_is = x_is at a call and mean_s at a missing call.  mean_s is the
 *             context's own mean over ALL samples (or what fpca_set_meansd loaded): nothing is re-estimated over train.  In steps: B = V with
 *             the rows outside train zeroed goes through the context's own K2 pass, T_sk = sum_{i in train} z_is V_ik; rhs_sk = mean_s c_k +
 *             sd_s T_sk with c_k = sum_{i in train} V_ik (sd z = x - mean, whichever standardisation the context has); beta_s = A^-1 rhs_s
 *             with A = V_train' V_train, factored once on the host by Cholesky in fp64 (A and c summed in long double and rounded once) and
 *             refused when a pivot is <= 1e-12 x the largest pivot before it; the two substitutions per SNP run on the device.
 *   Usable    mu_is = V_i.beta_s / 2 (the dot product in the order k = 0 .. d - 1).  SNP s is USABLE in sample i when it is live, called in
 *             i, and eps < mu_is < 1 - eps (strict).  0 <= eps < 0.5; 0.01 is GENESIS's maf.thresh.
 *   Operands  r_is = x_is - 2 mu_is and w_is = sqrt(mu_is (1 - mu_is)) where usable, both 0 elsewhere.
 *      S_ij = sum_s r_is r_js        D_ij = sum_s w_is w_js        kin_ij = S_ij / (4 D_ij)
 *   one multiply by 4 (exact) and ONE fp64 divide; D_ij == 0 is tested and gives NaN.  The diagonal is (1 + f_i) / 2: the inbreeding
 *   coefficient is 2 kin_ii - 1.  S and D are accumulated in fp64 without atomics and without a split along the SNPs: a call is
 *   deterministic, kin_ij and kin_ji are the same bits.
 *   fpca_pcrelate_beta    beta[P_g][npc + 1], row-major.
 *   fpca_pcrelate_block   kin[ni][nj], row-major: kin[a][b] is the kinship of samples i0 + a and j0 + b, for any rectangle; den (may be
 *                         NULL): D likewise.  FPCA_EINVAL when kin would exceed 1 GiB.
 *   fpca_pcrelate_tri     the lower triangle with the diagonal, row by row: entry i (i + 1) / 2 + j is kin_ij, j <= i, N (N + 1) / 2 entries;
 *                         den (may be NULL): D in the same order.  Host buffers of any size; computed in slabs of rows, each downloaded as
 *                         it finishes.
 *   beta == NULL in the last two means "estimate it from train": the result is bit for bit that of fpca_pcrelate_beta followed by the call
 *   with its beta.  With beta given, train is ignored.
 *   Every call makes its own sample-major copy of the packed matrix, a scratch of at most 256 MiB for S and D of a slab and panels of r and
 *   w of at most 1 GiB (FPCA_ENOMEM with the sizes in the message when one does not fit, or when one 512-SNP panel would pass 1 GiB) and
 *   frees them before it returns.
 *   All: FPCA_EINVAL, before any device work, for a NULL context or output, a dense context, a context under a sample mask, one shard of
 *   several, npc outside 0 .. 31, a non-finite entry of pcs or beta, fewer than npc + 2 training samples, a rank-deficient A, eps outside
 *   [0, 0.5), and a range outside the context or a zero-sized block.  The context is not changed. */
int fpca_pcrelate_beta(fpca_ctx *ctx, const double *pcs /* [N][npc] */, int npc, const uint8_t *train /* [N] or NULL */,
                       double *beta /* [P_g][npc + 1] */);
int fpca_pcrelate_block(fpca_ctx *ctx, const double *pcs /* [N][npc] */, int npc, const double *beta /* [P_g][npc + 1] or NULL */,
                        const uint8_t *train /* [N] or NULL */, double eps, uint64_t i0, uint64_t ni, uint64_t j0, uint64_t nj,
                        double *kin /* [ni][nj] */, double *den /* same, or NULL */);
int fpca_pcrelate_tri(fpca_ctx *ctx, const double *pcs /* [N][npc] */, int npc, const double *beta /* [P_g][npc + 1] or NULL */,
                      const uint8_t *train /* [N] or NULL */, double eps, double *kin /* [N (N + 1) / 2] */, double *den /* same, or NULL */);

/* PC-Relate IBD sharing: the probabilities k0, k1, k2 that a pair shares 0, 1, 2 alleles identical by descent, adjusted for the principal
 * components as the kinship above is, the SNPs usable in both samples, and the relationship type they imply -- what tells a parent-offspring
 * pair (k0 = 0) from full sibs (k0 = 1/4) where both have kinship 1/4.  Dosage, live SNPs, V = [1 | pcs], beta, mu_is = V_i.beta_s / 2 (the dot
 * product in the order k = 0 .. d - 1) and USABLE (live, called, eps < mu_is < 1 - eps, strict) are those of PC-Relate above, unchanged.
 *   Operands  m_is in {0, 1} is the usable indicator.  At a usable cell, with mu = mu_is and x = x_is:
 *                v = mu (1 - mu)        gD = mu if x = 0, 0 if x = 1, 1 - mu if x = 2        q = gD - v
 *                u = mu^2               t = (1 - mu)^2               a = [x = 0]               c = [x = 2]
 *             each product and each difference rounded once (nothing is fused); every operand is 0 where m_is = 0.
 *   Sums      Q_ij = sum_s q_is q_js        E_ij = sum_s v_is v_js        H_ij = sum_s (u_is t_js + t_is u_js)
 *             I0_ij = sum_s (a_is c_js + c_is a_js), the opposite homozygotes among the SNPs usable in both samples
 *             n_ij = sum_s m_is m_js
 *             all in fp64 without atomics and without a split along the SNPs: a call is deterministic.  The two halves of H, sum u_i t_j and
 *             sum t_i u_j, are kept apart in SNP order and added once, so k2, k0 and nsnp of (i, j) and (j, i) are the same bits.  I0 and n
 *             are integers, exact.
 *   k2_ij   = Q_ij / E_ij - f_i f_j (the corrected form of GENESIS): ONE fp64 divide, one rounded multiply, one rounded subtract, never a
 *             fused multiply-add; E_ij == 0 is tested and gives NaN.  f[N] are inbreeding coefficients supplied by the caller -- 2 kin_ii - 1
 *             from fpca_pcrelate_tri; NULL means zeros.
 *   k0_ij   = I0_ij / H_ij: one divide; H_ij == 0 is tested and gives NaN.
 *   nsnp_ij = n_ij as uint32.
 *   Diagonal entries follow the same formulas and carry no meaning.
 *   fpca_pcrelate_ibd_block   k2[ni][nj], k0[ni][nj], nsnp[ni][nj], row-major, of samples i0 + a and j0 + b, for any rectangle.  Any of the
 *                             three may be NULL, not all three.  FPCA_EINVAL when ni x nj doubles would exceed 1 GiB.
 *   fpca_pcrelate_ibd_tri     the lower triangle with the diagonal, row by row: entry i (i + 1) / 2 + j, j <= i, N (N + 1) / 2 entries each;
 *                             host buffers of any size, computed in slabs of rows, each downloaded as it finishes.
 *   beta == NULL means "estimate it from train", bit for bit that of fpca_pcrelate_beta followed by the call with its beta.
 *   Every call makes its own sample-major copy of the packed matrix, a scratch of at most 256 MiB for the six sums of a slab (Q, E, the two
 *   halves of H, 2 I0, n) and three operand panels of at most 1 GiB together (FPCA_ENOMEM with the sizes in the message when one does not fit,
 *   or when three 512-SNP panels would pass 1 GiB) and frees them before it returns.
 *   Both: FPCA_EINVAL, before any device work, for everything fpca_pcrelate_block refuses -- a NULL context, a dense context, a context under
 *   a sample mask, one shard of several, npc outside 0 .. 31, a non-finite entry of pcs or beta, fewer than npc + 2 training samples, a
 *   rank-deficient A, eps outside [0, 0.5), a range outside the context or a zero-sized block -- for three NULL outputs and for a non-finite
 *   entry of f.  The context is not changed.
 *   fpca_pcrelate_classify    host only, no context: per pair p from kin[p] (fpca_pcrelate_tri), k0[p] (the IBS0 form above), k2[p], nsnp[p]
 *                                k0_out = k0 when kin > k0_switch, else 1 - 4 kin + k2 (the paper's rule: the IBS0 form for close pairs)
 *                                k1_out = 1 - k0_out - k2
 *                             and type[p], fpca_king_classify's codes at KING's cut points on kin, in this order:
 *                                255  no value: kin is NaN, k0_out is NaN or nsnp == 0
 *                                  5  duplicate / MZ twin: kin > 0.354
 *                                  1  parent-offspring: 0.177 < kin <= 0.354 and k0_out < po_k0
 *                                  2  full sibs: 0.177 < kin <= 0.354 otherwise
 *                                  3  second degree: 0.0884 < kin <= 0.177
 *                                  4  third degree: 0.0442 < kin <= 0.0884
 *                                  0  unrelated
 *                             FPCA_EINVAL for a NULL array with n_pairs > 0 and for a k0_switch or po_k0 that is NaN or infinite.  Both
 *                             thresholds are conventions of the caller: the Python layer passes k0_switch = 2^-5.5 (the paper's third-degree
 *                             bound) and po_k0 = 0.1 (after KING's manual).  Parity with GENESIS::pcrelate is not claimed. */
int fpca_pcrelate_ibd_block(fpca_ctx *ctx, const double *pcs /* [N][npc] */, int npc, const double *beta /* [P_g][npc + 1] or NULL */,
                            const uint8_t *train /* [N] or NULL */, double eps, const double *f /* [N] or NULL */, uint64_t i0, uint64_t ni,
                            uint64_t j0, uint64_t nj, double *k2 /* [ni][nj] or NULL */, double *k0 /* same, or NULL */,
                            uint32_t *nsnp /* same, or NULL */);
int fpca_pcrelate_ibd_tri(fpca_ctx *ctx, const double *pcs /* [N][npc] */, int npc, const double *beta /* [P_g][npc + 1] or NULL */,
                          const uint8_t *train /* [N] or NULL */, double eps, const double *f /* [N] or NULL */,
                          double *k2 /* [N (N + 1) / 2] or NULL */, double *k0 /* same, or NULL */, uint32_t *nsnp /* same, or NULL */);
int fpca_pcrelate_classify(uint64_t n_pairs, const double *kin, const double *k0, const double *k2, const uint32_t *nsnp, double k0_switch,
                           double po_k0, double *k0_out /* [n_pairs] */, double *k1_out /* [n_pairs] */, uint8_t *type /* [n_pairs] */);

/* Genotype census: counts per SNP over a chosen set of samples, counts per sample over a chosen set of SNPs, the Hardy-Weinberg exact test
 * on such counts, and the two QC rules on top of them -- PLINK's --mind (per-sample call rate) and --geno / --maf / --hwe over the KEPT
 * samples.  The masks they leave feed fpca_set_sample_mask and fpca_create_snp_subset.
 *   Raw codes.  Every count is indexed by the raw .bed code c: 0 homozygous A1 (dosage 2), 1 missing, 2 heterozygous, 3 homozygous A2
 *   (dosage 0).  Pad cells (samples >= N, records >= P_g) are never counted.
 *   fpca_snp_counts      counts[j][c], j < P_g: over the samples i < N with samples[i] != 0 (NULL: all).
 *   fpca_sample_counts   counts[i][c], i < N: over the SNPs j < P_g with snps[j] != 0 (NULL: all).  Slabs of SNPs are combined with integer
 *                        adds, so a repeat call is bit-identical.
 *   fpca_sample_qc       samples[N] in and out, as for fpca_snp_qc: an entry that is 0 stays 0; *n_kept (may be NULL) = entries left
 *                        non-zero.  n_snps = the SNPs counted (snps as above), miss_i = (double)counts[i][1] / (double)n_snps over ALL of
 *                        them whatever samples[] holds; sample i is dropped when miss_i > max_missing (strict: a sample exactly at the
 *                        threshold stays).  max_missing >= 1 disables the filter.  FPCA_EINVAL when n_snps == 0, max_missing is NaN or < 0.
 *   fpca_snp_qc_samples  snps[P_g] in and out likewise.  Counts over the samples with samples[i] != 0 (NULL: all), n of them;
 *                        ngood = cnt[0] + cnt[2] + cnt[3].
 *                           geno: dropped when (double)cnt[1] / (double)n > max_missing                     (max_missing >= 1: off)
 *                           maf:  mean = (double)(2 cnt[0] + cnt[2]) / (double)ngood, p = mean / 2, maf = ngood == 0 ? 0 : min(p, 1 - p);
 *                                 dropped when maf < min_maf -- K1's arithmetic: with all samples the decision is fpca_snp_qc's, bit for
 *                                 bit                                                                        (min_maf <= 0: off)
 *                           hwe:  dropped when p_hwe < min_hwe_p (strict), p_hwe as below                    (min_hwe_p <= 0: off)
 *                        FPCA_EINVAL for the thresholds fpca_snp_qc refuses, min_hwe_p NaN or above 1, and a mask that keeps no sample.
 *   fpca_hwe_exact       p[k], k < n, from counts[k][4] as above (column 1 is not read): the exact test of Wigginton, Cutler & Abecasis
 *                        (2005), without their array.
 *                           a = cnt[2], b = min(cnt[0], cnt[3]), c = max(cnt[0], cnt[3]), n = a + b + c, r = 2 b + a        (n == 0: p = 1)
 *                           the possible heterozygote counts are h = r, r - 2, ... >= 0
 *                           mid = floor(r (2n - r) / (2n)) in integers, plus 1 when its parity differs from r's;  w(mid) = 1
 *                           with hr = (r - h) / 2, hc = n - h - hr:
 *                              downwards  w(h - 2) = w(h) * (h (h - 1)) / (4 (hr + 1) (hc + 1))
 *                              upwards    w(h + 2) = w(h) * (4 hr hc) / ((h + 2) (h + 1))
 *                           (the integer factors are exact in fp64 for n < 2^26; ONE multiply and ONE divide are rounded per step, no FMA)
 *                           p = min(1, sum{ w(h) : w(h) <= w(a) (1 + 2^-20) } / sum w(h))
 *                        The factor 1 + 2^-20 makes exact ties (mirror-image terms) count whatever the rounding does.  A walk stops at a
 *                        term that is exactly 0.0 (every later one is 0 too); there is no other truncation.  w(a) == 0 through underflow
 *                        gives p = 0.  On the device, one SNP per lane.
 *   Not claimed: the mid-p variant; founders-only or controls-only counting; byte parity with the plink binary.
 *   All five: FPCA_EINVAL, before any device work, for a NULL argument (a mask documented as "NULL: all" excepted), a dense context, one
 *   shard of several, a context under a sample mask (clear it and pass the mask as `samples`), N or P_g >= 2^32.  A preloaded mean/sd is
 *   not refused: nothing here reads it.  The context is not changed. */
int fpca_snp_counts(fpca_ctx *ctx, const uint8_t *samples /* [N] or NULL */, uint32_t *counts /* [P_g][4] */);
int fpca_sample_counts(fpca_ctx *ctx, const uint8_t *snps /* [P_g] or NULL */, uint32_t *counts /* [N][4] */);
int fpca_hwe_exact(fpca_ctx *ctx, const uint32_t *counts /* [n][4] */, uint64_t n, double *p /* [n] */);
int fpca_sample_qc(fpca_ctx *ctx, const uint8_t *snps /* [P_g] or NULL */, double max_missing, uint8_t *samples /* [N] in/out */, uint64_t *n_kept);
int fpca_snp_qc_samples(fpca_ctx *ctx, const uint8_t *samples /* [N] or NULL */, double min_maf, double max_missing, double min_hwe_p,
                        uint8_t *snps /* [P_g] in/out */, uint64_t *n_kept);

/* ------------------------------------------------------------------------------------------------
 * Operator.  b columns at a time; b = 1 is exactly the reference's perform_op.
 *   fpca_apply_xxt : Y = X_g X_g' B        replaces SVDWideOnline::perform_op / perform_op_mat
 *                                           (svdwide.cpp:21-68, 71-118); summed over ranks when a
 *                                           communicator / all-reduce hook is installed
 *   fpca_apply_xt  : T = X_g' B  (P_g x b)  replaces SVDWideOnline::crossprod / crossprod2 (svdwide.cpp:122-188)
 *   fpca_apply_x   : Y = X_g T   (N x b)    replaces SVDWideOnline::prod / prod3 (svdwide.cpp:193-226, 312-343)
 * B, Y: N x b; T: P_g x b; host pointers, column-major, leading dimensions ldb/ldy/ldt (>= rows). */
int fpca_apply_xxt(fpca_ctx *ctx, const double *B, int64_t ldb, int b, double *Y, int64_t ldy);
int fpca_apply_xt(fpca_ctx *ctx, const double *B, int64_t ldb, int b, double *T, int64_t ldt);
int fpca_apply_x(fpca_ctx *ctx, const double *T, int64_t ldt, int b, double *Y, int64_t ldy);

/* Device-resident variants: B/Y are DEVICE pointers to row-major [fpca_block_rows()][b] fp64 blocks (rows
 * >= N must be zero on input and are zero on output); T lives in the context.  The kernels are enqueued on
 * `stream` (a hipStream_t; NULL = the context's own stream) and the call returns without synchronising.
 * This is what the solver and bench.py use so that B and Y never leave HBM during the iteration. */
uint64_t fpca_block_rows(const fpca_ctx *ctx); /* N rounded up to the kernels' sample tile (512) */
int fpca_apply_xxt_dev(fpca_ctx *ctx, const double *dB, int b, double *dY, void *stream);
/* contexts' own stream handle (hipStream_t) and a device-wide synchronise */
void *fpca_stream(fpca_ctx *ctx);
int fpca_synchronize(fpca_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU (SNP-sharded; one rank per GPU).  Two transports for the sum of the N x b partial products: */
#define FPCA_UNIQUE_ID_BYTES 128
/* (a) RCCL inside the library: rank 0 makes an id, the launcher broadcasts it, every rank joins. */
int fpca_comm_unique_id(uint8_t id[FPCA_UNIQUE_ID_BYTES]);
int fpca_comm_init_rank(fpca_ctx *ctx, int nranks, int rank, const uint8_t id[FPCA_UNIQUE_ID_BYTES]);
/* (b) caller-supplied in-place sum all-reduce of `count` fp64 at device pointer `dbuf`, ordered on `stream`
 * (e.g. torch.distributed over RCCL).  Must return 0 on success.
 * CONTRACT OF EVERY HOOK BELOW (all-reduce, all-gather, reduce-scatter): a collective fails AS A WHOLE -- a non-zero return must
 * be reported on EVERY rank for the same call, and must leave no collective of that call outstanding on any rank.  The
 * library reacts to a failed collective of the row-sharded solve by making the decision common (one all-reduce of a flag through
 * this hook) and starting over on the replicated solver; a hook that fails on one rank only leaves that rank in the
 * agreement while its peers are still inside the collective that failed for it.  A transport that cannot guarantee this by
 * construction should check that all ranks have entered the SAME call before moving data (tag + count; the CLI's test transport
 * does) and fail on all of them otherwise.  What the library does on its side: every step on which the ranks must agree is
 * time-bounded (120 s) -- a rank that does not get its answer aborts the built-in RCCL communicator (ncclCommAbort; RCCL's
 * asynchronous errors are polled meanwhile), marks the transport of the context dead (every later collective returns
 * FPCA_ECOMM at once) and returns FPCA_ECOMM, for the launcher to end the job.  A hook that BLOCKS inside the caller's own
 * code cannot be bounded from here. */
typedef int (*fpca_allreduce_fn)(void *user, double *dbuf, uint64_t count, void *stream);
int fpca_set_allreduce(fpca_ctx *ctx, fpca_allreduce_fn fn, void *user);
/* ... and, optionally beside it, the caller's all-gather and reduce-scatter (sum) of fp64 on device buffers, ordered on `stream`:
 * `send` holds count_per_rank doubles (all-gather) / nranks * count_per_rank (reduce-scatter), `recv` the opposite; rank r's
 * piece sits at offset r * count_per_rank of the long buffer.  With all three callbacks installed (and fpca_set_rank) the
 * row-sharded solver issues exactly the sequence of collectives it issues over RCCL -- per row chunk, the reduce-scatter of
 * chunk i on a second stream under the K3 of chunk i + 1 -- instead of building both from the sum (twice the bytes). */
/* The all-gather must move its payload as OPAQUE 8-byte words: in the eigensolver's passes on <= 4 slices the words are byte slices
 * of the operand (4 bytes per entry of the block instead of 8), not numbers -- no conversion, no reduction, no NaN canonicalisation. */
typedef int (*fpca_allgather_fn)(void *user, const double *send, double *recv, uint64_t count_per_rank, void *stream);
typedef int (*fpca_reducescatter_fn)(void *user, const double *send, double *recv, uint64_t count_per_rank, void *stream);
int fpca_set_collectives(fpca_ctx *ctx, fpca_allgather_fn allgather, fpca_reducescatter_fn reducescatter, void *user);
/* rank / size of this context among the shards when the transport is a caller's all-reduce (fpca_comm_init_rank sets
 * them itself).  Once they are known and nranks > 1, fpca_pca ROW-SHARDS the eigensolver's N-sized work: the operator becomes
 * all-gather -> K2, K3 -> reduce-scatter (the bytes of the one all-reduce, built from the caller's all-reduce if that is all
 * there is), every rank keeps and orthogonalises N / nranks rows of the Krylov basis, and the only other collective is the
 * all-reduce of the (m+1) b^2 Gram coefficients.  Without this call a hook-only context keeps round 2's replicated solver. */
int fpca_set_rank(fpca_ctx *ctx, int nranks, int rank);
/* data-path collectives this context has issued so far: number of calls and payload bytes (tests, scale model) */
int fpca_collective_stats(const fpca_ctx *ctx, uint64_t *calls, uint64_t *bytes);
/* total SNP count over all shards (the divisor "p", randompca.cpp:183) -- defaults to the shard's P_g */
int fpca_set_total_snps(fpca_ctx *ctx, uint64_t P_total);

/* ------------------------------------------------------------------------------------------------
 * Driver.  Replaces RandomPCA::pca_fast(Data&, block_size, ndim, maxiter, tol, seed, do_loadings)
 * (randompca.cpp:168-218) with a block Krylov-Schur eigensolver whose basis stays in HBM; the projected
 * (m*b x m*b) Rayleigh-Ritz problem is solved on the host.  Convergence rule per Ritz pair is the one the
 * reference's Spectra solver applies: ||A u - theta u|| < tol * max(eps^(2/3), |theta|) for the ndim largest.
 * With fewer than three block widths of samples (N < 3 b; the reference admits ndim <= (min(N,P)-1)/2, flashpca.cpp:623-633)
 * X X' is formed from ceil(N/b) applies on the identity and decomposed directly. */
typedef struct fpca_pca_opts {
   uint32_t struct_size; /* sizeof(fpca_pca_opts) / sizeof(fpca_pca_info) of the header the CALLER was compiled against: written by */
   uint32_t info_size;   /* FPCA_PCA_OPTS_INIT from the caller's own sizeof, checked by fpca_pca (FPCA_EINVAL on a mismatch) */
   int ndim;        /* --ndim (flashpca.cpp:325 default 10) */
   int blockvec;    /* block width b (16, 32, 48 or 64); 0 = automatic: 16 for ndim <= 64, 32 for ndim <= 128, else 64 -- the
                     * narrowest block gives the shortest time to solution (pca_driver.cpp).  ndim may exceed b -- up to the
                     * reference's (min(N,P)-1)/2 --: the solver then carries ceil(ndim/b) + 1 blocks of Ritz vectors across
                     * restarts */
   int maxiter;     /* --maxiter, counted like the reference counts it: restarts of Spectra's ncv = 2 ndim + 1 Lanczos
                     * factorisation (flashpca.cpp:423-433 default 500, randompca.cpp:178 compute(maxiter, tol)).  A restart
                     * re-applies the operator to at most ndim + 1 vectors, so the reference's budget is
                     * 2 ndim + 1 + maxiter (ndim + 1) operator applications; the block solver stops after
                     * ceil(that / 16) block applies -- 16 at a time whatever the width, because a wide block needs about as
                     * many passes as a narrow one (max_applies is the explicit cap in passes) */
   double tol;      /* --tol (flashpca.cpp:440 default 1e-6) */
   int divisor;     /* FPCA_DIVISOR_* (flashpca.cpp:484 default p) */
   int do_loadings; /* --outload given */
   int max_blocks;  /* basis cap in blocks before a thick restart; 0 = automatic */
   int verbose;
   uint64_t seed;   /* start block seed; the reference ignores --seed for PCA (randompca.cpp:168-218) */
   int replicated_solver; /* multi-GPU only: 1 = every rank keeps whole copies of the Krylov basis and repeats the
                     * orthogonalisation (round 2's scheme: one all-reduce per apply); 0 (default) = row-sharded, see fpca_set_rank */
   int max_applies; /* hard cap on block applies, overriding the budget derived from maxiter; 0 = none.  Must allow at least
                     * ceil(ndim / b) of them (FPCA_EINVAL otherwise: fewer basis vectors than wanted pairs) */
   int mixed;       /* exact-integer arithmetic only.  0 = automatic (on), 1 = on, -1 = off.  On: the Krylov passes run on
                     * `cheap_slices` byte slices of the fp64 operand instead of the context's S (4 slices = a 30-bit operand:
                     * ~1e-9 of operator noise, nothing accumulating -- a pass costs about 0.6 of an exact one), and when the
                     * reference's convergence rule holds on those passes the Ritz vectors are put through the EXACT operator
                     * (all S slices) once: the eigenvalues returned are Rayleigh quotients of the exact operator and the rule
                     * ||A u - theta u|| < tol max(eps^(2/3), |theta|) (randompca.cpp:173-178) is judged on exact residuals.  If
                     * it does not hold there, the iteration continues from those vectors with exact passes only. */
   int cheap_slices; /* 0 = automatic (4); 3..S-1 */
   int partial_rows; /* multi-GPU only.  1 = this rank writes ONLY ITS OWN ROWS of U and Px (still N x ndim, leading dimension N):
                     * its row slice of the row-sharded solver, or an even share of the rows under the replicated one -- no gather
                     * of the eigenvector blocks, 1 / nranks of the PCIe traffic per rank.  For callers whose ranks share the
                     * output memory (flashpca --gpus: one mmap'ed region) or gather the slices themselves
                     * (fpca_pca_row_ranges).  0 (default) = every rank that passes U / Px gets all N rows. */
} fpca_pca_opts;

/* fpca_pca_info.solver_path: which layout of the eigensolver's N-sized work the solve ran on */
#define FPCA_SOLVER_SINGLE 0              /* one rank */
#define FPCA_SOLVER_ROWSHARD 1            /* row-sharded: all-gather -> K2, K3 -> reduce-scatter per apply (default for nranks > 1) */
#define FPCA_SOLVER_REPLICATED 2          /* replicated, as asked (replicated_solver = 1, or an all-reduce hook without fpca_set_rank) */
#define FPCA_SOLVER_REPLICATED_SELFTEST 3 /* replicated after the self-test of the row-sharded exchange failed on some rank */
#define FPCA_SOLVER_REPLICATED_FAILURE 4  /* replicated, started over after a collective of the row-sharded solve reported a failure */

typedef struct fpca_pca_info {
   int converged;         /* all ndim pairs met the rule (mixed precision: on residuals of the exact operator) */
   int block_applies;     /* passes over the packed matrix (each = b single-vector operator applications) */
   int vector_ops;        /* block_applies * b  == the reference's nops unit (svdwide.cpp:67) */
   int restarts;          /* thick restarts */
   int blockvec;          /* b actually used */
   double trace;          /* sum X^2 / div (randompca.cpp:205) */
   double max_residual;   /* max_i ||A u_i - theta_i u_i|| / max(eps^(2/3), theta_i) at exit */
   double seconds_apply;  /* device time in the operator (K2+K3+all-reduce) */
   double seconds_ortho;  /* device time in basis orthogonalisation / Ritz rotation */
   double seconds_host;   /* host time in the projected eigenproblem */
   double seconds_total;
   double seconds_download; /* U and Px to the caller's memory (pinned, pipelined; Px = U sqrt(d) fused into the host side) */
   double seconds_post;     /* loadings (one K2 pass per block of eigenvectors) + mean/sd download */
   int cheap_applies;       /* of block_applies: passes on cheap_slices byte slices (0 when mixed precision is off) */
   int cheap_slices;        /* slices of those passes (0: none ran) */
   double seconds_exact;    /* of seconds_apply: the exact passes (verification and whatever followed it) */
   int solver_path;         /* FPCA_SOLVER_*: identical on every rank (a demotion is agreed through one all-reduce of a flag) */
} fpca_pca_info;

/* Defaults of the reference CLI (flashpca.cpp:276-484) + the CALLER's struct sizes, so that fpca_pca can refuse a caller built
 * against another revision of this header: never more than opts_size bytes are written.  C callers use the macro. */
void fpca_pca_init_opts(fpca_pca_opts *opts, size_t opts_size, size_t info_size);
#define FPCA_PCA_OPTS_INIT(o) fpca_pca_init_opts((o), sizeof(*(o)), sizeof(fpca_pca_info))
/* (Revision 4 removed fpca_pca_default_opts, which wrote the LIBRARY's sizeof into the caller's struct: a binary built against an
 * older header now fails to resolve the symbol at load time instead of being overrun by 8 bytes.) */
/* partial_rows = 1: the row ranges [begin, end) of U / Px this rank writes -- ranges[2 i], ranges[2 i + 1], at most max_ranges of
 * them are stored, the count is returned (<= 4; negative FPCA_E* on error).  After an fpca_pca call the answer reflects the
 * layout that call ended on (a demotion to the replicated solver changes the ranges). */
int fpca_pca_row_ranges(fpca_ctx *ctx, const fpca_pca_opts *opts, uint64_t *ranges, int max_ranges);
/* Outputs (host, column-major, caller-allocated; any may be NULL):
 *   U  N x ndim eigenvectors (unit 2-norm, sign arbitrary like Spectra's) ..... RandomPCA::U
 *   d  ndim eigenvalues of X X'/div, descending .............................. RandomPCA::d
 *   Px N x ndim = U diag(sqrt(d)) ............................................. RandomPCA::Px
 *   pve ndim = d / trace ....................................................... RandomPCA::pve
 *   V  P_g x ndim loadings rows of this shard = X_g' U diag(1/sqrt(d))/sqrt(div)  RandomPCA::V (randompca.cpp:191-204)
 *   mean_sd P_g x 2 ............................................................. RandomPCA::X_meansd */
int fpca_pca(fpca_ctx *ctx, const fpca_pca_opts *opts, double *U, double *d, double *Px, double *pve,
             double *V, double *mean_sd, fpca_pca_info *info);

/* Replaces RandomPCA::check(Data&, block_size, evec, eval) (randompca.cpp:663-703):
 * err[j] = || X X' u_j / div - u_j lambda_j ||^2, mse = sum(err)/(N k), rmse = sqrt(mse). */
int fpca_check(fpca_ctx *ctx, const double *evec, int64_t ldu, const double *eval, int k, int divisor,
               double *err, double *mse, double *rmse);

/* ------------------------------------------------------------------------------------------------
 * Per-SNP association with k phenotypes.  Replaces RandomPCA::ucca(Data&) + wilks (randompca.cpp:103-119, 530-625; flashpca --ucca,
 * the R function ucca()): a multivariate ANOVA of every SNP of this shard on the phenotypes, in the style of plink.multivariate.
 * Y is N x k fp64 column-major (leading dimension ldy, NaN = missing), standardised like fpca_create_dense standardises its input
 * (stand_y: any FPCA_STANDARDISE_*).  With x_j the SNP's standardised column as the PCA path builds it,
 *   r2_j = || W' x_j ||^2 / || x_j - mean(x_j) 1 ||^2,  W = (Y - 1 mean(Y)') R^-1,  Y = Q R
 * (exactly the reference's SVD formula), and res (P_g x 3, column-major, leading dimension ldres) receives
 *   R = sqrt(r2),  Fstat = r2 / (1 - r2) (N - k - 1) / k,  P = upper tail of F(k, N - k - 1) at Fstat.
 * A SNP without variance gets NaN in all three; r2 >= 1 gives R = 1, Fstat = +inf, P = 0.  The product X_g' W runs through the
 * context's own arithmetic; a shard's rows are its own SNPs and no collective is issued.  FPCA_EINVAL for k < 1, k > N - 2, a bad
 * ldy / ldres, an unknown stand_y, a rank-deficient standardised Y, or a context whose mean/sd were preloaded. */
int fpca_ucca(fpca_ctx *ctx, const double *Y, int64_t ldy, int k, int stand_y, double *res, int64_t ldres);

/* ------------------------------------------------------------------------------------------------
 * Sparse canonical correlation analysis of the genotypes with k phenotypes.  Replaces RandomPCA::scca(Data&, ...)
 * (randompca.cpp:387-528, norm_thresh :225-245; the R function scca()).  The reference makes two passes over the genotypes per
 * iteration; here fpca_scca_prepare forms C = invdiv X' Yh (P_g x k, fp64) with ONE pass and keeps it on the device, and every
 * fpca_scca_fit -- one per penalty pair of a grid -- iterates on C alone and ends with one pass for Px.
 *
 * fpca_scca_prepare (randompca.cpp:402-415): Y is N x k fp64 column-major (leading dimension ldy, NaN = missing), standardised
 * like fpca_create_dense standardises its input (stand_y: any FPCA_STANDARDISE_*); Yh = that * invdiv, invdiv = 1 / sqrt(N - 1)
 * for divisor FPCA_DIVISOR_N1 and 1 for every other value.  C and Yh stay with the context until the next fpca_scca_prepare or
 * fpca_destroy.  FPCA_ENOMEM (with the size in the message) when C does not fit; FPCA_EINVAL for k < 1, k > 3840, a bad ldy, an
 * unknown stand_y, or a context that is one shard of several (a communicator, an all-reduce hook, fpca_set_rank with nranks > 1:
 * the normalisation of u spans all SNPs). */
int fpca_scca_prepare(fpca_ctx *ctx, const double *Y, int64_t ldy, int k, int stand_y, int divisor);
/* fpca_scca_fit (randompca.cpp:417-528): from V0 (k x ndim, leading dimension ldv0, required), for each dimension j
 *     u <- C v_j, sequential Gram-Schmidt against U[:, <j], norm_thresh(u, lambda1)
 *     v <- C'u,   sequential Gram-Schmidt against V[:, <j], norm_thresh(v, lambda2)
 * until iter > 0 and max |u - u_old| < tol and max |v - v_old| < tol, at most maxiter iterations; d_j = u'C v.
 * Outputs (host, column-major, caller-allocated; any may be NULL): U P_g x ndim, V k x ndim, d ndim, Px = invdiv X U and
 * Py = Yh V (N x ndim each), *converged, iters[ndim] (the reference's "dim j finished in ... iterations"), nzero_x / nzero_y[ndim]
 * (non-zeros of every column of U / V, randompca.cpp:509-510), *status = FPCA_SCCA_*.
 * The call SUCCEEDS with *converged = 0 when
 *   - maxiter is reached in dimension j (FPCA_SCCA_MAXITER): its current u, v stay in U, V, d_j = 0, no later dimension is
 *     attempted (U zero, V as in V0, d zero there, iters zero); Px and Py are computed from what is there;
 *   - all of u (or v) is below tol in absolute value after norm_thresh (FPCA_SCCA_LAMBDA1_TOO_LARGE / _LAMBDA2_): the finished
 *     dimensions are kept, column j and the later ones are U zero, V as in V0, d zero.
 * FPCA_EINVAL: no fpca_scca_prepare before, ndim outside 1 .. min(N, P_g, k), lambda1 / lambda2 < 0, tol <= 0, maxiter < 1, V0
 * NULL or not finite, a leading dimension too small, a context that is one shard of several. */
#define FPCA_SCCA_OK 0
#define FPCA_SCCA_MAXITER 1
#define FPCA_SCCA_LAMBDA1_TOO_LARGE 2
#define FPCA_SCCA_LAMBDA2_TOO_LARGE 3
int fpca_scca_fit(fpca_ctx *ctx, double lambda1, double lambda2, int ndim, int maxiter, double tol, const double *V0, int64_t ldv0,
                  double *U, int64_t ldu, double *V, int64_t ldv, double *d, double *Px, int64_t ldpx, double *Py, int64_t ldpy,
                  int *converged, int *iters, int64_t *nzero_x, int64_t *nzero_y, int *status);

/* ------------------------------------------------------------------------------------------------
 * K-fold cross-validation of the SCCA penalties on the packed genotypes.  Replaces the R function cv.scca() (flashpcaR/R/scca.R:410-557),
 * which accepts numeric matrices only; here the packed matrix is the supported input and is never copied: ONE pass counts the
 * genotypes of every fold, and per fold f (T_f = the samples outside it, H_f = those in it)
 *   - the per-SNP mean / sd over T_f (the rule of the PCA path, exact integer sums) standardise ALL N rows, the held-out rows
 *     included, as a projection standardises new samples; Y is standardised on T_f by stand_y the same way (NaN imputed as there);
 *   - C_f = invdiv_f^2 X[T_f]' Y[T_f] from one K2 pass, invdiv_f = 1 / sqrt(|T_f| - 1) for FPCA_DIVISOR_N1, else 1;
 *   - if warm_lambda >= 0 the fit at (warm_lambda, warm_lambda) from V0_f gives the V every grid fit of the fold starts from,
 *     converged or not (scca.R:474-481: 1e-12); warm_lambda < 0: they start from V0_f;
 *   - the n1 x n2 fits of fpca_scca_fit, edge rules unchanged;
 *   - xpred[H_f] = X[H_f] U and ypred[H_f] = Y[H_f] V (scca.R:504-505; no invdiv), NaN where the model did not converge.
 * corr is the Pearson correlation of xpred and ypred over all N samples pooled (scca.R:525-536; NaN when a row is NaN or a variance
 * is zero), nzero_x / nzero_y the mean over the folds of the non-zero counts of U / V (scca.R:516-523).  best_corr is the largest finite
 * corr of dimension opt_dim (1-based), best_lambda1 / best_lambda2 its penalties, ties in which()'s order: lambda1's index fastest,
 * first hit (scca.R:538-547); all three NaN when no cell is finite -- the call still succeeds.
 * Inputs: Y N x k column-major (ldy); fold[N] in 0 .. nfolds - 1, 2 <= nfolds <= 64 (a fold without samples trains on everything and
 * predicts nothing, as R's loop does); lambda1[n1], lambda2[n2]; V0: one k x ndim matrix per fold, matrix f at V0 + f * v0_stride,
 * leading dimension ldv0 (v0_stride 0: one matrix for every fold).
 * Outputs (host, caller-allocated, any may be NULL), C index order, i over lambda1, j over lambda2, q over dimensions:
 *   corr, nzero_x, nzero_y [ndim][n1][n2] ....... (q * n1 + i) * n2 + j
 *   converged [nfolds][n1][n2], iters [nfolds][n1][n2][ndim], warm_iters [nfolds][ndim] (zero without a warm start)
 *   xpred, ypred: N x (n1 n2 ndim) column-major, leading dimension N, column (i * n2 + j) * ndim + q -- downloaded only if asked for.
 * The context's mean / sd / table are swapped per fold and restored on every way out, errors included (also a standardisation
 * preloaded with fpca_set_meansd); the state of an earlier fpca_scca_prepare is RELEASED: fpca_scca_fit needs a new prepare afterwards.
 * FPCA_EINVAL: what fpca_scca_prepare / fpca_scca_fit refuse; a dense context (fpca_create_dense keeps only its standardised matrix);
 * nfolds outside 2 .. 64; a fold id >= nfolds; a training set of fewer than 2 samples; ndim outside 1 .. min(smallest |T_f|, P_g, k);
 * opt_dim outside 1 .. ndim; a negative or non-finite penalty.  FPCA_ENOMEM (with the size in the message) when C, xpred / ypred or a
 * workspace does not fit. */
int fpca_scca_cv(fpca_ctx *ctx, const double *Y, int64_t ldy, int k, const uint8_t *fold, int nfolds, const double *lambda1, int n1,
                 const double *lambda2, int n2, int ndim, int stand_y, int divisor, int maxiter, double tol, const double *V0, int64_t ldv0,
                 int64_t v0_stride, double warm_lambda, int opt_dim, double *corr, double *nzero_x, double *nzero_y, int *converged,
                 int *iters, int *warm_iters, double *best_lambda1, double *best_lambda2, double *best_corr, double *xpred, double *ypred);

#ifdef __cplusplus
}
#endif
#endif /* FPCA_H */
