/*
 * include/fpca_debug.h -- measurement hooks and hardware diagnostics of libfpca.so.
 *
 * NOT part of the drop-in boundary: a maintainer binding the reference's operator seam (svdwide.h:77-81) or driver
 * (randompca.h:77-80) needs include/fpca.h only.  What is declared here serves bench.py (HIP-event timing of the kernels
 * inside the timed region), the kernel parity tests (operand-layout probes, the eigensolver's K4 helpers on caller data) and
 * the lab scripts under scripts/ (MFMA stream rates, workgroup placement).  Same conventions as fpca.h.
 */
#ifndef FPCA_DEBUG_H
#define FPCA_DEBUG_H

#include "fpca.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Measurement hooks (bench.py): run `steps` block-applies of width b on device-resident random blocks after
 * `warmup` untimed ones; HIP events on the context's stream bracket every kernel.  Times in milliseconds. */
typedef struct fpca_bench_result {
   double ms_total;      /* wall (event) time of the timed region, all steps */
   double ms_xt;         /* average per step in K2 (xt_b), incl. its split-K reduce */
   double ms_x;          /* average per step in K3 (x_t), incl. its split-K reduce */
   double ms_allreduce;  /* average per step in the all-reduce (0 for one rank) */
   double flops_per_step;           /* 4 N P_g b */
   double packed_bytes_per_step;    /* 2 ceil(N/4) P_g */
   double ms_gemm_xt;    /* average per step of the K2 GEMM kernel launch alone */
   double ms_gemm_x;     /* average per step of the K3 GEMM kernel launch alone */
} fpca_bench_result;
int fpca_bench_apply(fpca_ctx *ctx, int b, int steps, int warmup, fpca_bench_result *res);
/* Live profiling of caller-driven applies: between fpca_profile_begin and fpca_profile_end every
 * fpca_apply_xxt_dev call (up to max_steps of them) records HIP events on its stream around K2, K3 and the
 * all-reduce; fpca_profile_end synchronises and returns the per-step averages over the recorded calls
 * (ms_total = sum of all recorded steps; *nsteps = number recorded). */
int fpca_profile_begin(fpca_ctx *ctx, int max_steps);
/* Eight in-stream events per apply are not free at small sizes (0.62 vs 0.53 ms per apply at 50,000 x 20,000): with
 * stride > 1 only every stride-th apply of the profiled span carries them, the others run exactly as the solver runs
 * them.  Default 1. */
int fpca_profile_sample_every(fpca_ctx *ctx, int stride);
int fpca_profile_end(fpca_ctx *ctx, int b, fpca_bench_result *res, int *nsteps);
/* time the one-off statistics pass (K1) the same way: milliseconds per launch, bytes read */
int fpca_bench_stats(fpca_ctx *ctx, int reps, double *ms_per_launch, double *bytes_per_launch);

/* diagnostic: D(16x16, row-major) = A(16x4) B(4x16) through v_mfma_f64_16x16x4_f64 with the lane->operand mapping the
 * kernels assume; host pointers.  Used by tests/test_gpu_kernels.py as a guard on the hardware layout. */
int fpca_debug_mfma_probe(const double *A, const double *B, double *D);
/* diagnostic: D(32x32 int32, row-major) = A(32x32 int8, row-major) * Bt(32x32 int8, row j = column j of B)' through
 * v_mfma_i32_32x32x32_i8 with the lane->operand mapping of kernels_i8.hip; host pointers */
int fpca_debug_mfma_i8_probe(const int8_t *A, const int8_t *Bt, int32_t *D);
/* diagnostic: the two int8 instructions of the GEMM with their operands as above (exchanged = 0) or exchanged, stored through
 * the register map of exchanged = 0 -- exchanged, D comes back transposed.  shape 32: v_mfma_i32_32x32x32_i8, A, Bt and D as
 * above; shape 16: v_mfma_i32_16x16x64_i8, A(16x64) Bt(16x64)' = D(16x16).  Any other shape: FPCA_EINVAL.  Host pointers. */
int fpca_debug_mfma_i8_ports(int shape, int exchanged, const int8_t *A, const int8_t *Bt, int32_t *D);
/* diagnostic: sustained rate (TFLOP/s) of a pure v_mfma_f64_16x16x4_f64 stream with `waves_per_simd` (1..8) resident
 * waves per SIMD and no memory traffic; pattern 0..3 selects the operand-register sharing pattern (kernels.hip).  The
 * practical ceiling to read the GEMM kernels' roofline fraction against (72-74 TFLOP/s at 2 waves/SIMD vs 78.6 datasheet).
 * pattern 10 / 11: v_mfma_i32_32x32x32_i8 in TOP/s with zero / pseudo-random operands.  12..17: the same stream with the two
 * operand ports filled differently (source A / source B): 12 random / zero, 13 zero / random, 14 genotype bytes {0, 1, 2} / random,
 * 15 random / genotype bytes; 16 as 14 with B changing every instruction and A every second (14, 15, 17: the reverse; 17 repeats
 * 14's stream).  Any other pattern: FPCA_EINVAL. */
int fpca_debug_mfma_peak(int waves_per_simd, int iters, int pattern, double *tflops);
/* diagnostic (tests/test_gpu_kernels.py): the K4 helpers the eigensolver runs on its HBM-resident basis, on caller data and
 * through the very backend object the solver drives (HipBackend::gram incl. its split-K plane reduction, HipBackend::gemm).
 * V: N x (nq b) fp64 column-major with leading dimension N, basis block q = columns [q b, (q+1) b); W: N x b.
 *   C_gram (may be NULL): [q][p][c] = sum_s V_q[s][p] W[s][c]                       nq b b doubles
 *   Out (may be NULL), N x b: (use_init ? W : 0) + sum_q V_q C_in[q]                C_in: [q][p][c], nq b b doubles
 *   G_out (may be NULL): [p][c] = sum_s Out[s][p] Out[s][c], from the SAME launch that writes Out (HipBackend::gemm_gram)  b b doubles
 * fpca_debug_k4, _k4_fused and _k4_inplace first fill the context's split-K partial buffer, at the size earlier calls left it, with
 * NaNs: from the second call of a kind on a context on, a partial plane that a kernel does not write shows in the result. */
int fpca_debug_k4(fpca_ctx *ctx, int b, int nq, const double *V, const double *W, double *C_gram, const double *C_in, int use_init,
                  double *Out, double *G_out);
/* round 6: the first Gram-Schmidt projection's update and the second projection's Gram matrices from ONE pass over the basis
 * (HipBackend::gemm_gramvw, k_update_gram16): Out (may be NULL) = W + sum_q V_q C_in[q]; Cg: [q][p][c] = sum_s V_q[s][p] Out[s][c] for
 * q < nq, Cg[nq] = Out' Out -- (nq + 1) b b doubles; and its launch time (kernel + plane reduction) on nq random blocks */
int fpca_debug_k4_fused(fpca_ctx *ctx, int b, int nq, const double *V, const double *W, const double *C_in, double *Out, double *Cg);
int fpca_debug_k4_fused_bench(fpca_ctx *ctx, int b, int nq, int reps, double *ms_fused);
/* HipBackend::gemm / gemm_gram with the output block among the operands, in the forms the solver calls (V, W, C_in as above):
 *   mode 0: Out = W + sum_q V_q C_in[q], written over W (out = init)
 *   mode 1: Out = sum_q V_q C_in[q], written over V_{nq-1} (out = the last operand block, no init; W may be NULL)
 *   mode 2: mode 1 through gemm_gram; G_out: [p][c] = sum_s Out[s][p] Out[s][c], b b doubles (G_out must be NULL in modes 0 and 1)
 * Out, N x b: the overwritten block, downloaded after the call. */
int fpca_debug_k4_inplace(fpca_ctx *ctx, int b, int nq, const double *V, const double *W, const double *C_in, int mode, double *Out,
                          double *G_out);
/* launch times of the K4 kernels on nq device-resident random basis blocks of this context's height: ms per Gram (kernel + plane
 * reduction) and per block GEMM (Out = Init + sum_q V_q C_q) */
int fpca_debug_k4_bench(fpca_ctx *ctx, int b, int nq, int reps, double *ms_gram, double *ms_gemm);

/* diagnostic (tests/test_gpu_fp_splits.py): the split-K plans fpca_apply_xt / fpca_apply_x / fpca_apply_xxt launch on this context's
 * fp64, fp32 or dense kernels for a block of b columns (1 .. 64, rounded up to 16 as the operator does), from the very host
 * functions the launches take their numbers from; nothing runs on the device.
 *   out[0..2]: X'B -- splits, chunks per split as handed to the kernel, chunks in all;   out[3..5]: the same for X T.
 * Split i owns chunks [i out[1], min((i + 1) out[1], out[2])): the last one may be short, and trailing ones empty. */
int fpca_debug_fp_plan(fpca_ctx *ctx, int b, int out[6]);
/* fills the operator's split-K partial buffer and its T buffer, at the capacity earlier calls left them, with NaNs on the context's
 * stream: after one product has sized them, a plane or tile that the next product does not write shows in its result */
int fpca_debug_poison_partials(fpca_ctx *ctx);

/* diagnostic (tests/test_gpu_missing_gathers.py): the index lists of the missing calls that the exact-integer mode's list routes
 * (fpca_missing_mode 3 and 4) gather over, for blocks of b columns (16, 32 or 64).  Makes the lists ready the way the operator does
 * before its first product on such a route and downloads them; FPCA_EINVAL if the context is not on a list route for this b.
 *   by_sample 0: one list per SNP, the samples with a missing call, ascending;  ptr_out: nsnps + 1 entries
 *   by_sample 1: one list per sample, the SNPs with a missing call, ascending;  ptr_out: nsamples + 1 entries
 * List r is idx_out[ptr_out[r] .. ptr_out[r + 1]).  *nnz: the length of idx; idx_out (may be NULL, as may ptr_out) is written if idx_cap
 * >= *nnz, else FPCA_EINVAL with *nnz set.  On the hybrid route the lists are those of that route's view of the matrix: the SNPs whose
 * indicator rows go to the matrix cores have empty lists and appear in no sample's list. */
int fpca_debug_missing_lists(fpca_ctx *ctx, int b, int by_sample, uint32_t *ptr_out, uint32_t *idx_out, uint64_t idx_cap, uint64_t *nnz);
/* diagnostic (tests/test_gpu_missing_gathers.py): the gather-sum kernels of those routes on caller data, host pointers, no context:
 *   out[r][c] = (init ? init[r][c] : 0) + sum over t in [ptr[r], ptr[r + 1]) of V[idx[t]][c] (rowscale ? rowscale[idx[t]] : 1),  r < nrec,
 * and init or 0 for nrec <= r < rows_out; row-major, b = 16, 32 or 64 columns.  ptr: nrec + 1 entries from 0 to nnz, not decreasing; idx:
 * nnz entries below v_rows (checked before anything is launched).  use_f32 0: V is v_rows x b fp64, rowscale (may be NULL) v_rows
 * factors, colw NULL.  use_f32 1: V is fp32 and the sums are multiplied by 32 colw[c], as for the rows the slicing pass leaves; no
 * rowscale.  short_lists and avg_len go to the launch as the operator passes them (K2: 0, 0; K3: 1, listed calls per sample) and choose
 * the kernel; *variant reports it: 1 one wave per row, 2 the same with batched index reads, 3 several rows per wave. */
int fpca_debug_gather(int b, int use_f32, const uint32_t *ptr, const uint32_t *idx, uint64_t nnz, const void *V, uint64_t v_rows,
                      const double *rowscale, const double *colw, const double *init, uint64_t nrec, uint64_t rows_out, int short_lists,
                      double avg_len, double *out, int *variant);

/* diagnostic (tests/test_gpu_i8_slices.py): the kernels that cut an fp64 operand into the int8 digit planes of the exact-integer
 * arithmetic (csrc/kernels_i8.hip, top), on caller data, host pointers, no context -- through the host launchers the operator calls, in
 * the operator's order.  V: rows_pad x b fp64 row-major (b = 16, 32, 48 or 64; rows_pad a multiple of 16 up to 2^20); rows >= `rows`
 * are not read: the device block holds zeros there, as the operator's blocks do.  S = 2 .. 8 slices.  rowscale0 / rowscale1 (may be
 * NULL; `rows` factors each): none = one operand V; rowscale0 alone = one operand V diag(rowscale0); both = the two operands of X T from
 * one pass (route 0 only), the second answered in out1.  peers (may be NULL): n_peers x 64 column maxima standing for the other ranks'
 * answers to the small all-gather; one operand only.
 *   route 0, the operator's own slicing:  maxbits zeroed; i8_colmax over `rows`; with peers i8_maxbits_fold + i8_maxbits_set over
 *            [own; peers]; i8_slice.
 *   route 1, the row-sharded exchange:    maxbits zeroed; i8_colmax over rows_pad; i8_maxbits_fold; i8_maxbits_set over [own; peers];
 *            i8_slice_rows over rows_pad rows -> Qrm; i8_unpack_slices(Qrm, rows_valid, the copies); i8_dequant_rows(Qrm) once per
 *            requested output.  S b <= 512.
 * Before the launches Q (all nsc_pad rows) and Qrm are filled with the byte 0x55, colw (all nsc_pad entries) and every requested copy with
 * NaNs (all bits set), and colsum with zeros: what a kernel does not write, or writes where it should not, shows.
 * Every member of fpca_debug_slices_out is a host buffer or NULL (not wanted); colsum, copy32, copy64, dq32 and dq64 are also the switch:
 * the kernels are asked for what is not NULL.  At most one of copy32 / copy64 per operand, and fp32 rows with S <= 4 only, as the operator
 * asks.  *nsc_pad (may be NULL): the padded number of slice-columns, gemm_i8_nsc_pad(S, b); fpca_debug_i8_nsc_pad returns it alone, for
 * sizing Q and colw, and touches no device.
 * FPCA_EINVAL, with a message that names the argument, before anything touches the device: route not 0 / 1; b or S outside their sets;
 * rows_pad not a multiple of 16 in 16 .. 2^20; rows or rows_valid > rows_pad; V or out0 NULL; rowscale1 without rowscale0, or without
 * out1, or out1 without it; rowscale1 or S b > 512 on route 1; n_peers outside 0 .. 63 or not matching peers; peers with two operands;
 * both copies, or fp32 rows with S > 4; Qrm / dq32 / dq64 on route 0; a non-finite entry in V (rows < `rows`), a row scale or peers, or
 * a negative one in peers. */
typedef struct fpca_debug_slices_out {
   double *colmax;        /* [64] the operand's own column maxima, shards folded (route 0 with one operand and route 1: by i8_maxbits_fold) */
   uint64_t *maxbits_own; /* [8][64] the sharded maxima as i8_colmax left them, bit patterns of doubles */
   uint64_t *maxbits;     /* [8][64] the same as the slicing kernels read them: after i8_maxbits_set where it ran */
   int8_t *Q;             /* [nsc_pad][rows_pad] */
   int8_t *Qrm;           /* [rows_pad][S b], route 1 */
   double *colw;          /* [nsc_pad] */
   int64_t *colsum;       /* [8][640] per shard: the sum over the shards is the column sum */
   float *copy32;         /* [rows_pad][b] from i8_slice (route 0) or i8_unpack_slices (route 1: rows < rows_valid) */
   double *copy64;        /* the same in fp64 */
   float *dq32;           /* [rows_pad][b] from i8_dequant_rows, route 1 */
   double *dq64;
} fpca_debug_slices_out;
int fpca_debug_i8_nsc_pad(int S, int b, int *nsc_pad);
int fpca_debug_i8_slices(int route, int b, int S, uint64_t rows, uint64_t rows_pad, uint64_t rows_valid, const double *V, const double *rowscale0,
                         const double *rowscale1, const double *peers, int n_peers, fpca_debug_slices_out *out0, fpca_debug_slices_out *out1,
                         int *nsc_pad);
/* diagnostic (tests/test_gpu_i8_planes.py): the table of int8 GEMM kernel instances (csrc/kernels_i8.hip, I8Instances), host only, no
 * device involved.  keys (may be NULL when cap is 0): cap rows of six int32 -- two operands (0 / 1), mode (0 both matrices, 1 the same
 * skipping empty blocks of E, 2 G.M alone), nt (column tiles per workgroup), half tile (0 / 1), tile rows (128 / 256 / 512), band-tiled
 * `packed` (0 / 1) -- in the table's order; min(*count, cap) rows are written.  *count: the number of instances.  A test that launches
 * the GEMM under FPCA_I8_VERBOSE can rebuild the same six numbers from the plan and launch lines and hold its cases to the whole table. */
int fpca_debug_i8_instances(int32_t *keys, int cap, int *count);
/* diagnostic (tests/test_gather_blocks_cpu.py): the grid of a missing-call gather that runs on the side stream beside an int8 GEMM
 * (csrc/missing_kernels.hip, gather_blocks_beside), host only, no device involved.  One workgroup of the GEMM: gemm_waves waves,
 * gemm_vgprs registers per lane (as the compiler asks for them), gemm_lds bytes of LDS; gather_vgprs: registers per lane of the gather
 * kernel (256-thread blocks, no LDS); ncu: compute units.  *limit: ncu times the blocks that stay resident on a CU beside the GEMM
 * workgroups sharing it, at least ncu.  *grid_side / *grid_inline: the blocks of a launch of the one-wave-per-row kernels over rows_out
 * rows on the side stream (under that limit) and inline (four rows a block, at most 65536 blocks).  FPCA_EINVAL unless gemm_waves is
 * 1 .. 16, the register counts 1 .. 512, gemm_lds 0 .. 163840, ncu 1 .. 4096 and rows_out >= 1. */
int fpca_debug_gather_blocks(int gemm_waves, int gemm_vgprs, int gemm_lds, int gather_vgprs, int ncu, uint64_t rows_out, uint32_t *limit,
                             uint32_t *grid_side, uint32_t *grid_inline);

/* diagnostic (tests): the F tail of fpca_ucca, from the host build of the same source the finishing kernel runs (no device
 * involved): F = r2 / (1 - r2) (n - k - 1) / k and P = upper tail of F(k, n - k - 1) at F = I_{1 - r2}((n - k - 1) / 2, k / 2).
 * FPCA_EINVAL unless k >= 1 and n >= k + 2. */
int fpca_debug_f_sf(double r2, uint64_t n, int k, double *F, double *P);
/* diagnostic (tests/test_gpu_f_tail.py): the same from the DEVICE build, on the current device: one small kernel, one lane per value
 * of r2[count], f_sf called as the finishing kernel of fpca_ucca calls it; F[count], P[count] out.  Refuses what fpca_debug_f_sf
 * refuses; count = 0 returns at once. */
int fpca_debug_f_sf_dev(const double *r2, uint64_t count, uint64_t n, int k, double *F, double *P);
/* diagnostic (tests/test_gpu_scca_widths.py): the largest k fpca_scca_prepare accepts, the bytes of LDS the k-sized kernel of
 * fpca_scca_fit needs at it (static arrays plus two vectors of k_pad doubles), and what `device` allows one workgroup
 * (hipDeviceAttributeMaxSharedMemoryPerBlock): a property query, nothing is launched. */
int fpca_debug_scca_lds(int device, int *max_k, int *need_at_max_k, int *per_workgroup);
/* diagnostic (tests, scripts/cv_scca_measure.py): the one pass of fpca_scca_cv over the packed stream.  fold[N] in 0 .. nfolds - 1
 * (2 <= nfolds <= 64); counts (may be NULL): uint32 [nfolds][P_g][3], the samples of each fold with dosage 0, 1, 2 (the missing calls
 * are the fold's size minus the three); mean_sd (may be NULL): P_g x 2 like fpca_stats, the mean / sd over the samples OUTSIDE fold
 * which_fold as fpca_scca_cv installs them for that fold.  The context is not changed. */
int fpca_debug_fold_stats(fpca_ctx *ctx, const uint8_t *fold, int nfolds, uint32_t *counts, int which_fold, double *mean_sd);
/* diagnostic (tests): the QC rule of fpca_snp_qc on caller arrays, no context and no device involved: mean[P] and n_missing[P] as K1
 * leaves them, N samples; keep[P] in and out, as for fpca_snp_qc.  FPCA_EINVAL for the thresholds fpca_snp_qc refuses. */
int fpca_debug_snp_qc_rule(const double *mean, const uint32_t *n_missing, uint64_t N, uint64_t P, double min_maf, double max_missing,
                           uint8_t *keep, uint64_t *n_kept);
/* time the record gather of fpca_create_snp_subset alone (scripts/snp_subset_measure.py): the destination and the index list are
 * allocated before the clock starts; one untimed launch, then `reps` timed ones on src's stream.  Milliseconds per launch and the bytes
 * one launch moves (2 pitch P_kept: read and written).  src is not changed. */
int fpca_debug_snp_subset_bench(fpca_ctx *src, const uint8_t *keep, int reps, double *ms_per_launch, double *bytes_per_launch);
/* diagnostic (tests): the pruning rule of fpca_ld_prune on caller arrays, no context and no device involved.  bits: the band bitmap,
 * P rows of ceil((window - 1) / 32) uint32 words, bit d - 1 of row i set when r2(i, i + d) is above the threshold (bits of pairs past
 * the last SNP or across a chromosome boundary are ignored); totals: uint64 [P][3] = calls, sum x, sum x^2 over the SNP's own calls;
 * maf[P]; chrom[P] or NULL; keep[P] in and out.  FPCA_EINVAL for the window / step fpca_ld_prune refuses. */
int fpca_debug_ld_prune_rule(const uint32_t *bits, uint64_t P, uint32_t window, uint32_t step, const uint64_t *totals, const double *maf,
                             const uint32_t *chrom, uint8_t *keep, uint64_t *n_kept);
/* time the bitmap kernel of fpca_ld_prune alone (scripts/ld_prune_measure.py) over all SNPs of the context at threshold r2 = 0.05:
 * per-SNP totals and the bitmap are ready before the clock starts; one untimed launch, then `reps` launches with a pair of HIP events
 * around each, ms[reps].  *macs (may be NULL): int8 multiply-accumulates one launch issues (32 x 32 x 32 per MFMA, pad samples and
 * pad SNPs included). */
int fpca_bench_ld(fpca_ctx *ctx, uint32_t span, int reps, double *ms, double *macs);
/* diagnostic (tests): the rule of fpca_king_cutoff on caller arrays, no context and no device involved.  (i[k], j[k]), k < n_pairs: the
 * pairs above the threshold, in any order, samples below N; keep[N] in and out.  FPCA_EINVAL for a pair outside the N samples. */
int fpca_debug_king_rule(const uint32_t *i, const uint32_t *j, uint64_t n_pairs, uint64_t N, uint8_t *keep, uint64_t *n_kept);
/* time the pair kernel of fpca_king_pairs alone (scripts/king_measure.py) over the whole triangle at thr = 0.0884, no keep: the
 * sample-major copy and the per-sample totals are ready before the clock starts; one untimed pass, then `reps` passes (every launch of the
 * triangle) with a pair of HIP events around each, ms[reps].  *macs (may be NULL): int8 multiply-accumulates one pass issues (32 x 32 x
 * 32 per MFMA, pad SNPs included). */
int fpca_bench_king(fpca_ctx *ctx, int reps, double *ms, double *macs);
/* the same for the pair kernel of fpca_king_related (scripts/king_rel_measure.py), at thr = 0.0884, min_shared = 0, no keep: seven
 * products per pair of 32-sample blocks on the general path, two where neither block has a missing call. */
int fpca_bench_king_rel(fpca_ctx *ctx, int reps, double *ms, double *macs);
/* the same for the census kernel of fpca_pcair_king (k_king_census, scripts/pcair_measure.py): the whole triangle at kin_thr = 2^-5.5,
 * div_thr = -2^-5.5, no keep, no exclusion list, a pair list of 2^20 slots; the counter and both count arrays are cleared before each
 * pass, outside the clock.  k_king's products, so fpca_bench_king's MAC count applies. */
int fpca_bench_king_census(fpca_ctx *ctx, int reps, double *ms);
/* time the FP64 Gram kernel of the relationship matrix alone (k_grm_dot, scripts/grm_measure.py) over the whole lower triangle, slab by slab as
 * fpca_grm_tri launches it: the sample-major copy, the totals and the slab scratch are ready before the clock starts; one untimed pass,
 * then `reps` passes with a pair of HIP events around each, ms[reps].  *flops (may be NULL): floating-point operations one pass issues
 * (2 x 32 x 32 x 4 pitch per 32 x 32 block of pairs on or below the diagonal, pad SNPs included).  Test build with FPCA_GRM_BENCH_SHARED=1:
 * the shared-call count kernel (k_grm_shared) is timed instead. */
int fpca_bench_grm(fpca_ctx *ctx, int reps, double *ms, double *flops);
/* time the Gram kernel of PC-Relate alone (k_pcr_gram, scripts/pcrelate_measure.py) over the whole lower triangle, slab by slab and panel by
 * panel as fpca_pcrelate_tri launches it, on a model of npc columns made up here that leaves every call of a live SNP usable: the
 * sample-major copy, the slab scratch and a panel (the last the untimed pass of both kernels built) are ready before the clock starts;
 * then `reps` passes with a pair of HIP events around each, ms[reps].  *flops (may be NULL): floating-point operations one pass issues,
 * both Grams counted (2 x 2 x 32 x 32 x round_up(P_g, 512) per 32 x 32 block of pairs on or below the diagonal).  Test build with
 * FPCA_PCR_BENCH_OPERANDS=1: the operand kernel (k_pcr_operands), every launch of the triangle, is timed instead. */
int fpca_bench_pcrelate(fpca_ctx *ctx, int npc, int reps, double *ms, double *flops);
/* fpca_bench_pcrelate for PC-Relate's IBD sharing (scripts/pcrelate_ibd_measure.py): the three instances of k_pcr_ibd alone over the whole
 * lower triangle, slab by slab and panel by panel as fpca_pcrelate_ibd_tri launches them, on the same made-up model; the sample-major copy,
 * the slab scratch and the three panels (the last the untimed pass of all kernels built) are ready before the clock starts.  *flops (may be
 * NULL): seven products counted (7 x 2 x 32 x 32 x round_up(P_g, 512) per 32 x 32 block of pairs on or below the diagonal).  Test build
 * with FPCA_PCR_BENCH_OPERANDS=1: the operand kernel (k_pcr_ibd_operands), every launch of the triangle, is timed instead. */
int fpca_bench_pcrelate_ibd(fpca_ctx *ctx, int npc, int reps, double *ms, double *flops);
/* diagnostic (tests): the rules of fpca_sample_qc / fpca_snp_qc_samples on caller arrays, no context and no device involved.  counts:
 * uint32 [N][4] / [P][4] by raw code; n_snps: the SNPs the per-sample counts were taken over; n: the samples the per-SNP counts were taken
 * over; p_hwe[P]: the p-values, read only when min_hwe_p > 0 (may be NULL otherwise); samples[N] / keep[P] in and out.  FPCA_EINVAL for
 * the thresholds the entry points refuse, n_snps == 0 and n == 0. */
int fpca_debug_sample_qc_rule(const uint32_t *counts, uint64_t n_snps, uint64_t N, double max_missing, uint8_t *samples, uint64_t *n_kept);
int fpca_debug_snp_qc_counts_rule(const uint32_t *counts, const double *p_hwe, uint64_t n, uint64_t P, double min_maf, double max_missing,
                                  double min_hwe_p, uint8_t *keep, uint64_t *n_kept);
/* time the three kernels of the genotype census alone (scripts/qc_measure.py), all samples and all SNPs: scratch is ready before the clock
 * starts; one untimed launch, then `reps` timed ones.  ms[3]: milliseconds per launch of the per-SNP count pass, of the per-sample count
 * pass (with the clear of its count planes) and of the HWE kernel on the counts of the first.  *hwe_steps (may be NULL): recurrence steps
 * one HWE launch makes at most. */
int fpca_bench_qc(fpca_ctx *ctx, int reps, double *ms, double *hwe_steps);

/* diagnostic (tests/test_synth_cpu.py, tests/test_gpu_synth.py): the synthetic genotype model of fpca_create_synthetic_model on the
 * HOST, from the functions of csrc/synth.hpp alone -- no device involved, no HIP call made.  Writes records [snp_begin, snp_begin + P_g)
 * of the (N, seed, model) matrix into out, (N + 3) / 4 bytes each, .bed body layout.  The pad samples of a record's last byte are code
 * 01, as the kernel writes them into the resident matrix (fpca_download_packed hands them out as 00, as PLINK writes them: compare
 * after clearing them).  fixed (may be NULL): the five integers the model's doubles are reduced to before anything is
 * generated -- fst_fp (16.16), miss_thr (0.16), conc_fp (0.16), med_q32 (0.32), sig2_fp (16.16) -- by the very function the device
 * entry takes them from.  Refuses what fpca_create_synthetic_model refuses of a model, N outside 1 .. 2^40 - 1, and a NULL out. */
int fpca_debug_synth_host(uint64_t N, uint64_t snp_begin, uint64_t P_g, uint64_t seed, const fpca_synth_model *model, uint8_t *out,
                          uint64_t fixed[5]);

/* diagnostic (tests/test_gpu_scratch.py), builds with -DFPCA_TEST_HOOKS only: what the entry points hold for the length of one call --
 * device memory, pinned host memory, events (csrc/dev_scratch.hpp) -- is counted, and one acquisition can be made to fail.
 *   fpca_debug_scratch_live     out[0..2] = live device allocations, pinned allocations, events made through those owners: equal before
 *                               and after a call that leaks nothing, whichever way it ends.
 *   fpca_debug_scratch_fail_at  the n-th acquisition from now (1 = the next; allocation or event alike) throws FPCA_ENOMEM as if the
 *                               device were full, before the runtime is asked for anything; the countdown then disarms.  n = 0 disarms.
 * In the product build both return FPCA_EINVAL with a message that says so and do nothing: no switch changes what it computes. */
int fpca_debug_scratch_live(uint64_t out[3]);
int fpca_debug_scratch_fail_at(uint64_t n);
/* diagnostic (tests/test_gpu_i8_cheap_passes.py), builds with -DFPCA_TEST_HOOKS only: the slice count of the context's NEXT products in
 * the exact-integer arithmetic -- fpca_apply_xt, fpca_apply_x, fpca_apply_xxt run on Sc slices inside the context made for more, the state
 * the eigensolver's cheap passes put it in (the very field HipBackend::set_cheap sets).  Sc = 0 clears it: the passes are exact again.
 * fpca_missing_mode keeps reporting the route of the exact passes.  fpca_pca clears the setting: the solver's backend object sets the
 * field for its own passes and leaves it at 0 when it goes (~HipBackend).
 * FPCA_EINVAL, with a message that names the reason, unless the context runs both products in the exact-integer arithmetic and Sc is 0
 * or 2 <= Sc < the slice count the context was created with.  In the product build it returns FPCA_EINVAL with a message that says so
 * and does nothing: no switch changes what it computes. */
int fpca_debug_set_pass_slices(fpca_ctx *ctx, int Sc);

#ifdef __cplusplus
}
#endif
#endif /* FPCA_DEBUG_H */
