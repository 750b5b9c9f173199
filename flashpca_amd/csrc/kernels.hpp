// kernels.hpp -- launch wrappers of the hand-written gfx950 kernels; every section names the file that defines its wrappers.
// All pointers are DEVICE pointers; every launch is asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace fpca {
namespace kern {

// ---- upload path (kernels.hip) ----
// back-to-back records of np bytes -> rows of `pitch` bytes
void repitch(const uint8_t *src, uint64_t np, uint64_t nrec, uint8_t *dst, size_t pitch, hipStream_t stream);
// rewrite the pad bits of the last valid byte of every record to the "missing" code (N % 4 != 0)
void fix_last_byte(uint8_t *packed, size_t pitch, uint64_t np, int valid_in_last, uint64_t P_g, hipStream_t stream);
// ---- record gather (snp_subset.hip) ----
// dst[j][:] = src[idx[j]][:] over `pitch` bytes (a multiple of 16) for j < nrec; dst has the same pitch,
// nothing at or after record nrec is written
void gather_records(const uint8_t *src, size_t pitch, const uint32_t *idx, uint64_t nrec, uint8_t *dst, hipStream_t stream);
// ---- LD band (ld_band.hip) ----
// ld_totals: tot[rec][4] = (sum x, sum x^2, codes "01" = missing calls + pad samples, 0) over the `pitch` bytes
// of records [0, nrec).  ld_band: every pair i in [i0, i0 + ni), j in (i, min(i + span, jend - 1)] of records of `packed`; r2 != null:
// r2[(i - i0) * span + (j - i - 1)] = the statistic (fp64); else bit (j - i - 1) of the row of `words` uint32 words of record i - i0 is
// OR-ed into bits (zeroed by the caller) when the statistic is above thr.  npad = 4 pitch - N; jend <= records allocated.
void ld_totals(const uint8_t *packed, size_t pitch, uint64_t nrec, uint32_t *tot, hipStream_t stream);
void ld_band(const uint8_t *packed, size_t pitch, const uint32_t *tot, uint32_t npad, uint64_t i0, uint64_t ni, uint64_t jend, uint32_t span,
             double *r2, uint32_t *bits, uint32_t words, double thr, bool force_general, hipStream_t stream);

// ---- statistics, the fp64 / fp32 GEMMs, the dense path, K4 helpers, generator and probes (kernels.hip) ----
// K1: per-SNP code counts -> mean, sd, lookup table (by raw PLINK code), sum of squares
//   lut [P_pad][4], mean/sd/sumsq [P_pad]; rows >= P_g untouched (must be pre-zeroed)
void bed_stats(const uint8_t *packed, size_t pitch, uint64_t N, uint64_t P_g, int stand_method, double *lut,
               double *mean, double *sd, double *sumsq, uint32_t *nmiss /* per-SNP missing calls, or null */, hipStream_t stream);
// lookup table from preloaded mean/sd (projection path, data.cpp:293-320)
void lut_from_meansd(const double *mean, const double *sd, uint64_t P_g, double *lut, hipStream_t stream);

// K2: Tpart[split][P_pad][b] = X^T B over the split's sample chunks.   b = 16*NT, NT in 1..4
//   B: [N_pad][b] row-major.  nsplit==1 writes the final T directly.  fp32: v_mfma_f32 products / fp32 sums over at most 512 samples (4 chunks),
//   accumulation folded into fp64 accumulators (FPCA_ACCUM_FP32), else everything fp64.
void xt_b(const uint8_t *packed, size_t pitch, const double *lut, const double *B, double *Tpart, uint64_t N_pad,
          uint64_t P_pad, int b, int nsplit, bool fp32, hipStream_t stream);
// K3: Ypart[split][N_pad][b] = X T over the split's SNP chunks.  T: [P_pad][b] row-major
void x_t(const uint8_t *packed, size_t pitch, const double *lut, const double *T, double *Ypart, uint64_t N_pad,
         uint64_t P_pad, int b, int nsplit, bool fp32, hipStream_t stream);
// out[i] = sum_s part[s*count + i]   (deterministic split-K combine)
void reduce_sum(const double *part, double *out, uint64_t count, int nsplit, hipStream_t stream);

// heuristics (host): number of splits for K2 / K3 given the problem and the chip (256 CUs, 2 WGs/CU)
int xt_b_splits(uint64_t N_pad, uint64_t P_pad, int b, bool fp32);
int x_t_splits(uint64_t N_pad, uint64_t P_pad, int b, bool fp32);
// what a launch with `nsplit` splits hands its kernel: chunks of the reduction in all, and chunks per split (workgroup row y owns
// chunks [y cps, min((y + 1) cps, total)) -- a short or empty range stores a short sum or a plane of zeros).  The launchers take
// their numbers from these, and so does fpca_debug_fp_plan.
struct SplitChunks {
   int total, per_split;
};
SplitChunks xt_b_chunks(uint64_t N_pad, int b, int nsplit);
SplitChunks x_t_chunks(uint64_t P_pad, int b, int nsplit, bool fp32);

// Dense (in-memory fp64 matrix) path: Xd [P_pad][N_pad] fp64, one row per column of the caller's N x P matrix
// util.cpp:24-192 in place (method 0 none, 1 sd, 2 binom, 3 binom2, 4 center; NaN = missing); mean/sd/sumsq [P_pad]
void dense_standardise(double *Xd, uint64_t N_pad, uint64_t N, uint64_t P_g, int method, double *mean, double *sd,
                       double *sumsq, hipStream_t stream);
int xt_b_dense_splits(uint64_t N_pad, uint64_t P_pad);
int x_t_dense_splits(uint64_t N_pad, uint64_t P_pad);
SplitChunks xt_b_dense_chunks(uint64_t N_pad, int nsplit);
SplitChunks x_t_dense_chunks(uint64_t P_pad, int nsplit);
void xt_b_dense(const double *Xd, const double *B, double *Tpart, uint64_t N_pad, uint64_t P_pad, int b, int nsplit,
                hipStream_t stream);
void x_t_dense(const double *Xd, const double *T, double *Ypart, uint64_t N_pad, uint64_t P_pad, int b, int nsplit,
               hipStream_t stream);

// K4 helpers on row-major [N_pad][b] blocks ------------------------------------------------------------
// part[4*split + wave][q][b][b] (row-major p,c) = A_q^T W over the rows of one wave of split `split` (gram_splits(N_pad,
// rows) workgroups of `rows` = gram_rows(N_pad, nq, b) rows each); `blocks` = device array of nq pointers
void gram(const double *const *blocks, int nq, const double *W, double *part, uint64_t N_pad, int b, int rows, hipStream_t stream);
int gram_rows(uint64_t N_pad, int nq, int b);
int gram_splits(uint64_t N_pad, int rows);
// Out = (Init ? Init : 0) + sum_q A_q C_q,   C: [nq][b][b] row-major (C_q[p][c]); Out may alias Init or any A_q
// gram_part non-null (only where block_gemm_gram_planes(N_pad, b) > 0): the launch also leaves that many partial planes [b][b] of
// Out' Out there (sum them with reduce_sum)
void block_gemm(const double *const *blocks, int nq, const double *C, const double *Init, double *Out, uint64_t N_pad,
                int b, hipStream_t stream, double *gram_part = nullptr);
int block_gemm_gram_planes(uint64_t N_pad, int b);
// Out = Init + sum_q A_q C_q, and from the same pass over the basis G_q = A_q' Out (q < nq), G_nq = Out' Out: update_gram_planes()
// partial planes [nq + 1][b][b] in gpart (0 planes: no fused kernel for this shape -- 16 columns, nq <= 28 only)
int update_gram_planes(uint64_t N_pad, int nq, int b);
void update_gram(const double *const *blocks, int nq, const double *C, const double *Init, double *Out, uint64_t N_pad, int b, double *gpart,
                 hipStream_t stream);
// uniform(-0.5, 0.5) entries for rows < N, zero for rows in [N, N_pad)
void fill_random(double *blk, uint64_t N, uint64_t rows, int b, uint64_t seed, hipStream_t stream, uint64_t row0 = 0);
// *out_bits = max(*out_bits, bits of max |a - scale b|) over n doubles (NaN counts as +inf); out_bits zeroed by the caller
void max_abs_diff(const double *a, const double *b, double scale, uint64_t n, unsigned long long *out_bits, hipStream_t stream);
// row-major [N_pad][b] block <-> column-major N x ncols (ld) device staging buffer
void block_to_colmajor(const double *blk, uint64_t N, int b, int ncols, double *out, uint64_t ld, hipStream_t stream);
void colmajor_to_block(const double *in, uint64_t ld, uint64_t N, uint64_t N_pad, int b, int ncols, double *blk,
                       hipStream_t stream);
// T [P_pad][b] row-major -> column-major P_g x ncols, scaled per column
void t_to_colmajor(const double *T, uint64_t P_g, int b, int ncols, const double *colscale, double *out, uint64_t ld,
                   hipStream_t stream);
void colmajor_to_t(const double *in, uint64_t ld, uint64_t P_g, uint64_t P_pad, int b, int ncols, double *T,
                   hipStream_t stream);

// synthetic genotype generator (synth.hpp model), one workgroup per SNP record
//   maf_model 0: ancestral frequency uniform in [0.05, 0.95); 1: rare-variant spectrum 0.001 + 0.499 u^3
//   missing_model 0: every call missing with probability miss_thr / 65536; 1: concentrated in a fraction conc_fp / 65536 of
//   the SNPs (10-30 % of their calls), the others at most 0.1 %; 2: per-SNP rates log-normal, median med_q32 (0.32 fixed point),
//   log2-sd sig2_fp (16.16)  (synth.hpp)
void synth_generate(uint8_t *packed, size_t pitch, uint64_t N, uint64_t snp_begin, uint64_t P_g, uint64_t seed,
                    int n_pop, uint32_t fst_fp, uint32_t miss_thr, hipStream_t stream, int maf_model = 0, int missing_model = 0,
                    uint32_t conc_fp = 0, uint64_t med_q32 = 0, uint32_t sig2_fp = 0);

// diagnostic: D(16x16) = A(16x4) B(4x16) through v_mfma_f64_16x16x4_f64 with this file's operand mapping
void mfma_layout_probe(const double *A, const double *B, double *D, hipStream_t stream);

// issue-rate ceiling of the FP64 MFMA (TFLOP/s) with `waves_per_simd` resident waves per SIMD
double mfma_peak_tflops(int waves_per_simd, int iters, int pattern, hipStream_t stream);

// ---- exact-integer int8-sliced path (kernels_i8.hip) ----
// one int8 operand cut from an fp64 matrix V[rows_pad][b]: Q[S*b][rows_pad] digits of V * rowscale[row], weights colw,
// optional exact column sums; maxbits = per-column max |V * rowscale| as double bit patterns (input of i8_slice)
constexpr int I8_SHARDS = 8, I8_CS_STRIDE = 640; // accumulator sharding (see kernels_i8.hip)
struct SliceOp {
   const double *rowscale;      // null: none
   unsigned long long *maxbits; // [I8_SHARDS][64]
   int8_t *Q;
   double *colw;       // [gemm_i8_nsc_pad(S, b)]
   long long *colsum;  // [I8_SHARDS][I8_CS_STRIDE] or null; accumulated with atomics: zero it first
   double *copy64;     // optional: the scaled operand itself, row-major [rows][b] (what the sparse gathers of the missing-call
   float *copy32;      // route read: no per-entry row factor; fp32, column-scaled, when the slices carry no more than 30 bits anyway)
};
void i8_colmax(const double *V, uint64_t rows, int b, int nops, const SliceOp *ops, hipStream_t stream); // maxbits must be zeroed
void i8_slice(const double *V, uint64_t rows_pad, uint64_t rows, int b, int S, int nops, const SliceOp *ops, hipStream_t stream);
// row-sharded operand exchange: slices of a rank's own rows in a row-major layout, and what every rank makes of the gathered rows
void i8_maxbits_fold(const unsigned long long *bits, double *out64, hipStream_t stream);      // [I8_SHARDS][64] -> 64 doubles
void i8_maxbits_set(const double *all, int G, unsigned long long *bits, hipStream_t stream);   // max over [G][64] -> shard 0
void i8_slice_rows(const double *V, uint64_t rows, int b, int S, const SliceOp &op, int8_t *Qrm, hipStream_t stream); // -> Qrm[rows][S*b], op.colw
// -> op.Q, op.colsum; optionally the scaled operand itself (rows < rows_valid) for the sparse gathers: fp32 (copy32) or fp64 (copy64)
void i8_unpack_slices(const int8_t *Qrm, uint64_t rows_pad, int b, int S, const SliceOp &op, hipStream_t stream, uint64_t rows_valid = 0,
                      float *copy32 = nullptr, double *copy64 = nullptr);
void i8_dequant_rows(const int8_t *Qrm, uint64_t rows, int b, int S, const SliceOp &op, float *copy32, double *copy64, hipStream_t stream);
// Band-tiled layout of a packed copy that only the int8 GEMM streams (the sample-major copy, and the SNP-major copy made for K2).
// Size, pitch and the offset of a band of 32 rows (32 * pitch bytes) are those of the row-major layout; inside a band the 32 rows x
// 64 bytes of chunk c (256 codes per row) are 2 KB contiguous, ordered so that the 16-byte piece lane (row i, k-half kh) of the
// GEMM wants as its h-th load sits at (h * 64 + kh * 32 + i) * 16: one global_load_dwordx4 of a wave reads 1 KB = 8 whole lines.
// Byte offset of the 16-byte piece q of row r (piece q = bytes [16 q, 16 q + 16) of the record; pitch a multiple of 64):
__host__ __device__ inline size_t packed_piece_offset(uint64_t r, uint64_t q, size_t pitch, bool tiled)
{
   if (!tiled) return (size_t)(r * pitch + q * 16);
   const uint64_t c = q >> 2, kh = (q >> 1) & 1, h = q & 1;
   return (size_t)((r >> 5) * 32 * pitch + c * 2048 + (h * 64 + kh * 32 + (r & 31)) * 16);
}
int gemm_i8_nsc_pad(int S, int b); // rows of a Q operand: S*b rounded up to the 256-column workgroup tile
size_t gemm_i8_workspace_doubles(uint64_t rows_pad, uint64_t k_pad, int S, int b, bool two);
// every k_gemm_i8 instance there is as (two operands, mode, nt, half tile, tile rows, band-tiled): writes min(count, cap), returns the count
int gemm_i8_instances(int (*out)[6], int cap);
// what one workgroup of a kernel holds of a CU: its waves, the registers of a lane (VGPRs + AGPRs, as the compiler asks for them) and its LDS
struct CuFootprint {
   int waves, vgprs, lds_bytes;
};
// of the k_gemm_i8 instance gemm_i8 launches for these arguments (the registers from the loaded code object, asked once per instance)
CuFootprint gemm_i8_footprint(uint64_t rows_pad, int S, int b, bool two, int mode, bool e_only, bool tiled);
// out[rows_pad][b] = recombined ( (G.M) Qg' , M Qm' ); mean/sd non-null: K2 flavour (per-row standardisation)
void gemm_i8(const uint8_t *packed, size_t pitch, const int8_t *Qg, const int8_t *Qm, const double *wg, const double *wm,
             const long long *colsum_m, const double *mean, const double *sd, double *out, double *ws, uint64_t rows_pad, uint64_t k_pad,
             uint64_t rows_valid, int mode /* 0 full, 1 skip E blocks without a missing genotype, 2 G.M alone */,
             const double *eplane /* with mode 2: E'Q [rows_pad][b] from sparse_rows_sum, or null if nothing is missing */, int b, int S,
             const SliceOp *next_ops, hipStream_t stream, hipEvent_t *gemm_events = nullptr, hipEvent_t before_combine = nullptr,
             bool e_only = false /* mode 2 only: multiply the missing-indicator matrix E instead of G.M; out = E Q */,
             bool tiled = false /* `packed` is in the band-tiled layout (two-matrix and G.M-alone kernels) */);
void i8_rowscales(const double *mean, const double *sd, uint64_t P_g, uint64_t P_pad, double *inv_sd, double *mu_inv_sd,
                  hipStream_t stream);
void transpose_packed(const uint8_t *in, size_t pitch_in, uint64_t N_pad, uint64_t P_pad, uint8_t *out, size_t pitch_out,
                      hipStream_t stream, bool tiled = false /* write the band-tiled layout */);
// out = the band-tiled arrangement of the row-major records in[rows][pitch] (rows a multiple of 32, pitch of 64)
void tile_packed(const uint8_t *in, size_t pitch, uint64_t rows, uint8_t *out, hipStream_t stream);
// what the bare int8 MFMA stream multiplies: two register sets per operand port, index 0, 1 = the sets of source A, 2, 3 = of source B
enum { I8_FILL_ZERO = 0, I8_FILL_RANDOM = 1 /* hashed bytes */, I8_FILL_GENO = 2 /* bytes 0, 1, 2, a third each */ };
struct I8PeakFill {
   uint32_t seed[4]; // hash seed of each set (equal seeds and kinds: equal sets, nothing changes between instructions)
   uint32_t kind[4]; // I8_FILL_*
   int order;        // 0: A alternates its sets every instruction, B holds one for two; 1: A holds, B alternates
};
double mfma_i8_peak_tops(int waves_per_simd, int iters, const I8PeakFill &fill, hipStream_t stream);
void mfma_i8_probe(const int8_t *A, const int8_t *Bt, int *D, hipStream_t stream);
void mfma_i8_ports(int shape /* 32 | 16 */, bool exchanged, const int8_t *A, const int8_t *Bt, int *D, hipStream_t stream);

// ---- missing calls of the exact-integer path: index lists, gather-sums, row shuffles (missing_kernels.hip) ----
// the hybrid missing-indicator route's row shuffles
void gather_packed_rows(const uint8_t *src, size_t pitch, const uint32_t *idx, uint32_t nidx, uint32_t rows_out, uint8_t *dst, hipStream_t stream);
void patch_missing_rows(uint8_t *packed, size_t pitch, const uint32_t *idx, uint32_t nidx, hipStream_t stream);
void scatter_packed_rows(const uint8_t *src, size_t pitch, const uint32_t *idx, uint32_t nidx, uint8_t *packed, hipStream_t stream);
void gather_scaled_rows(const double *V, const double *scale, const uint32_t *idx, uint32_t nidx, uint64_t rows_out, int b, double *dst, hipStream_t stream);
void scatter_rows(const double *src, const uint32_t *idx, uint32_t nidx, int b, double *dst, hipStream_t stream);
// index lists of the missing calls of 2-bit records (positions < ncols), and the gather-sum over them
// (tiled: the records are in the band-tiled layout)
void count_missing(const uint8_t *packed, size_t pitch, uint64_t ncols, uint64_t nrec, uint32_t *cnt, hipStream_t stream, bool tiled = false);
void fill_missing(const uint8_t *packed, size_t pitch, uint64_t ncols, uint64_t nrec, const uint32_t *ptr, uint32_t *idx, hipStream_t stream,
                  bool tiled = false);
void sparse_rows_sum(const uint32_t *ptr, const uint32_t *idx, const double *V, const double *rowscale, int b, uint64_t nrec,
                     uint64_t rows_out, double *out, hipStream_t stream, const double *init = nullptr /* [rows_out][b] added to the sums */,
                     bool short_lists = false /* many short lists (per sample): the batched index reads */,
                     double avg_len = 0 /* entries per list, if known: a dozen or so takes the several-rows-per-wave kernel */,
                     unsigned block_limit = 0 /* most blocks of the one-wave-per-row kernels (sparse_rows_sum_blocks_beside); 0: no limit */);
// the same over the fp32 rows k_slice leaves (SliceOp::copy32: each column scaled into (-2, 2) by its slice exponent; colw = that
// operand's slice weights, which carry the exponent back)
void sparse_rows_sum_f32(const uint32_t *ptr, const uint32_t *idx, const float *V, const double *colw, int b, uint64_t nrec, uint64_t rows_out,
                         double *out, hipStream_t stream, const double *init = nullptr, bool short_lists = false, double avg_len = 0,
                         unsigned block_limit = 0);
// which kernel the two launches above take for these arguments (rowscale: a per-row factor is given): 1 one wave per row, 2 the same
// with batched index reads, 3 several rows per wave
int sparse_rows_sum_variant(int b, bool rowscale, bool short_lists, double avg_len);
// The grid of a gather that runs on the side stream beside a GEMM: as many 256-thread blocks (a wave per SIMD) as stay resident on `ncu`
// CUs next to the workgroups of `gemm` that share a CU -- what is left of the 8 wave slots and 512 registers of a SIMD (allocated in
// eights).  Such a grid is placed once and queues nothing: a CU that a GEMM workgroup leaves is not refilled with gather blocks before
// the next one arrives.  At least one block per CU, also where nothing is left.  Pure: no device involved.
unsigned gather_blocks_beside(const CuFootprint &gemm, int gather_vgprs, int ncu);
// blocks of a launch of the one-wave-per-row kernels over rows_out rows: four rows a block up to 65536 blocks, and no more than
// block_limit (0: no limit -- an inline launch)
unsigned sparse_rows_sum_grid(uint64_t rows_out, unsigned block_limit);
// ... for the kernel sparse_rows_sum / sparse_rows_sum_f32 take for these arguments, on the current device; 0 (no limit) for the
// several-rows-per-wave kernel, whose lists are too short to be worth a side stream
unsigned sparse_rows_sum_blocks_beside(const CuFootprint &gemm, int b, bool f32, bool rowscale, bool short_lists, double avg_len);

} // namespace kern
} // namespace fpca
